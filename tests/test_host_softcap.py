"""CPU tests of the logit soft-capping boundary: include/mi355fa_softcap.h declares exactly four entry points and
MI355FA_ERR_SOFTCAP, libmi355fa.so and the ctypes tables export them, bad arguments are refused before anything is
launched, the Python surface is as documented, and the fp64 reference of tests/attn_ref.py (closed-form gradients with
the (1 - t^2) factor) agrees with torch.autograd through an eager implementation.  No compute is launched on a GPU here."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from conftest import ROOT
import attn_ref as sr
import variantcheck as vck

NAMES = ["fa_bwd_dkv_softcap", "fa_bwd_dq_softcap", "fa_fwd_kvcache_softcap", "fa_fwd_softcap"]
BAD_CAPS = (0.0, -0.0, -30.0, math.nan, math.inf, -math.inf)


BASES = (("fa_fwd_softcap", "fa_fwd_gqa"), ("fa_bwd_dq_softcap", "fa_bwd_dq_gqa"), ("fa_bwd_dkv_softcap", "fa_bwd_dkv_gqa"),
         ("fa_fwd_kvcache_softcap", "fa_fwd_kvcache"))


def test_companion_header_declares_the_four_softcap_entry_points():
    txt, body, names = vck.header_functions(os.path.join(ROOT, "include", "mi355fa_softcap.h"))
    assert names == NAMES
    assert '#include "mi355fa_kvcache.h"' in txt
    assert re.search(r"#define\s+MI355FA_ERR_SOFTCAP\s+\(-10\)", txt)
    for name in NAMES:   # the cap follows the scale
        sig = body[body.index(name + "("):]
        assert re.search(r"float scale,\s*float softcap,\s*int window_left", sig[:sig.index(";")]), name
    # mi355fa.h is untouched: same ABI version, and it does not know the new calls
    base = open(os.path.join(ROOT, "include", "mi355fa.h")).read()
    assert "softcap" not in base and re.search(r"#define\s+MI355FA_ABI_VERSION\s+7\b", base)


def test_library_and_ctypes_tables_export_them():
    import _mi355fa as fa
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in fa.SOFTCAP_SIGNATURES and name in fa.ALL_SIGNATURES, name
        assert name not in fa.SIGNATURES, name
    assert fa.ERR_SOFTCAP == -10
    assert fa.lib.fa_abi_version() == 7
    # the _gqa / kvcache signatures with one float (softcap) after the scale
    vck.check_spliced_signatures(fa.SOFTCAP_SIGNATURES, [(n, fa.SIGNATURES[b]) for n, b in BASES], [ctypes.c_float])


def _calls(p):
    """name -> f(scale, (cap,), H, H_kv, wl, opts), B = 1"""
    import _mi355fa as fa
    return vck.entry_calls(fa.lib, NAMES, p, B=1)


@pytest.mark.parametrize("cap", BAD_CAPS, ids=["0", "-0", "-30", "nan", "inf", "-inf"])
def test_bad_softcap_is_refused_before_launch(cap):
    import _mi355fa as fa
    _buf, p = vck.aligned_ptr()
    for name, f in _calls(p).items():
        assert f(0.125, (cap,), 4, 2, -1, None) == fa.ERR_SOFTCAP, name
        err = fa.lib.fa_last_error()
        assert name.encode() in err and b"softcap" in err, (name, err)


def test_other_bad_arguments_keep_their_own_codes():
    _buf, p = vck.aligned_ptr()
    for name, texts in vck.check_common_refusals(_calls(p), (30.0,)).items():
        assert b"H_kv" in texts["group"], name


def test_python_surface():
    import My_FlashAttention_optimized as M
    import _mi355fa_torch as ext
    assert str(inspect.signature(M.flash_attention_softcap)) == (
        "(Q, K, V, softcap, is_causal=False, window_size=(-1, -1), softmax_scale=None, cu_seqlens_q=None, "
        "cu_seqlens_k=None, max_seqlen_q=None, max_seqlen_k=None)")
    assert str(inspect.signature(M.flash_attention_kvcache_softcap)) == (
        "(q, k_cache, v_cache, cache_seqlens, softcap, k_new=None, v_new=None, is_causal=False, window_size=(-1, -1), "
        "softmax_scale=None, return_lse=False)")
    # the existing entry points keep their signatures
    assert str(inspect.signature(M.flash_attention)) == "(Q, K, V, is_causal=False)"
    assert str(inspect.signature(M.flash_attention_gqa)) == (
        "(Q, K, V, is_causal=False, window_size=(-1, -1), cu_seqlens_q=None, cu_seqlens_k=None, "
        "max_seqlen_q=None, max_seqlen_k=None)")
    assert hasattr(M, "FlashAttentionSoftcapFunction")
    for name in ("flash_attention_softcap", "softcap_forward_launch", "softcap_backward_launch", "kvcache_softcap_forward"):
        assert hasattr(ext, name), name
    for fn in (M.flash_attention_softcap, M.flash_attention_kvcache_softcap):
        doc = " ".join(fn.__doc__.split())
        for phrase in ("tanh(scale", "finite and > 0", "aligned", "LSE = -inf"):
            assert phrase in doc, (fn.__name__, phrase)
    doc = " ".join(M.flash_attention_softcap.__doc__.split())
    for phrase in ("(1 - t_ij^2)", "top-left aligned", "Dropout is not supported"):
        assert phrase in doc, phrase
    assert "bottom-right aligned" in " ".join(M.flash_attention_kvcache_softcap.__doc__.split())


def test_python_refuses_a_bad_cap_or_scale():
    import My_FlashAttention_optimized as M
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    Q, K = mk(1, 4, 16, 64), mk(1, 2, 16, 64)
    for cap in (0.0, -5.0, math.inf):
        with pytest.raises(AssertionError, match="softcap"):
            M.flash_attention_softcap(Q, K, K, cap)
        with pytest.raises(AssertionError, match="softcap"):
            M.flash_attention_kvcache_softcap(Q, K, K, torch.zeros(1, dtype=torch.int32), cap)
    for sc in (0.0, -0.1):
        with pytest.raises(AssertionError, match="softmax_scale"):
            M.flash_attention_softcap(Q, K, K, 30.0, softmax_scale=sc)
    with pytest.raises(AssertionError):
        M.flash_attention_softcap(Q, K, K, 30.0, is_causal=True, window_size=(-1, 4))


def test_cpp_binding_checks():
    """The C++ functions' own checks (no device needed): good calls stop only at the device check."""
    import _mi355fa_torch as ext
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    Q, K = mk(2, 8, 16, 64), mk(2, 2, 16, 64)
    with pytest.raises(AssertionError, match="device tensors"):
        ext.flash_attention_softcap(Q, K, K, 30.0, -1, 0)
    with pytest.raises(AssertionError, match="device tensors"):
        ext.softcap_forward_launch(Q, K, K, 30.0, -1, 0, 0.1)
    for cap in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(AssertionError, match="softcap"):
            ext.flash_attention_softcap(Q, K, K, cap, -1, 0)
        with pytest.raises(AssertionError, match="softcap"):
            ext.kvcache_softcap_forward(Q, K, K, torch.zeros(2, dtype=torch.int32), cap)
    with pytest.raises(AssertionError, match="softmax_scale"):
        ext.flash_attention_softcap(Q, K, K, 30.0, -1, 0, -0.5)
    with pytest.raises(AssertionError, match="multiple"):
        ext.flash_attention_softcap(Q, mk(2, 3, 16, 64), mk(2, 3, 16, 64), 30.0, -1, 0)


CASES = [  # B, H, H_kv, S_q, S_k, D, cap, scale, (wl, wr), bottom-right L (None: training)
    (2, 4, 2, 9, 13, 8, 5.0, 1.0, (-1, -1), None),
    (1, 4, 1, 12, 12, 8, 30.0, 144 ** -0.5 * 12, (-1, 0), None),
    (2, 2, 2, 11, 17, 16, 5.0, 0.25, (3, 0), None),
    (1, 6, 3, 10, 10, 8, 50.0, 8.0, (2, 2), None),
    (1, 4, 2, 3, 20, 8, 5.0, 0.5, (6, 0), 14),
    (2, 6, 2, 9, 13, 8, 5.0, 0.5, (-1, 0), None),     # g = 3
    (2, 7, 1, 5, 20, 8, 5.0, 0.5, (6, 2), 14),        # g = 7, multi-query, decoding with keys right of the queries
]


@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_fp64_reference_agrees_with_autograd(case):
    """tests/attn_ref.py's closed-form gradients against autograd through the eager implementation (fp64, CPU)."""
    B, H, Hkv, Sq, Sk, D, cap, scale, (wl, wr), L = case
    # scores of about 0.7 x the cap: far into tanh's curve, so that the cap matters (checked at the end)
    Q, K, V, _, vis, gt = vck.reference_agrees_with_autograd(case[:6], scale, (wl, wr), L, dict(cap=cap),
                                                             amp=0.7 * cap / (scale * D ** 0.5))
    # LSE = logsumexp of the visible capped scores; rows without a visible key: -inf, O = 0
    u = cap * torch.tanh(scale * (Q @ K.repeat_interleave(H // Hkv, 1).transpose(-1, -2)) / cap)
    lse = torch.logsumexp(u.masked_fill(~vis, -torch.inf), -1)
    assert torch.equal(torch.isneginf(lse), torch.isneginf(gt["LSE"]))
    fin = torch.isfinite(lse)
    assert torch.allclose(lse[fin], gt["LSE"][fin], rtol=0, atol=1e-12)
    assert (gt["O"][~fin] == 0).all() and (gt["dQ"][~fin] == 0).all()
    # the cap matters at these shapes: the uncapped LSE is far away, and at the small caps O too (at cap 50 both softmaxes
    # are nearly one-hot on the same key)
    unc = sr.attention_fp64(Q, K, V, None, scale, vis)
    assert (unc["LSE"][fin] - gt["LSE"][fin]).abs().max() > 1.0
    if cap <= 30:
        assert (unc["O"] - gt["O"]).norm() / gt["O"].norm() > 0.1
