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

NAMES = ["fa_bwd_dkv_softcap", "fa_bwd_dq_softcap", "fa_fwd_kvcache_softcap", "fa_fwd_softcap"]
BAD_CAPS = (0.0, -0.0, -30.0, math.nan, math.inf, -math.inf)


def _header():
    return open(os.path.join(ROOT, "include", "mi355fa_softcap.h")).read()


def _header_functions():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(fa_[a-z_]+)\s*\(", txt)))


def test_companion_header_declares_the_four_softcap_entry_points():
    assert _header_functions() == NAMES
    txt = _header()
    assert '#include "mi355fa_kvcache.h"' in txt
    assert re.search(r"#define\s+MI355FA_ERR_SOFTCAP\s+\(-10\)", txt)
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
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
    for name, base in (("fa_fwd_softcap", "fa_fwd_gqa"), ("fa_bwd_dq_softcap", "fa_bwd_dq_gqa"),
                       ("fa_bwd_dkv_softcap", "fa_bwd_dkv_gqa"), ("fa_fwd_kvcache_softcap", "fa_fwd_kvcache")):
        a, b = fa.SOFTCAP_SIGNATURES[name][1], fa.SIGNATURES[base][1]
        i = b.index(ctypes.c_float)
        assert a == b[:i + 1] + [ctypes.c_float] + b[i + 1:], name


def _ptr():
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _calls(p):
    """name -> f(scale, cap, H, H_kv, wl, opts): one otherwise well-formed call per entry point (B = 1, S = 8, D = 64)."""
    import _mi355fa as fa
    L = fa.lib
    B, S, D, dt = 1, 8, 64, fa.BF16
    return {
        "fa_fwd_softcap": lambda s, c, H, Hkv, wl, o: L.fa_fwd_softcap(p, p, p, p, p, B, H, Hkv, S, S, D, dt, s, c, wl, 0, o, None),
        "fa_bwd_dq_softcap": lambda s, c, H, Hkv, wl, o: L.fa_bwd_dq_softcap(p, p, p, p, p, p, p, p, B, H, Hkv, S, S, D, dt, s, c,
                                                                             wl, 0, o, None),
        "fa_bwd_dkv_softcap": lambda s, c, H, Hkv, wl, o: L.fa_bwd_dkv_softcap(p, p, p, p, p, p, p, p, B, H, Hkv, S, S, D, dt, s,
                                                                               c, wl, 0, o, None),
        "fa_fwd_kvcache_softcap": lambda s, c, H, Hkv, wl, o: L.fa_fwd_kvcache_softcap(
            p, p, p, None, None, p, p, p, p, 1 << 12, B, H, Hkv, 1, S, 0, D, dt, s, c, wl, 0, o, None),
    }


@pytest.mark.parametrize("cap", BAD_CAPS, ids=["0", "-0", "-30", "nan", "inf", "-inf"])
def test_bad_softcap_is_refused_before_launch(cap):
    import _mi355fa as fa
    _buf, p = _ptr()
    for name, f in _calls(p).items():
        assert f(0.125, cap, 4, 2, -1, None) == fa.ERR_SOFTCAP, name
        err = fa.lib.fa_last_error()
        assert name.encode() in err and b"softcap" in err, (name, err)


def test_other_bad_arguments_keep_their_own_codes():
    import _mi355fa as fa
    _buf, p = _ptr()
    drop = fa.Opts.make(p_drop=0.25, seed=1)
    for name, f in _calls(p).items():
        for s in (0.0, -0.125, math.nan, math.inf):
            assert f(s, 30.0, 4, 2, -1, None) == -2, (name, s)           # a bad scale: MI355FA_ERR_SHAPE
            assert b"scale" in fa.lib.fa_last_error()
        assert f(0.125, 30.0, 4, 2, -2, None) == fa.ERR_WINDOW, name       # a window below -1
        assert f(0.125, 30.0, 4, 0, -1, None) == fa.ERR_GROUP, name        # H_kv = 0
        assert f(0.125, 30.0, 6, 4, -1, None) == fa.ERR_GROUP, name        # H % H_kv != 0
        assert b"H_kv" in fa.lib.fa_last_error()
        assert f(0.125, 30.0, 4, 2, -1, ctypes.byref(drop)) == -2, name     # dropout: MI355FA_ERR_SHAPE
        assert b"dropout" in fa.lib.fa_last_error()


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
    g = torch.Generator().manual_seed(sum(case[:6]))
    # scores of about 0.7 x the cap: far into tanh's curve, so that the cap matters (checked at the end)
    Q = torch.randn(B, H, Sq, D, generator=g, dtype=torch.float64) * (0.7 * cap / (scale * D ** 0.5))
    K, V = (torch.randn(B, Hkv, Sk, D, generator=g, dtype=torch.float64) for _ in range(2))
    dO = torch.randn(B, H, Sq, D, generator=g, dtype=torch.float64)
    vis = sr.visible(Sq, Sk, wl, wr, "cpu", L=L)
    gt = sr.attention_fp64(Q, K, V, dO, scale, vis, cap=cap)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    o = sr.attention_eager(q, k, v, scale, vis, cap=cap)
    o.backward(dO)
    for n, t in (("O", o.detach()), ("dQ", q.grad), ("dK", k.grad), ("dV", v.grad)):
        assert torch.allclose(gt[n], t, rtol=1e-10, atol=1e-10), (n, (gt[n] - t).abs().max().item())
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
