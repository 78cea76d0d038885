"""CPU tests of the ALiBi boundary: include/mi355fa_alibi.h declares exactly four entry points and MI355FA_ERR_ALIBI,
libmi355fa.so and the ctypes tables export them, bad arguments are refused before anything is launched, the Python and
C++ surfaces check the slopes, alibi_slopes(H) gives the paper's slopes, and the fp64 reference of tests/attn_ref.py
agrees with torch.autograd through an eager implementation.  No compute is launched on a GPU here."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
import attn_ref as ar
import variantcheck as vck

NAMES = ["fa_bwd_dkv_alibi", "fa_bwd_dq_alibi", "fa_fwd_alibi", "fa_fwd_kvcache_alibi"]
BASES = (("fa_fwd_alibi", "fa_fwd_gqa"), ("fa_bwd_dq_alibi", "fa_bwd_dq_gqa"), ("fa_bwd_dkv_alibi", "fa_bwd_dkv_gqa"),
         ("fa_fwd_kvcache_alibi", "fa_fwd_kvcache"))


def test_companion_header_declares_the_four_alibi_entry_points():
    txt, body, names = vck.header_functions(os.path.join(ROOT, "include", "mi355fa_alibi.h"))
    assert names == NAMES
    assert '#include "mi355fa_kvcache.h"' in txt
    assert re.search(r"#define\s+MI355FA_ERR_ALIBI\s+\(-11\)", txt)
    for name in NAMES:   # the slopes follow the scale
        sig = body[body.index(name + "("):]
        assert re.search(r"float scale,\s*const float\* alibi_slopes,\s*long long slopes_batch_stride,\s*int window_left",
                         sig[:sig.index(";")]), name
    base = open(os.path.join(ROOT, "include", "mi355fa.h")).read()
    assert "alibi" not in base.lower() and re.search(r"#define\s+MI355FA_ABI_VERSION\s+7\b", base)


def test_library_and_ctypes_tables_export_them():
    import _mi355fa as fa
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in fa.ALIBI_SIGNATURES and name in fa.ALL_SIGNATURES, name
        assert name not in fa.SIGNATURES and name not in fa.SOFTCAP_SIGNATURES, name
    assert fa.ERR_ALIBI == -11
    assert fa.lib.fa_abi_version() == 7
    # the base signature with (const float*, long long) spliced in after the scale
    vck.check_spliced_signatures(fa.ALIBI_SIGNATURES, [(n, fa.SIGNATURES[b]) for n, b in BASES],
                                 [ctypes.c_void_p, ctypes.c_longlong])


def _calls(p):
    """name -> f(scale, (slopes, stride), H, H_kv, wl, opts), B = 2"""
    import _mi355fa as fa
    return vck.entry_calls(fa.lib, NAMES, p, B=2)


@pytest.mark.parametrize("stride", [-1, -4, 1, 3], ids=["-1", "-4", "1", "H-1"])
def test_bad_stride_is_refused_before_launch(stride):
    import _mi355fa as fa
    _buf, p = vck.aligned_ptr()
    for name, f in _calls(p).items():
        assert f(0.125, (p, stride), 4, 2, -1, None) == fa.ERR_ALIBI, name
        err = fa.lib.fa_last_error()
        assert name.encode() in err and b"slopes_batch_stride" in err, (name, err)


def test_null_and_misaligned_slopes_are_refused():
    import _mi355fa as fa
    _buf, p = vck.aligned_ptr()
    for name, f in _calls(p).items():
        assert f(0.125, (None, 0), 4, 2, -1, None) == -1, name          # MI355FA_ERR_NULL
        assert b"alibi_slopes" in fa.lib.fa_last_error()
        for off in (1, 2, 3):
            assert f(0.125, (p + off, 0), 4, 2, -1, None) == -5, name   # MI355FA_ERR_ALIGN
            assert b"alibi_slopes" in fa.lib.fa_last_error()
        # strides of 0 ((H,)), H and above ((B, H) with padding), and a 4-byte (not 16-byte) aligned pointer pass these
        # checks; the calls then stop at the first later check: a window below -1
        for st in (0, 4, 9):
            assert f(0.125, (p + 4, st), 4, 2, -2, None) == fa.ERR_WINDOW, (name, st)
        assert f(0.125, (p, 1 << 31), 4, 2, -1, None) == fa.ERR_ALIBI, name   # (B - 1) * stride beyond int


def test_other_bad_arguments_keep_their_own_codes():
    _buf, p = vck.aligned_ptr()
    for name, texts in vck.check_common_refusals(_calls(p), (p, 0)).items():
        if name != "fa_fwd_kvcache_alibi":
            assert b"ALiBi" in texts["dropout"], name


def test_python_surface():
    import My_FlashAttention_optimized as M
    import _mi355fa_torch as ext
    assert str(inspect.signature(M.flash_attention_alibi)) == (
        "(Q, K, V, alibi_slopes, is_causal=False, window_size=(-1, -1), softmax_scale=None, cu_seqlens_q=None, "
        "cu_seqlens_k=None, max_seqlen_q=None, max_seqlen_k=None)")
    assert str(inspect.signature(M.flash_attention_kvcache_alibi)) == (
        "(q, k_cache, v_cache, cache_seqlens, alibi_slopes, k_new=None, v_new=None, is_causal=False, "
        "window_size=(-1, -1), softmax_scale=None, return_lse=False)")
    for name in ("FlashAttentionAlibiFunction", "flash_attention_alibi_forward", "flash_attention_alibi_backward",
                 "alibi_slopes"):
        assert hasattr(M, name), name
    for name in ("flash_attention_alibi", "alibi_forward_launch", "alibi_backward_launch", "kvcache_alibi_forward"):
        assert hasattr(ext, name), name
    assert str(inspect.signature(M.flash_attention)) == "(Q, K, V, is_causal=False)"


@pytest.mark.parametrize("H, expect", [
    (8, [2.0 ** -(i + 1) for i in range(8)]),
    (12, [2.0 ** -(i + 1) for i in range(8)] + [2.0 ** -(0.5 + i) for i in range(4)]),
    (32, [2.0 ** (-(i + 1) / 4) for i in range(32)]),
    (40, [2.0 ** (-(i + 1) / 4) for i in range(32)] + [2.0 ** (-(2 * i + 1) / 8) for i in range(8)]),
])
def test_alibi_slopes_match_the_paper(H, expect):
    import My_FlashAttention_optimized as M
    s = M.alibi_slopes(H)
    assert s.dtype == torch.float32 and s.shape == (H,)
    assert torch.allclose(s.double(), torch.tensor(expect, dtype=torch.float64), rtol=1e-7, atol=0)


def _bad_slopes(H, B):
    """(slopes, message) pairs every checker refuses; the shapes are checked against B sequences of H heads"""
    ok = torch.ones(H)
    return [
        (ok.double(), "float32"),
        (ok.half(), "float32"),
        (torch.ones(H + 1), "shape"),
        (torch.ones(B + 1, H), "shape"),
        (torch.ones(1, 1, H), "shape"),
        (torch.ones(H, B).t(), "contiguous"),
        (torch.ones(H, requires_grad=True), "grad"),
    ]


def test_python_refuses_bad_slopes():
    """Python checks the slopes before anything else touches a device (CPU tensors here: the device check comes last)."""
    import My_FlashAttention_optimized as M
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    Q, K = mk(2, 4, 16, 64), mk(2, 2, 16, 64)
    sl = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(AssertionError, match="device"):
        M.flash_attention_alibi(Q, K, K, torch.ones(4, device="meta"))
    with pytest.raises(AssertionError, match="device"):
        M.flash_attention_kvcache_alibi(Q, K, K, sl, torch.ones(4, device="meta"))
    for s, msg in _bad_slopes(4, 2):
        with pytest.raises(AssertionError, match=msg):
            M.flash_attention_alibi(Q, K, K, s)
        with pytest.raises(AssertionError, match=msg):
            M.FlashAttentionAlibiFunction.apply(Q, K, K, s, -1, -1)
        with pytest.raises(AssertionError, match=msg):
            M.flash_attention_kvcache_alibi(Q, K, K, sl, s)
    with pytest.raises(AssertionError, match="softmax_scale"):
        M.flash_attention_alibi(Q, K, K, torch.ones(4), softmax_scale=-1.0)
    # varlen: B is the number of sequences
    cu = torch.tensor([0, 5, 9, 16], dtype=torch.int32)
    Qp, Kp = mk(16, 4, 64), mk(16, 2, 64)
    with pytest.raises(AssertionError, match="shape"):
        M.flash_attention_alibi(Qp, Kp, Kp, torch.ones(2, 4), cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=7,
                                max_seqlen_k=7)


def test_cpp_binding_checks():
    """The C++ functions' own checks (no device needed): the slopes are checked before Q's device, so CPU tensors reach
    each of them; well-formed CPU slopes stop at the slopes' device check."""
    import _mi355fa_torch as ext
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    Q, K = mk(2, 4, 16, 64), mk(2, 2, 16, 64)
    sl = torch.zeros(2, dtype=torch.int32)
    calls = (lambda s: ext.flash_attention_alibi(Q, K, K, s, -1, 0),
             lambda s: ext.alibi_forward_launch(Q, K, K, s, -1, 0, 0.1),
             lambda s: ext.alibi_backward_launch(Q, K, K, Q, Q, torch.zeros(2, 4, 16), s),
             lambda s: ext.kvcache_alibi_forward(Q, K, K, sl, s))
    for f in calls:
        for s, msg in _bad_slopes(4, 2) + [(torch.ones(4), "alibi_slopes must be a device tensor"),
                                           (torch.ones(2, 4), "alibi_slopes must be a device tensor")]:
            with pytest.raises(AssertionError, match=msg):
                f(s)
    with pytest.raises(AssertionError, match="softmax_scale"):
        ext.flash_attention_alibi(Q, K, K, torch.ones(4), -1, 0, -0.5)
    with pytest.raises(AssertionError, match="multiple"):
        ext.flash_attention_alibi(Q, mk(2, 3, 16, 64), mk(2, 3, 16, 64), torch.ones(4), -1, 0)


CASES = [  # B, H, H_kv, S_q, S_k, D, slope scale, scale, (wl, wr), bottom-right L (None: training), (B, H) slopes
    (2, 4, 2, 9, 13, 8, 1.0, 0.5, (-1, -1), None, False),
    (1, 4, 1, 12, 12, 8, 1.0, 0.35, (-1, 0), None, True),
    (2, 2, 2, 11, 17, 16, 4.0, 0.25, (3, 0), None, False),
    (1, 6, 3, 10, 10, 8, -0.5, 0.5, (2, 2), None, True),
    (2, 4, 2, 3, 20, 8, 1.0, 0.5, (6, 0), 14, True),
    (2, 6, 2, 9, 13, 8, 1.0, 0.5, (-1, 0), None, True),    # g = 3
    (2, 7, 1, 5, 20, 8, 1.0, 0.5, (6, 2), 14, True),       # g = 7, multi-query, decoding with keys right of the queries
]


@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_fp64_reference_agrees_with_autograd(case):
    """tests/attn_ref.py's closed-form gradients against autograd through the eager implementation (fp64, CPU)."""
    import My_FlashAttention_optimized as M
    B, H, Hkv, Sq, Sk, D, sc, scale, (wl, wr), L, per_batch = case
    slopes = M.alibi_slopes(H).double() * sc
    if per_batch:
        slopes = slopes[None, :] * torch.linspace(0.5, 1.5, B, dtype=torch.float64)[:, None]
    dist = ar.distance(Sq, Sk, "cpu", L=L)
    Q, K, V, _, vis, gt = vck.reference_agrees_with_autograd(case[:6], scale, (wl, wr), L, dict(slopes=slopes, dist=dist))
    # LSE = logsumexp of the visible biased scores; rows without a visible key: -inf, O = 0
    s = scale * (Q @ K.repeat_interleave(H // Hkv, 1).transpose(-1, -2)) + ar.bias(slopes, dist, B, H)
    lse = torch.logsumexp(s.masked_fill(~vis, -torch.inf), -1)
    assert torch.equal(torch.isneginf(lse), torch.isneginf(gt["LSE"]))
    fin = torch.isfinite(lse)
    assert torch.allclose(lse[fin], gt["LSE"][fin], rtol=0, atol=1e-12)
    assert (gt["O"][~fin] == 0).all() and (gt["dQ"][~fin] == 0).all()
    # the bias matters at these shapes: the unbiased O is far away
    unc = ar.attention_fp64(Q, K, V, None, scale, vis)
    assert (unc["O"] - gt["O"]).norm() / gt["O"].norm() > 0.02
    # the materialised mask of the SDPA baseline is the same bias
    m = ar.alibi_mask(slopes, B, H, Sq, Sk, vis, torch.float64, "cpu", L=L)
    sdpa = torch.nn.functional.scaled_dot_product_attention(Q, K.repeat_interleave(H // Hkv, 1),
                                                            V.repeat_interleave(H // Hkv, 1), attn_mask=m, scale=scale)
    assert torch.allclose(sdpa[fin.unsqueeze(-1).expand_as(sdpa)], gt["O"][fin.unsqueeze(-1).expand_as(sdpa)], atol=1e-10)
