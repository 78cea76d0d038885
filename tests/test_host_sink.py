"""CPU tests of the attention-sink boundary: include/mi355fa_sink.h declares exactly four entry points, libmi355fa.so and
the ctypes tables export them, bad arguments are refused before anything is launched, the Python and C++ surfaces check
the sinks, and the fp64 reference of tests/attn_ref.py agrees with torch.autograd through the eager implementation that
concatenates the sink column.  No compute is launched on a GPU here."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
import attn_ref as sr
import variantcheck as vck

NAMES = ["fa_bwd_dsink", "fa_fwd_kvcache_fp8_sink", "fa_fwd_kvcache_sink", "fa_fwd_sink"]
BASES = (("fa_fwd_sink", "fa_fwd_gqa", "SIGNATURES"), ("fa_fwd_kvcache_sink", "fa_fwd_kvcache", "SIGNATURES"),
         ("fa_fwd_kvcache_fp8_sink", "fa_fwd_kvcache_fp8", "KVCACHE_FP8_SIGNATURES"))


def test_companion_header_declares_the_four_sink_entry_points():
    txt, body, names = vck.header_functions(os.path.join(ROOT, "include", "mi355fa_sink.h"))
    assert names == NAMES
    assert '#include "mi355fa_kvcache_fp8.h"' in txt
    for name in NAMES:
        if name == "fa_bwd_dsink":
            continue
        sig = body[body.index(name + "("):]   # the sinks follow the scale
        assert re.search(r"float scale,\s*const float\* sinks,\s*int window_left", sig[:sig.index(";")]), name
    sig = body[body.index("fa_bwd_dsink("):]
    assert re.sub(r"\s+", " ", sig[:sig.index(";")]) == (
        "fa_bwd_dsink(const float* lse, const float* delta, const float* sinks, float* dsinks, int B, int H, int S_q, "
        "const mi355fa_opts* opts, void* stream)")
    # the comment states the formulas, the units, the backward order and the edge cases
    for needle in ("exp(z_h) + sum_j exp(s_ij)", "NOT multiplied by `scale`", "the sink INCLUDED", "fa_bwd_dq_gqa",
                   "fa_bwd_dkv_gqa", "LSE = z_h", "z_h = -inf", "OVERWRITTEN"):
        assert needle in txt, needle
    base = open(os.path.join(ROOT, "include", "mi355fa.h")).read()
    assert "sink" not in base.lower() and re.search(r"#define\s+MI355FA_ABI_VERSION\s+7\b", base)


def test_library_and_ctypes_tables_export_them():
    import _mi355fa as fa
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in fa.SINK_SIGNATURES and name in fa.ALL_SIGNATURES, name
        assert name not in fa.SIGNATURES and name not in fa.SOFTCAP_SIGNATURES and name not in fa.ALIBI_SIGNATURES, name
    assert fa.lib.fa_abi_version() == 7
    # the base signature with (const float*) spliced in after the scale
    vck.check_spliced_signatures(fa.SINK_SIGNATURES, [(n, getattr(fa, t)[b]) for n, b, t in BASES], [ctypes.c_void_p])
    assert fa.SINK_SIGNATURES["fa_bwd_dsink"][1] == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + \
        [fa.SIGNATURES["fa_fwd_gqa"][1][-2], ctypes.c_void_p]


def _calls(p):
    """name -> f(scale, (sinks,), H, H_kv, wl, opts) per forward entry point, B = 2"""
    import _mi355fa as fa
    return vck.entry_calls(fa.lib, [n for n in NAMES if n != "fa_bwd_dsink"], p, B=2)


def test_null_and_misaligned_sinks_are_refused():
    import _mi355fa as fa
    _buf, p = vck.aligned_ptr()
    for name, f in _calls(p).items():
        assert f(0.125, (None,), 4, 2, -1, None) == -1, name          # MI355FA_ERR_NULL
        assert name.encode() in fa.lib.fa_last_error() and b"sinks" in fa.lib.fa_last_error()
        for off in (1, 2, 3):
            assert f(0.125, (p + off,), 4, 2, -1, None) == -5, name   # MI355FA_ERR_ALIGN
            assert b"sinks" in fa.lib.fa_last_error()
        # a 4-byte (not 16-byte) aligned pointer passes these checks; the call then stops at the first later check
        assert f(0.0, (p + 4,), 4, 2, -1, None) == -2, name
        assert b"scale" in fa.lib.fa_last_error()
    L = fa.lib
    assert L.fa_bwd_dsink(p, p, None, p, 2, 4, 8, None, None) == -1 and b"sinks" in L.fa_last_error()
    assert L.fa_bwd_dsink(None, p, p, p, 2, 4, 8, None, None) == -1
    assert L.fa_bwd_dsink(p, None, p, p, 2, 4, 8, None, None) == -1
    assert L.fa_bwd_dsink(p, p, p, None, 2, 4, 8, None, None) == -1
    for off in (1, 2, 3):
        assert L.fa_bwd_dsink(p, p, p + off, p, 2, 4, 8, None, None) == -5 and b"sinks" in L.fa_last_error()
        assert L.fa_bwd_dsink(p, p, p, p + off, 2, 4, 8, None, None) == -5 and b"dsinks" in L.fa_last_error()
    assert L.fa_bwd_dsink(p + 4, p, p, p, 2, 4, 8, None, None) == -5 and b"lse" in L.fa_last_error()
    for shape in ((0, 4, 8), (2, 0, 8), (2, 4, 0)):
        assert L.fa_bwd_dsink(p, p, p + 4, p + 4, *shape, None, None) == -2, shape    # MI355FA_ERR_SHAPE
    bad = fa.Opts.make()
    bad.size = 8
    assert L.fa_bwd_dsink(p, p, p, p, 2, 4, 8, ctypes.byref(bad), None) == -2


def test_other_bad_arguments_keep_their_own_codes():
    import _mi355fa as fa
    _buf, p = vck.aligned_ptr()
    calls = _calls(p)
    for name, texts in vck.check_common_refusals(calls, (p,)).items():
        assert calls[name](0.125, (p,), 0, 1, -1, None) == -2, name   # H < 1: MI355FA_ERR_SHAPE
        if name == "fa_fwd_sink":
            assert b"sinks" in texts["dropout"], name
    L = fa.lib
    assert L.fa_fwd_sink(p, p, p, p, p, 2, 4, 2, 8, 8, 96, fa.BF16, 0.125, p, -1, 0, None, None) == -3   # MI355FA_ERR_HEAD_DIM
    assert L.fa_fwd_kvcache_fp8_sink(p, p, p, None, None, p, None, None, 0, p, p, p, 1 << 12, 2, 4, 2, 1, 8, 0, 64, fa.BF16, 1,
                                     0.125, p, -1, 0, None, None) == -4   # kv_dtype: MI355FA_ERR_DTYPE


def test_python_surface():
    import My_FlashAttention_optimized as M
    import _mi355fa_torch as ext
    assert str(inspect.signature(M.flash_attention_sink)) == (
        "(Q, K, V, sinks, is_causal=False, window_size=(-1, -1), softmax_scale=None, cu_seqlens_q=None, "
        "cu_seqlens_k=None, max_seqlen_q=0, max_seqlen_k=0)")
    assert str(inspect.signature(M.flash_attention_kvcache_sink)) == (
        "(q, k_cache, v_cache, cache_seqlens, sinks, k_new=None, v_new=None, is_causal=False, window_size=(-1, -1), "
        "softmax_scale=None, return_lse=False)")
    assert str(inspect.signature(M.flash_attention_kvcache_fp8_sink)).startswith(
        "(q, k_cache, v_cache, cache_seqlens, sinks, k_descale=None, v_descale=None, k_new=None, v_new=None, ")
    for name in ("FlashAttentionSinkFunction", "flash_attention_sink_forward", "flash_attention_sink_backward"):
        assert hasattr(M, name), name
    for name in ("flash_attention_sink", "sink_forward_launch", "sink_backward_launch", "kvcache_sink_forward",
                 "kvcache_fp8_sink_forward"):
        assert hasattr(ext, name), name
    # no existing function changed its signature
    assert str(inspect.signature(M.flash_attention)) == "(Q, K, V, is_causal=False)"
    assert str(inspect.signature(M.flash_attention_gqa)) == (
        "(Q, K, V, is_causal=False, window_size=(-1, -1), cu_seqlens_q=None, cu_seqlens_k=None, max_seqlen_q=None, "
        "max_seqlen_k=None)")


def _bad_sinks(H):
    """(sinks, message) pairs every checker refuses, for H query heads"""
    ok = torch.ones(H)
    return [
        (ok.double(), "float32"),
        (ok.half(), "float32"),
        (torch.ones(H + 1), "shape"),
        (torch.ones(2, H), "shape"),
        (torch.ones(H, 1), "shape"),
        (torch.ones(2 * H)[::2], "contiguous"),
    ]


def test_python_refuses_bad_sinks():
    """Python checks the sinks before anything else touches a device (CPU tensors here: the device check comes last)."""
    import My_FlashAttention_optimized as M
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    Q, K = mk(2, 4, 16, 64), mk(2, 2, 16, 64)
    K8 = torch.zeros(2, 2, 16, 64).to(torch.float8_e4m3fn)
    sl = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(AssertionError, match="device"):
        M.flash_attention_sink(Q, K, K, torch.ones(4, device="meta"))
    with pytest.raises(AssertionError, match="device"):
        M.flash_attention_kvcache_sink(Q, K, K, sl, torch.ones(4, device="meta"))
    with pytest.raises(AssertionError, match="device"):
        M.flash_attention_kvcache_fp8_sink(Q, K8, K8, sl, torch.ones(4, device="meta"))
    with pytest.raises(AssertionError, match="tensor"):
        M.flash_attention_sink(Q, K, K, [0.0] * 4)
    for s, msg in _bad_sinks(4):
        with pytest.raises(AssertionError, match=msg):
            M.flash_attention_sink(Q, K, K, s)
        with pytest.raises(AssertionError, match=msg):
            M.FlashAttentionSinkFunction.apply(Q, K, K, s, -1, -1)
        with pytest.raises(AssertionError, match=msg):
            M.flash_attention_kvcache_sink(Q, K, K, sl, s)
        with pytest.raises(AssertionError, match=msg):
            M.flash_attention_kvcache_fp8_sink(Q, K8, K8, sl, s)
    with pytest.raises(AssertionError, match="softmax_scale"):
        M.flash_attention_sink(Q, K, K, torch.ones(4), softmax_scale=-1.0)
    with pytest.raises(AssertionError, match="window_right"):
        M.flash_attention_sink(Q, K, K, torch.ones(4), is_causal=True, window_size=(-1, 3))
    # varlen: the heads are dim 1 of the packed Q
    cu = torch.tensor([0, 5, 9, 16], dtype=torch.int32)
    Qp, Kp = mk(16, 4, 64), mk(16, 2, 64)
    with pytest.raises(AssertionError, match="shape"):
        M.flash_attention_sink(Qp, Kp, Kp, torch.ones(16), cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=7, max_seqlen_k=7)


def test_decode_functions_refuse_requires_grad():
    """The two decoding functions are inference only: sinks (and q) that require grad are refused, in Python and in C++;
    the training call accepts sinks that require grad (it stops at the device check here)."""
    import My_FlashAttention_optimized as M
    import _mi355fa_torch as ext
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    Q, K = mk(2, 4, 16, 64), mk(2, 2, 16, 64)
    K8 = torch.zeros(2, 2, 16, 64).to(torch.float8_e4m3fn)
    sl = torch.zeros(2, dtype=torch.int32)
    zg = torch.ones(4, requires_grad=True)
    with pytest.raises(AssertionError, match="grad"):
        M.flash_attention_kvcache_sink(Q, K, K, sl, zg)
    with pytest.raises(AssertionError, match="grad"):
        M.flash_attention_kvcache_fp8_sink(Q, K8, K8, sl, zg)
    with pytest.raises(AssertionError, match="device"):   # not "grad": the training call may differentiate the sinks
        M.flash_attention_sink(Q, K, K, zg)
    with pytest.raises(AssertionError, match="sinks must be a device tensor"):
        ext.flash_attention_sink(Q, K, K, zg, -1, 0)


def test_cpp_binding_checks():
    """The C++ functions' own checks (no device needed): the sinks are checked before Q's device, so CPU tensors reach
    each of them; well-formed CPU sinks stop at the sinks' device check."""
    import _mi355fa_torch as ext
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    Q, K = mk(2, 4, 16, 64), mk(2, 2, 16, 64)
    K8 = torch.zeros(2, 2, 16, 64).to(torch.float8_e4m3fn)
    sl = torch.zeros(2, dtype=torch.int32)
    calls = (lambda s: ext.flash_attention_sink(Q, K, K, s, -1, 0),
             lambda s: ext.sink_forward_launch(Q, K, K, s, -1, 0, 0.1),
             lambda s: ext.sink_backward_launch(Q, K, K, Q, Q, torch.zeros(2, 4, 16), s),
             lambda s: ext.kvcache_sink_forward(Q, K, K, sl, s),
             lambda s: ext.kvcache_fp8_sink_forward(Q, K8, K8, sl, s))
    for f in calls:
        for s, msg in _bad_sinks(4) + [(torch.ones(4), "sinks must be a device tensor")]:
            with pytest.raises(AssertionError, match=msg):
                f(s)
    with pytest.raises(AssertionError, match="softmax_scale"):
        ext.flash_attention_sink(Q, K, K, torch.ones(4), -1, 0, -0.5)
    with pytest.raises(AssertionError, match="multiple"):
        ext.flash_attention_sink(Q, mk(2, 3, 16, 64), mk(2, 3, 16, 64), torch.ones(4), -1, 0)


CASES = [  # B, H, H_kv, S_q, S_k, D, scale, (wl, wr), bottom-right L (None: training), sinks
    (2, 4, 2, 9, 13, 8, 0.5, (-1, -1), None, (0.0, 3.0)),
    (1, 4, 1, 12, 12, 8, 0.35, (-1, 0), None, (-2.0, 2.0)),
    (2, 2, 2, 11, 17, 16, 0.25, (3, 0), None, (0.0, 8.0)),
    (1, 6, 3, 17, 10, 8, 0.5, (2, 2), None, (0.5, 4.0)),     # S_q > S_k under a window: rows 13.. see no key
    (2, 4, 2, 3, 20, 8, 0.5, (6, 0), 14, (1.0, 5.0)),
    (2, 4, 4, 8, 8, 8, 0.5, (-1, 0), None, (2.0, 2.0)),
    (2, 6, 2, 9, 13, 8, 0.5, (-1, 0), None, (0.0, 3.0)),   # g = 3
    (2, 7, 1, 5, 20, 8, 0.5, (6, 2), 14, (0.5, 4.0)),      # g = 7, multi-query, decoding with keys right of the queries
]


@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_fp64_reference_agrees_with_autograd(case):
    """tests/attn_ref.py's closed-form gradients, dz included, against autograd through the eager implementation that
    concatenates the sink column (fp64, CPU)."""
    B, H, Hkv, Sq, Sk, D, scale, (wl, wr), L, (z0, z1) = case
    sinks = torch.linspace(z0, z1, H, dtype=torch.float64)
    Q, K, V, _, vis, gt = vck.reference_agrees_with_autograd(case[:6], scale, (wl, wr), L, dict(sinks=sinks))
    assert (gt["den"] >= gt["dz"].abs() - 1e-12).all()
    # LSE = logsumexp over the visible scores and the sink; rows without a visible key: LSE = z, O = 0, dQ = 0
    s = scale * (Q @ K.repeat_interleave(H // Hkv, 1).transpose(-1, -2))
    zc = sinks.view(1, H, 1, 1).expand(B, H, Sq, 1)
    lse = torch.logsumexp(torch.cat([s.masked_fill(~vis, -torch.inf), zc], -1), -1)
    assert torch.allclose(lse, gt["LSE"], rtol=0, atol=1e-12)
    keyless = ~vis.expand(B, H, Sq, Sk).any(-1)
    if case[3] > case[4]:
        assert keyless.any()
    assert torch.equal(gt["LSE"][keyless], zc[..., 0][keyless])
    assert (gt["O"][keyless] == 0).all() and (gt["dQ"][keyless] == 0).all() and (gt["P0"][keyless] == 1).all()
    assert torch.allclose(gt["P0"], torch.exp(zc[..., 0] - lse), rtol=0, atol=1e-12)
    # the sink matters at these shapes: the sink-less O is far away
    unc = sr.attention_fp64(Q, K, V, None, scale, vis)
    assert (unc["O"] - gt["O"]).norm() / gt["O"].norm() > 0.02


@pytest.mark.parametrize("case", CASES[:4], ids=[str(i) for i in range(4)])
def test_minus_inf_sinks_reduce_to_plain_attention(case):
    """z = -inf: the reference is the sink-less attention (the call without sinks) exactly (keyless rows: O = 0,
    LSE = -inf), and dz = 0."""
    B, H, Hkv, Sq, Sk, D, scale, (wl, wr), L, _ = case
    g = torch.Generator().manual_seed(7 + sum(case[:6]))
    Q = torch.randn(B, H, Sq, D, generator=g, dtype=torch.float64)
    K, V = (torch.randn(B, Hkv, Sk, D, generator=g, dtype=torch.float64) for _ in range(2))
    dO = torch.randn(B, H, Sq, D, generator=g, dtype=torch.float64)
    vis = sr.visible(Sq, Sk, wl, wr, "cpu", L=L)
    gt = sr.attention_fp64(Q, K, V, dO, scale, vis, sinks=torch.full((H,), -torch.inf))
    plain = sr.attention_fp64(Q, K, V, dO, scale, vis)
    for n in ("O", "LSE", "dQ", "dK", "dV"):
        assert torch.equal(gt[n], plain[n]), n
    assert (gt["dz"] == 0).all() and (gt["den"] == 0).all() and (gt["P0"] == 0).all()
    none = sr.attention_fp64(Q, K, V, dO, scale, vis, sinks=None)
    for n in ("O", "LSE", "dQ", "dK", "dV", "dz"):
        assert torch.equal(gt[n], none[n]), n
