"""CPU tests of the packed MXFP4 decoding boundary (include/mi355fa_ragged_fp4.h; fp4_ragged_kvcache.py): the header declares
exactly two entry points and includes both parents; libmi355fa.so and a ctypes table of their own (RAGGED_FP4_SIGNATURES)
export them; the ABI version and the older headers are untouched ("fp4" still absent from those that did not have it); the
workspace is mi355fa_ragged.h's formula with this path's own split count, D = 256 included; every refusal is reported before
anything is launched, with the parents' codes; the D = 256 instances of the packed MXFP4 kernel stay inside the decode
kernels' register and LDS budget; the Python function's surface and refusals.  No compute is launched here (no GPU)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
import raggedcheck as rc
import variantcheck as vck

HDR = os.path.join(ROOT, "include", "mi355fa_ragged_fp4.h")
NAMES = ["fa_fwd_kvcache_fp4_ragged", "fa_fwd_kvcache_fp4_ragged_workspace_bytes"]
NULL, SHAPE, DTYPE, ALIGN, STRIDE = -1, -2, -4, -5, -6


def _lib():
    import _mi355fa as fa
    return fa


def test_header_library_and_ctypes_agree():
    fa = _lib()
    txt, body, functions = vck.header_functions(HDR)
    assert functions == NAMES
    assert '#include "mi355fa_ragged.h"' in txt and '#include "mi355fa_kvcache_fp4.h"' in txt
    assert "#define" not in body.replace("#define MI355FA_RAGGED_FP4_H_", "") and "typedef" not in body and "fa_debug" not in txt
    for phrase in ("D = 256", "pool of B pages", "soft-cap", "ALiBi", "MI355FA_ERR_RAGGED", "never 0"):
        assert phrase in txt, phrase
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in fa.RAGGED_FP4_SIGNATURES and name in fa.ALL_SIGNATURES, name
        assert name not in fa.RAGGED_SIGNATURES and name not in fa.KVCACHE_FP4_SIGNATURES, name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, body)
        assert len(fa.RAGGED_FP4_SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    assert len(fa.RAGGED_FP4_SIGNATURES["fa_fwd_kvcache_fp4_ragged"][1]) == 33
    assert fa.lib.fa_abi_version() == 7 and fa.ABI_VERSION == 7
    assert re.search(r"#define\s+MI355FA_ABI_VERSION\s+7\b", open(os.path.join(ROOT, "include", "mi355fa.h")).read())
    # the parents' function lists are as they were, and the headers that never spoke of fp4 still do not
    assert vck.header_functions(os.path.join(ROOT, "include", "mi355fa_ragged.h"))[2] == [
        "fa_fwd_kvcache_ragged", "fa_fwd_kvcache_ragged_workspace_bytes"]
    assert len(vck.header_functions(os.path.join(ROOT, "include", "mi355fa_kvcache_fp4.h"))[2]) == 4
    for older in ("mi355fa.h", "mi355fa_kvcache.h", "mi355fa_kvcache_fp8.h", "mi355fa_paged.h", "mi355fa_ragged.h", "mi355fa_sink.h",
                  "mi355fa_softcap.h", "mi355fa_alibi.h", "mi355fa_gqa.h", "mi355fa_local.h"):
        assert "fp4" not in open(os.path.join(ROOT, "include", older)).read().lower(), older


def _rule(wgs, S_cache, D):
    """this path's split rule (the comment above kvcache_splits): 512 workgroups, splits of sqrt(64 S) keys, sqrt(16 S) at D = 256"""
    n = -(-512 // wgs)
    by_len, keys = 1, 16 if D == 256 else 64
    while (by_len + 1) ** 2 * keys <= S_cache:
        by_len += 1
    return max(1, min(n, by_len, 64))


def test_workspace_is_the_ragged_formula_with_this_paths_split_count():
    fa = _lib()
    W = fa.lib.fa_fwd_kvcache_fp4_ragged_workspace_bytes
    shapes = ((8, 8, 32, 8, 128, 128, 128), (145, 32, 32, 8, 128, 128, 128), (1, 1, 4, 4, 1, 32, 64), (17, 300, 8, 1, 3, 32, 64),
              (33, 5, 16, 16, 7, 96, 128), (8, 8, 16, 8, 128, 128, 256), (1, 1, 8, 1, 32, 128, 256), (14, 6, 5, 1, 4, 96, 256))
    try:
        for n in (1, 2, 7):
            vck.splits(n)
            for (T, B, H, Hkv, MP, page, D) in shapes:
                got = W(T, B, H, Hkv, MP, page, D)
                assert got == rc.workspace_bytes(n, T, B, H, Hkv, D) and got >= 32, (n, T, B, H, Hkv, MP, page, D, got)
                plan = (16 + 8 * rc.nb_max(H // Hkv, T, B) + 15) // 16 * 16
                assert got == plan + (n * H * T * (D + 2) * 4 if n > 1 else 0)
                if D != 256:                                                    # the 16-bit call's bytes at the same forced n
                    assert got == fa.lib.fa_fwd_kvcache_ragged_workspace_bytes(T, B, H, Hkv, MP, page, D, fa.PAGED_CACHE_16BIT)
        vck.splits(0)
        for (T, B, H, Hkv, MP, page, D) in shapes:
            n = _rule(Hkv * rc.nb_max(H // Hkv, T, B), MP * page, D)
            assert W(T, B, H, Hkv, MP, page, D) == rc.workspace_bytes(n, T, B, H, Hkv, D), (T, B, H, Hkv, MP, page, D, n)
    finally:
        vck.splits(0)
    assert W(8, 8, 16, 8, 128, 128, 256) > 0                                    # D = 256 is accepted here ...
    assert fa.lib.fa_fwd_kvcache_fp4_paged_workspace_bytes(8, 16, 8, 1, 128, 128, 0, 256) == SHAPE   # ... and only here
    for D in (96, 32, 512):
        assert W(8, 8, 16, 8, 128, 128, D) == SHAPE, D
    for page in (16, 0, 48):
        assert W(8, 8, 16, 8, 128, page, 128) == fa.ERR_PAGED, page
    assert W(0, 8, 16, 8, 128, 128, 128) == fa.ERR_RAGGED and W(8, 0, 16, 8, 128, 128, 128) == fa.ERR_RAGGED
    assert W(8, 8, 16, 3, 128, 128, 128) == fa.ERR_GROUP


def _call(fa, p, **over):
    """One otherwise well-formed packed MXFP4 call (11 rows over B 3, H 8, H_kv 2, 6 pages of 64 keys per sequence, D 128, bf16,
    every pointer p) with the arguments of `over` replaced."""
    a = dict(q=p, kp=p, vp=p, ks=p, vs=p, kn=None, vn=None, cu=p, sl=p, bt=p, kss=None, vss=None, sinks=None, o=p, ws=p,
             wsb=1 << 20, T=11, B=3, H=8, Hkv=2, NP=100, page=64, MP=6, bts=6, D=128, dt=fa.BF16, kvdt=fa.KV_MXFP4, scale=0.125,
             wl=-1, wr=-1, opts=None)
    a.update(over)
    return fa.lib.fa_fwd_kvcache_fp4_ragged(a["q"], a["kp"], a["vp"], a["ks"], a["vs"], a["kn"], a["vn"], a["cu"], a["sl"], a["bt"],
                                            a["kss"], a["vss"], a["sinks"], a["o"], None, a["ws"], a["wsb"], a["T"], a["B"], a["H"],
                                            a["Hkv"], a["NP"], a["page"], a["MP"], a["bts"], a["D"], a["dt"], a["kvdt"], a["scale"],
                                            a["wl"], a["wr"], a["opts"], None)


def test_refusals_come_before_launch():
    fa = _lib()
    L = fa.lib
    _buf, p = vck.aligned_ptr()
    S3 = lambda *s: ctypes.cast((ctypes.c_longlong * 3)(*s), ctypes.POINTER(ctypes.c_longlong))
    err = lambda: L.fa_last_error().decode()
    fn = "fa_fwd_kvcache_fp4_ragged"
    for n in (1, 4):
        vck.splits(n)
        try:
            for kvdt in (0, 2, -1):
                assert _call(fa, p, kvdt=kvdt) == DTYPE and err() == "%s: kv_dtype must be MI355FA_KV_MXFP4" % fn
            for D in (96, 32, 512):
                assert _call(fa, p, D=D) == SHAPE, D
                assert err() == "%s: packed queries over an MXFP4 cache take head dim 64, 128 or 256 (got %d)" % (fn, D)
            for page in (16, 0, 48):
                assert _call(fa, p, page=page) == fa.ERR_PAGED, page
                assert err() == "%s: page_size must be a positive multiple of 32" % fn
            for kw in ({"NP": 0}, {"MP": 0}, {"bts": 5}):
                assert _call(fa, p, **kw) == fa.ERR_PAGED, kw
            # misaligned pools and scales: 16 bytes, and the scale row of D / 32 bytes (8 at D = 256: the kernel's 4-byte half loads)
            assert _call(fa, p, kp=p + 8) == ALIGN and "16-byte aligned" in err()
            assert _call(fa, p, vp=p + 8) == ALIGN
            for D, off in ((256, 4), (256, 2), (128, 2), (128, 1), (64, 1)):
                assert _call(fa, p, ks=p + off, D=D) == ALIGN, (D, off)
                assert err() == "%s: k_scale / v_scale must be aligned to their row of D / 32 bytes" % fn
                assert _call(fa, p, vs=p + off, D=D) == ALIGN, (D, off)
            # short or odd scale strides
            keep = S3(2 * 64 * 4, 64 * 4, 0)
            assert _call(fa, p, kss=keep) == STRIDE and err() == "%s: the scale row stride must be at least D / 32 bytes" % fn
            keep = S3(2 * 64 * 4, 64 * 4, 6)
            assert _call(fa, p, kss=keep) == STRIDE and "multiples of D / 32" in err()
            keep = S3(2 * 64 * 8, 64 * 8, 12)
            assert _call(fa, p, vss=keep, D=256) == STRIDE and "multiples of D / 32" in err()
            keep = S3(2 * 64 * 4 + 2, 64 * 4, 4)
            assert _call(fa, p, vss=keep) == STRIDE
            keep = S3(2 * 64 * 64, 64 * 64, 72)                                  # a pool row stride off 16 bytes
            assert _call(fa, p, opts=ctypes.byref(fa.Opts.make(k_strides=keep, v_strides=keep))) == STRIDE and "MXFP4 cache" in err()
            # the packed geometry: MI355FA_ERR_RAGGED
            for T in (0, -1):
                assert _call(fa, p, T=T) == fa.ERR_RAGGED and "total_q" in err(), T
            for B in (0, -3):
                assert _call(fa, p, B=B) == fa.ERR_RAGGED and "B must be" in err(), B
            assert _call(fa, p, T=(1 << 24) // 8 + 1) == fa.ERR_RAGGED
            for which in ("q_strides", "o_strides"):
                for st in ((0, 128, 8 * 128 + 4), (0, 128 + 2, 8 * 128), (0, 128, 120), (0, -128, 8 * 128)):
                    keep = S3(*st)
                    assert _call(fa, p, opts=ctypes.byref(fa.Opts.make(**{which: keep}))) == fa.ERR_RAGGED, (which, st)
                    assert "strides of packed q / o" in err()
            # NULL table / cu / scales, and the alignment of the integer vectors
            assert _call(fa, p, bt=None) == NULL and "block_table" in err()
            assert _call(fa, p, cu=None) == NULL and "cu_seqlens_q" in err()
            assert _call(fa, p, ks=None) == NULL and _call(fa, p, vs=None) == NULL
            assert _call(fa, p, cu=p + 2) == ALIGN and _call(fa, p, bt=p + 2) == ALIGN and _call(fa, p, sinks=p + 2) == ALIGN
            assert _call(fa, p, kn=p) == NULL and "k_new and v_new" in err()
            assert _call(fa, p, Hkv=3) == fa.ERR_GROUP and _call(fa, p, wl=-2) == fa.ERR_WINDOW and _call(fa, p, dt=2) == DTYPE
            # the workspace: never 0, refused one byte short and when absent; D = 256 passes every check up to it
            for D in (128, 256):
                need = L.fa_fwd_kvcache_fp4_ragged_workspace_bytes(11, 3, 8, 2, 6, 64, D)
                assert need == rc.workspace_bytes(n, 11, 3, 8, 2, D)
                assert _call(fa, p, D=D, wsb=need - 1) == fa.ERR_WORKSPACE and _call(fa, p, D=D, ws=None) == fa.ERR_WORKSPACE
        finally:
            vck.splits(0)


def test_d256_instances_stay_inside_the_decode_budget():
    """The four D = 256 instances of the packed MXFP4 kernel (fa_decode_ragged_kernel<T, 256, SINK>), held to what
    tests/test_host_decode_d256.py holds the 16-bit and e4m3 ones to; the D = 64 / 128 ones and the append have no scratch."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj
    found = {64: 0, 128: 0, 256: 0}
    appends = 0
    for k in codeobj.kernels():
        m = re.match(r"_ZN2fa23fa_decode_ragged_kernelINS_\d+(BF16|FP16)ELi(\d+)ELb[01]EEE", k["name"])
        if m:
            found[int(m.group(2))] += 1
            assert k["wg"] == 256 and k["vgpr"] + k["agpr"] <= 256, (k["name"], k["vgpr"], k["agpr"])
            assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 81920, k["name"]
        elif re.match(r"_ZN2fa31fa_kvcache_append_ragged_kernelINS_\d+(BF16|FP16)EEE", k["name"]):
            appends += 1
            assert k["scratch"] == 0 and k["spill"] == 0, k["name"]
    assert found == {64: 4, 128: 4, 256: 4} and appends == 2, (found, appends)


def _args(D=64, page=64, dtype=torch.bfloat16):
    B, H, Hkv, NP, MP, T = 2, 4, 2, 8, 3, 5
    kc, ks = torch.zeros(NP, Hkv, page, D // 2, dtype=torch.uint8), torch.zeros(NP, Hkv, page, D // 32, dtype=torch.uint8)
    return dict(q=torch.zeros(T, H, D, dtype=dtype), k_cache=kc, v_cache=kc.clone(), k_scale=ks, v_scale=ks.clone(),
                cu_seqlens_q=torch.tensor([0, 2, 5], dtype=torch.int32), cache_seqlens=torch.zeros(B, dtype=torch.int32),
                block_table=torch.zeros(B, MP, dtype=torch.int32))


def test_python_surface_and_refusals():
    import fp4_ragged_kvcache as R
    import fp4_kvcache as F
    import ragged_kvcache as G
    import _mi355fa_fp4_torch as ext
    assert R.__all__ == ["flash_attention_kvcache_fp4_ragged"]
    assert F.__all__ == ["quantize_kv_mxfp4", "dequantize_kv_mxfp4", "flash_attention_kvcache_fp4", "flash_attention_kvcache_fp4_paged"]
    assert G.__all__ == ["flash_attention_kvcache_ragged"]
    assert str(inspect.signature(R.flash_attention_kvcache_fp4_ragged)) == (
        "(q, k_cache, v_cache, k_scale, v_scale, cu_seqlens_q, cache_seqlens, block_table, k_new=None, v_new=None, "
        "is_causal=False, window_size=(-1, -1), softmax_scale=None, return_lse=False, sinks=None, out=None)")
    assert hasattr(ext, "kvcache_fp4_ragged_forward") and hasattr(ext, "kvcache_fp4_forward")
    f = R.flash_attention_kvcache_fp4_ragged

    def refused(what, **over):
        kw = _args(**{k: over.pop(k) for k in ("page", "D") if k in over})
        kw.update(over)
        with pytest.raises(AssertionError, match=what):
            f(**kw)

    a = _args()
    refused("cu_seqlens_q must be a device tensor")               # everything else in order: the host tensor is what is left
    refused("cu_seqlens_q must be a device tensor", D=256)        # D = 256 passes the wrapper's checks
    refused("cu_seqlens_q must be int32", cu_seqlens_q=a["cu_seqlens_q"].to(torch.int64))
    refused("cu_seqlens_q must be a vector of B \\+ 1 entries", cu_seqlens_q=a["cu_seqlens_q"][:1])
    refused("block_table must be int32", block_table=a["block_table"].to(torch.int64))
    refused("block_table must be \\[B, max_pages_per_seq\\] with B = 2", block_table=torch.zeros(3, 3, dtype=torch.int32))
    refused("cache_seqlens must have B = 2 entries", cache_seqlens=torch.zeros(3, dtype=torch.int32))
    refused("q must be \\[total_q, H, D\\]", q=a["q"][None])
    refused("D = 64, 128 or 256", q=torch.zeros(5, 4, 96, dtype=torch.bfloat16))
    refused("multiple of 32", page=48)
    refused("float4_e2m1fn_x2", k_cache=a["k_cache"].to(torch.float16), v_cache=a["v_cache"].to(torch.float16))
    refused("float8_e8m0fnu", k_scale=a["k_scale"].to(torch.int8), v_scale=a["v_scale"].to(torch.int8))
    refused("out must have q's shape", out=torch.zeros(6, 4, 64, dtype=torch.bfloat16))
    refused("out must have q's dtype", out=torch.zeros(5, 4, 64, dtype=torch.float16))
    refused("softmax_scale must be finite and > 0", softmax_scale=-1.0)
    refused("is_causal=True with window_right > 0", is_causal=True, window_size=(-1, 3))
    refused("k_new and v_new must be given together", k_new=torch.zeros(5, 2, 64, dtype=torch.bfloat16))
    refused("has no backward: q must not require grad", q=a["q"].clone().requires_grad_(True))
    refused("has no backward: sinks must not require grad", sinks=torch.ones(4, requires_grad=True))
    refused("has no backward: out must not require grad", out=a["q"].clone().requires_grad_(True))
    with pytest.raises(TypeError):
        f(**a, softcap=30.0)                                                    # no soft-cap or ALiBi argument
    # the binding's own checks are reached with host tensors too
    with pytest.raises(AssertionError, match="device tensors"):
        ext.kvcache_fp4_ragged_forward(a["q"], a["k_cache"], a["v_cache"], a["k_scale"], a["v_scale"], a["cu_seqlens_q"],
                                       a["cache_seqlens"], a["block_table"], None, None, -1, -1, 0.0, None, None)
    with pytest.raises(AssertionError, match="head dim 64, 128 or 256"):
        ext.kvcache_fp4_ragged_forward(torch.zeros(5, 4, 96, dtype=torch.bfloat16), a["k_cache"], a["v_cache"], a["k_scale"],
                                       a["v_scale"], a["cu_seqlens_q"], a["cache_seqlens"], a["block_table"], None, None, -1, -1,
                                       0.0, None, None)
    # the rectangular calls keep refusing D = 256
    with pytest.raises(AssertionError, match="D = 64 or 128"):
        u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
        F.flash_attention_kvcache_fp4(torch.zeros(2, 8, 1, 256, dtype=torch.float16), u8(2, 2, 128, 128), u8(2, 2, 128, 128),
                                      u8(2, 2, 128, 8), u8(2, 2, 128, 8), torch.zeros(2, dtype=torch.int32))
