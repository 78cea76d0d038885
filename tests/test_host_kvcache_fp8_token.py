"""CPU tests of the per-token-scaled e4m3 decoding boundary (include/mi355fa_kvcache_fp8_token.h; fp8_token_kvcache.py): the
header declares exactly six entry points and the library exports them with ctypes signatures of their own; the ABI version and
every other header's function list are untouched; the workspace functions follow the shared formulas with the e4m3 path's split
rule; every bad argument is refused before anything is launched, with the parents' codes and a message naming the function; the
Python surface and refusals; quantize_kv_fp8_per_token against a numpy reference written here, element for element; the new
kernels are in the library at the expected counts and inside the decode kernels' budget.  No compute is launched (no GPU)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import raggedcheck as rc
import variantcheck as vck

HDR = os.path.join(ROOT, "include", "mi355fa_kvcache_fp8_token.h")
NAMES = sorted(["fa_fwd_kvcache_fp8_token", "fa_fwd_kvcache_fp8_token_workspace_bytes", "fa_fwd_kvcache_fp8_token_paged",
                "fa_fwd_kvcache_fp8_token_paged_workspace_bytes", "fa_fwd_kvcache_fp8_token_ragged",
                "fa_fwd_kvcache_fp8_token_ragged_workspace_bytes"])
NULL, SHAPE, HEAD_DIM, DTYPE, ALIGN, STRIDE = -1, -2, -3, -4, -5, -6
F8 = torch.float8_e4m3fn


def _lib():
    import _mi355fa as fa
    return fa


def _T():
    import fp8_token_kvcache as T
    return T


# ---------------------------------------------------------------- the C boundary
def test_header_library_and_ctypes_agree():
    fa = _lib()
    txt, body, functions = vck.header_functions(HDR)
    assert functions == NAMES
    for parent in ("mi355fa_kvcache_fp8.h", "mi355fa_paged.h", "mi355fa_ragged.h"):
        assert '#include "%s"' % parent in txt, parent
    assert "#define" not in body.replace("#define MI355FA_KVCACHE_FP8_TOKEN_H_", "") and "typedef" not in body and "fa_debug" not in txt
    assert "kv_dtype" not in body
    for phrase in ("amax / 448.0f", "s = 1.0f", "nearest even", "-0.0 kept", "ELEMENT strides", "pool of B pages", "Exactness",
                   "exponent field", "MI355FA_ERR_SHAPE", "MI355FA_ERR_HEAD_DIM", "never 0"):
        assert phrase in txt, phrase
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in fa.KVCACHE_FP8_TOKEN_SIGNATURES and name in fa.ALL_SIGNATURES, name
        assert name not in fa.KVCACHE_FP8_SIGNATURES and name not in fa.KVCACHE_FP4_SIGNATURES and name not in fa.RAGGED_FP4_SIGNATURES
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, body)
        assert len(fa.KVCACHE_FP8_TOKEN_SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    assert len(fa.KVCACHE_FP8_TOKEN_SIGNATURES) == 6
    # the MXFP4 signatures without kv_dtype
    for tok, fp4, table in (("fa_fwd_kvcache_fp8_token", "fa_fwd_kvcache_fp4", fa.KVCACHE_FP4_SIGNATURES),
                            ("fa_fwd_kvcache_fp8_token_paged", "fa_fwd_kvcache_fp4_paged", fa.KVCACHE_FP4_SIGNATURES),
                            ("fa_fwd_kvcache_fp8_token_ragged", "fa_fwd_kvcache_fp4_ragged", fa.RAGGED_FP4_SIGNATURES)):
        assert len(fa.KVCACHE_FP8_TOKEN_SIGNATURES[tok][1]) == len(table[fp4][1]) - 1, tok


def test_abi_and_function_lists_are_unchanged():
    fa = _lib()
    assert fa.lib.fa_abi_version() == 7 and fa.ABI_VERSION == 7
    assert re.search(r"#define\s+MI355FA_ABI_VERSION\s+7\b", open(os.path.join(ROOT, "include", "mi355fa.h")).read())
    counts = {"mi355fa_kvcache.h": 2, "mi355fa_kvcache_fp8.h": 2, "mi355fa_kvcache_fp4.h": 4, "mi355fa_ragged_fp4.h": 2,
              "mi355fa_ragged.h": 2, "mi355fa_paged.h": 2, "mi355fa_softcap.h": 4, "mi355fa_alibi.h": 4, "mi355fa_sink.h": 4}
    for name, n in counts.items():
        txt, _, functions = vck.header_functions(os.path.join(ROOT, "include", name))
        assert len(functions) == n, (name, functions)
        assert "fp8_token" not in txt, name
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(list(counts) + ["mi355fa.h", "mi355fa_local.h", "mi355fa_gqa.h",
                                                                                       "mi355fa_kvcache_fp8_token.h"])


def _e4m3_rule(wgs, S_cache, D):
    """the e4m3 path's split rule (the comment above kvcache_splits): 256 workgroups (512 at D = 64), splits of sqrt(64 S) keys;
    sqrt(16 S) at D = 256"""
    n = -(-(512 if D == 64 else 256) // wgs)
    by_len, keys = 1, 16 if D == 256 else 64
    while (by_len + 1) ** 2 * keys <= S_cache:
        by_len += 1
    return max(1, min(n, by_len, 64))


def test_workspace_follows_the_shared_formulas():
    fa = _lib()
    L = fa.lib
    shapes = ((1, 32, 8, 1, 4096, 128), (8, 32, 8, 1, 16384, 128), (8, 32, 8, 1, 16384, 64), (3, 4, 4, 130, 768, 64),
              (1, 8, 1, 1, 1 << 20, 64), (32, 32, 8, 1, 4096, 128))
    packed = ((8, 8, 32, 8, 128, 128, 128), (145, 32, 32, 8, 128, 128, 128), (1, 1, 4, 4, 1, 32, 64), (17, 300, 8, 1, 3, 32, 64),
              (8, 8, 16, 8, 128, 128, 256), (14, 6, 5, 1, 4, 96, 256))
    try:
        for n in (0, 1, 2, 7):
            vck.splits(n)
            for (B, H, Hkv, Sq, Sc, D) in shapes:
                for Sn in (0, 5):
                    got = L.fa_fwd_kvcache_fp8_token_workspace_bytes(B, H, Hkv, Sq, Sc, Sn, D)
                    k = n or _e4m3_rule(B * Hkv * (-(-(H // Hkv) * Sq // 32)), Sc, D)
                    assert got == (0 if k == 1 else k * B * H * Sq * (D + 2) * 4), (n, B, H, Hkv, Sq, Sc, D, got)
                    assert got == L.fa_fwd_kvcache_fp8_workspace_bytes(B, H, Hkv, Sq, Sc, Sn, D)      # the e4m3 rule
                    for page in (32, 128):
                        assert L.fa_fwd_kvcache_fp8_token_paged_workspace_bytes(B, H, Hkv, Sq, Sc // page, page, Sn, D) == got
            for (T, B, H, Hkv, MP, page, D) in packed:
                got = L.fa_fwd_kvcache_fp8_token_ragged_workspace_bytes(T, B, H, Hkv, MP, page, D)
                k = n or _e4m3_rule(Hkv * rc.nb_max(H // Hkv, T, B), MP * page, D)
                assert got == rc.workspace_bytes(k, T, B, H, Hkv, D) and got >= 32, (n, T, B, H, Hkv, MP, page, D, got)
                assert got == L.fa_fwd_kvcache_ragged_workspace_bytes(T, B, H, Hkv, MP, page, D, fa.PAGED_CACHE_FP8_E4M3)
    finally:
        vck.splits(0)
    W, WP, WR = (L.fa_fwd_kvcache_fp8_token_workspace_bytes, L.fa_fwd_kvcache_fp8_token_paged_workspace_bytes,
                 L.fa_fwd_kvcache_fp8_token_ragged_workspace_bytes)
    assert W(1, 4, 4, 1, 64, 0, 256) == SHAPE and WP(8, 16, 8, 1, 128, 128, 0, 256) == SHAPE     # D = 256: the packed call only
    assert WR(8, 8, 16, 8, 128, 128, 256) > 0
    for D in (96, 32, 512):
        assert W(1, 4, 4, 1, 64, 0, D) == HEAD_DIM and WP(1, 4, 4, 1, 4, 32, 0, D) == HEAD_DIM and WR(8, 8, 16, 8, 128, 128, D) == HEAD_DIM
    for page in (16, 0, 48):
        assert WP(1, 4, 4, 1, 4, page, 0, 64) == fa.ERR_PAGED and WR(8, 8, 16, 8, 128, page, 128) == fa.ERR_PAGED
    assert W(1, 6, 4, 1, 64, 0, 64) == fa.ERR_GROUP
    assert WR(0, 8, 16, 8, 128, 128, 128) == fa.ERR_RAGGED and WR(8, 0, 16, 8, 128, 128, 128) == fa.ERR_RAGGED


def test_bad_arguments_are_refused_before_launch():
    fa = _lib()
    L = fa.lib
    _buf, p = vck.aligned_ptr()
    S3 = lambda *s: ctypes.cast((ctypes.c_longlong * 3)(*s), ctypes.POINTER(ctypes.c_longlong))
    B, H, Hkv, Sq, Sc = 2, 8, 2, 1, 1024
    err = lambda: L.fa_last_error().decode()

    def padded(q=p, kc=p, vc=p, ks=p, vs=p, kn=None, vn=None, kss=None, vss=None, sinks=None, Sn=0, D=128, dt=fa.BF16, opts=None,
               ws=p, wsb=1 << 24, page=None, table=None, cu=None):
        return L.fa_fwd_kvcache_fp8_token(q, kc, vc, ks, vs, kn, vn, p, kss, vss, sinks, p, None, ws, wsb, B, H, Hkv, Sq, Sc, Sn,
                                          D, dt, 0.125, -1, -1, opts, None)

    def paged(q=p, kc=p, vc=p, ks=p, vs=p, kn=None, vn=None, kss=None, vss=None, sinks=None, Sn=0, D=128, dt=fa.BF16, opts=None,
              ws=p, wsb=1 << 24, page=64, table=p, cu=None):
        return L.fa_fwd_kvcache_fp8_token_paged(q, kc, vc, ks, vs, kn, vn, p, table, kss, vss, sinks, p, None, ws, wsb, B, H, Hkv,
                                                Sq, 40, page, 16, 16, Sn, D, dt, 0.125, -1, -1, opts, None)

    def packed(q=p, kc=p, vc=p, ks=p, vs=p, kn=None, vn=None, kss=None, vss=None, sinks=None, Sn=0, D=128, dt=fa.BF16, opts=None,
               ws=p, wsb=1 << 24, page=64, table=p, cu=p, T=11):
        return L.fa_fwd_kvcache_fp8_token_ragged(q, kc, vc, ks, vs, kn, vn, cu, p, table, kss, vss, sinks, p, None, ws, wsb, T, B,
                                                 H, Hkv, 40, page, 16, 16, D, dt, 0.125, -1, -1, opts, None)

    for n in (1, 4):
        vck.splits(n)
        try:
            for call, fn in ((padded, "fa_fwd_kvcache_fp8_token"), (paged, "fa_fwd_kvcache_fp8_token_paged"),
                             (packed, "fa_fwd_kvcache_fp8_token_ragged")):
                rows = Sc if call is padded else 64
                for D in (96, 32, 512):
                    assert call(D=D) == HEAD_DIM and err().startswith(fn + ": head dim"), (fn, D)
                if call is packed:
                    assert call(D=256, ws=None) == fa.ERR_WORKSPACE                # D = 256 passes every check up to the workspace
                else:
                    assert call(D=256) == SHAPE and err().startswith(fn + ": a per-token-scaled cache takes head dim 256 with packed"), fn
                assert call(ks=None) == NULL and call(vs=None) == NULL and err() == fn + ": NULL pointer"
                for off in (1, 2, 6):
                    assert call(ks=p + off) == ALIGN and err().startswith(fn + ": k_scale / v_scale must be 4-byte aligned"), (fn, off)
                    assert call(vs=p + off) == ALIGN, (fn, off)
                assert call(kc=p + 8) == ALIGN and "16-byte aligned" in err()
                assert call(kss=S3(Hkv * rows, rows, -1)) == STRIDE and err() == fn + ": the scale strides must be non-negative element strides (got -1)"
                assert call(vss=S3(-8, rows, 1)) == STRIDE
                assert call(kss=S3(0, 0, 1 << 30)) == STRIDE and "2^31 bytes" in err()
                keep = S3(Hkv * rows * 128, rows * 128, 136)                        # a cache row stride off 16 bytes
                assert call(opts=ctypes.byref(fa.Opts.make(k_strides=keep, v_strides=keep))) == STRIDE and "fp8 cache strides" in err()
                assert call(sinks=p + 2) == ALIGN and "sinks" in err()
                assert call(kn=p) == NULL and "k_new and v_new" in err()
                assert call(dt=2) == DTYPE
                if call is not packed:
                    assert call(Sn=2) == NULL and err() == fn + ": S_new > 0 needs k_new and v_new"
                    assert call(kn=p, vn=p, Sn=0) == SHAPE
                if call is not padded:
                    for page in (48, 16, 0):
                        assert call(page=page) == fa.ERR_PAGED and err() == fn + ": page_size must be a positive multiple of 32", (fn, page)
                    assert call(table=None) == NULL and "block_table" in err()
                    assert call(table=p + 2) == ALIGN
                if call is packed:
                    assert call(cu=None) == NULL and "cu_seqlens_q" in err()
                    assert call(T=0) == fa.ERR_RAGGED and call(cu=p + 2) == ALIGN
                if n > 1:   # every check passed (4-byte aligned scales, any non-negative scale strides): the workspace is the last
                    assert call(ws=None) == fa.ERR_WORKSPACE and call(wsb=16) == fa.ERR_WORKSPACE
                    assert call(ks=p + 4, kss=S3(rows * Hkv, 1, Hkv), vss=S3(0, 0, 0), ws=None) == fa.ERR_WORKSPACE
        finally:
            vck.splits(0)


# ---------------------------------------------------------------- the Python surface
def test_python_surface_and_refusals():
    T = _T()
    import _mi355fa_fp8_token_torch as ext
    assert T.__all__ == ["quantize_kv_fp8_per_token", "dequantize_kv_fp8_per_token", "flash_attention_kvcache_fp8_token",
                         "flash_attention_kvcache_fp8_token_paged", "flash_attention_kvcache_fp8_token_ragged"]
    sig = lambda f: str(inspect.signature(f))
    assert sig(T.quantize_kv_fp8_per_token) == "(x)"
    assert sig(T.dequantize_kv_fp8_per_token) == "(x8, scale, dtype=torch.float32)"
    tail = "k_new=None, v_new=None, is_causal=False, window_size=(-1, -1), softmax_scale=None, return_lse=False, sinks=None"
    assert sig(T.flash_attention_kvcache_fp8_token) == "(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, %s)" % tail
    assert sig(T.flash_attention_kvcache_fp8_token_paged) == "(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, block_table, %s)" % tail
    assert sig(T.flash_attention_kvcache_fp8_token_ragged) == (
        "(q, k_cache, v_cache, k_scale, v_scale, cu_seqlens_q, cache_seqlens, block_table, %s, out=None)" % tail)
    assert hasattr(ext, "kvcache_fp8_token_forward") and hasattr(ext, "kvcache_fp8_token_ragged_forward")
    # the recorded surfaces of the other modules are as they were
    import fp4_kvcache, fp4_ragged_kvcache, paged_kvcache, ragged_kvcache
    assert fp4_kvcache.__all__ == ["quantize_kv_mxfp4", "dequantize_kv_mxfp4", "flash_attention_kvcache_fp4", "flash_attention_kvcache_fp4_paged"]
    assert fp4_ragged_kvcache.__all__ == ["flash_attention_kvcache_fp4_ragged"] and ragged_kvcache.__all__ == ["flash_attention_kvcache_ragged"]
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    c8 = lambda *s: torch.zeros(*s, dtype=torch.uint8).view(F8)
    q, sl = mk(2, 8, 1, 64), torch.zeros(2, dtype=torch.int32)
    kc, ks = c8(2, 2, 128, 64), torch.ones(2, 2, 128)
    call = T.flash_attention_kvcache_fp8_token
    with pytest.raises(AssertionError, match="float8_e4m3fn"):
        call(q, kc.view(torch.uint8), kc.view(torch.uint8), ks, ks, sl)
    with pytest.raises(AssertionError, match="float8_e4m3fn"):
        call(q, mk(2, 2, 128, 64), mk(2, 2, 128, 64), ks, ks, sl)
    with pytest.raises(AssertionError, match="k_scale and v_scale must be float32"):
        call(q, kc, kc, ks.half(), ks.half(), sl)
    with pytest.raises(AssertionError, match="the caches' shape without D"):
        call(q, kc, kc, ks[..., None], ks[..., None], sl)
    with pytest.raises(AssertionError, match="the caches' shape without D"):
        call(q, kc, kc, ks[:, :, :64], ks, sl)
    with pytest.raises(AssertionError, match="q must not require grad"):
        call(q.clone().requires_grad_(True), kc, kc, ks, ks, sl)
    with pytest.raises(AssertionError, match="k_scale must not require grad"):
        call(q, kc, kc, ks.clone().requires_grad_(True), ks, sl)
    with pytest.raises(AssertionError, match="k_new must not require grad"):
        call(q, kc, kc, ks, ks, sl, k_new=mk(2, 2, 1, 64).requires_grad_(True), v_new=mk(2, 2, 1, 64))
    with pytest.raises(AssertionError, match="sinks must not require grad"):
        call(q, kc, kc, ks, ks, sl, sinks=torch.zeros(8, requires_grad=True))
    with pytest.raises(AssertionError, match="together"):
        call(q, kc, kc, ks, ks, sl, k_new=mk(2, 2, 1, 64))
    with pytest.raises(AssertionError, match="64 or 128"):
        call(mk(2, 8, 1, 256), c8(2, 2, 128, 256), c8(2, 2, 128, 256), ks, ks, sl)
    with pytest.raises(AssertionError, match="window_right"):
        call(q, kc, kc, ks, ks, sl, is_causal=True, window_size=(-1, 2))
    with pytest.raises(AssertionError, match="softmax_scale must be finite"):
        call(q, kc, kc, ks, ks, sl, softmax_scale=0.0)
    with pytest.raises(TypeError):
        call(q, kc, kc, ks, ks, sl, softcap=30.0)
    with pytest.raises(AssertionError, match="device tensors"):
        call(q, kc, kc, ks, ks, sl)                                             # CPU tensors reach the binding and stop there
    with pytest.raises(AssertionError, match="head dim 64 or 128"):
        ext.kvcache_fp8_token_forward(mk(2, 8, 1, 256), c8(2, 2, 128, 256), c8(2, 2, 128, 256), ks, ks, sl, None, None, None, -1, -1, 0.0, None)
    bt = torch.zeros(2, 4, dtype=torch.int32)
    pg = T.flash_attention_kvcache_fp8_token_paged
    with pytest.raises(AssertionError, match="device tensor"):
        pg(q, kc, kc, ks, ks, sl, bt)
    with pytest.raises(AssertionError, match="int32"):
        pg(q, kc, kc, ks, ks, sl, bt.long())
    rg_ = T.flash_attention_kvcache_fp8_token_ragged
    qp, cu = mk(5, 8, 64), torch.tensor([0, 2, 5], dtype=torch.int32)
    kp, ksp = c8(8, 2, 64, 64), torch.ones(8, 2, 64)
    with pytest.raises(AssertionError, match="cu_seqlens_q must be a device tensor"):
        rg_(qp, kp, kp, ksp, ksp, cu, sl, bt)
    with pytest.raises(AssertionError, match="cu_seqlens_q must be a device tensor"):    # D = 256 passes the wrapper's checks
        rg_(mk(5, 8, 256), c8(8, 2, 64, 256), c8(8, 2, 64, 256), ksp, ksp, cu, sl, bt)
    with pytest.raises(AssertionError, match="64 or 128 or 256"):
        rg_(mk(5, 8, 96), c8(8, 2, 64, 96), c8(8, 2, 64, 96), ksp, ksp, cu, sl, bt)
    with pytest.raises(AssertionError, match="multiple of 32"):
        rg_(qp, c8(8, 2, 48, 64), c8(8, 2, 48, 64), torch.ones(8, 2, 48), torch.ones(8, 2, 48), cu, sl, bt)
    with pytest.raises(AssertionError, match="multiple of 32"):
        pg(q, c8(8, 2, 48, 64), c8(8, 2, 48, 64), torch.ones(8, 2, 48), torch.ones(8, 2, 48), sl, bt)
    with pytest.raises(AssertionError, match="out must have q's dtype"):
        rg_(qp, kp, kp, ksp, ksp, cu, sl, bt, out=torch.zeros(5, 8, 64, dtype=torch.bfloat16))
    with pytest.raises(AssertionError, match="float8_e4m3fn"):
        rg_(qp, kp.view(torch.uint8), kp.view(torch.uint8), ksp, ksp, cu, sl, bt)
    with pytest.raises(AssertionError, match="device tensors"):
        ext.kvcache_fp8_token_ragged_forward(qp, kp, kp, ksp, ksp, cu, sl, bt, None, None, -1, -1, 0.0, None, None)


# ---------------------------------------------------------------- the quantiser
E4M3 = np.array([0.0] + [2.0 ** -9 * m for m in range(1, 8)] +
                [2.0 ** (e - 7) * (1 + m / 8) for e in range(1, 16) for m in range(8)][:-1], dtype=np.float64)   # 0 .. 448: 127 values


def np_quantize(x):
    """the header's quantiser on fp64 rows x [n, D] holding fp32 values: (bytes uint8 [n, D], scales float32 [n])"""
    assert E4M3.size == 127 and E4M3[-1] == 448.0 and E4M3[8] == 2.0 ** -6
    x32 = x.astype(np.float32)
    amax = np.abs(x32).max(axis=1)
    s = (amax / np.float32(448.0)).astype(np.float32)
    normal = (s >= np.finfo(np.float32).tiny) & np.isfinite(s)
    s = np.where(normal, s, np.float32(1.0)).astype(np.float32)
    y = np.clip((x32 / s[:, None]).astype(np.float32).astype(np.float64), -448.0, 448.0)
    a = np.abs(y)
    hi = np.searchsorted(E4M3, a, side="left").clip(max=126)                     # E4M3[hi - 1] < a <= E4M3[hi]
    lo = (hi - 1).clip(min=0)
    dl, dh = a - E4M3[lo], E4M3[hi] - a
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))   # ties to the even code
    code = np.where(a == E4M3[hi], hi, code)
    return (code | (np.signbit(y).astype(np.int64) << 7)).astype(np.uint8), s


def _rows():
    g = torch.Generator().manual_seed(0)
    D = 64
    rows = [torch.randn(40, D, generator=g) * torch.exp2(torch.randint(-12, 12, (40, 1), generator=g).float())]
    zero = torch.zeros(1, D)
    sub = torch.zeros(1, D)
    sub[0, 3], sub[0, 9] = 2.0 ** -120, -2.0 ** -125                             # amax / 448 is subnormal: scale 1.0
    out = torch.randn(1, D, generator=g)
    out[0, 17] = 2.0 ** 12                                                       # one outlier
    # ties at e4m3 midpoints once the row's scale is 1.0 (amax = 448): (E4M3[i] + E4M3[i + 1]) / 2, both signs
    mids = torch.tensor((E4M3[:-1] + E4M3[1:]) / 2, dtype=torch.float32)
    ties = torch.cat([mids, -mids, torch.tensor([448.0, -448.0])])               # 254 values: four rows of 64
    ties = torch.cat([ties, torch.zeros(256 - ties.numel())]).view(4, D)
    ties[:, 0] = 448.0
    neg0 = torch.randn(1, D, generator=g)
    neg0[0, ::2] = -0.0
    # saturation through rounding only: amax 448.0000305 gives s slightly above 1, x / s below 448 that rounds up to it,
    # and values between 432 and 448 that round to 448 without ever exceeding it
    sat = torch.full((1, D), 447.9)
    sat[0, 0], sat[0, 1], sat[0, 2], sat[0, 3] = 448.00003, -448.00003, 440.0001, -463.9
    sat[0, 3] = -447.99
    return torch.cat([rows[0], zero, sub, out, ties, neg0, sat]), dict(zero=40, sub=41, out=42, ties=43, neg0=47, sat=48)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
def test_quantiser_matches_the_numpy_reference_element_for_element(dtype):
    T = _T()
    x, at = _rows()
    if dtype != torch.float32:
        x = x.clamp(-60000, 60000).to(dtype)
    x8, s = T.quantize_kv_fp8_per_token(x)
    assert x8.dtype == F8 and x8.shape == x.shape and s.dtype == torch.float32 and s.shape == x.shape[:-1]
    want8, wants = np_quantize(x.double().numpy())
    got8 = x8.view(torch.uint8).numpy()
    assert np.array_equal(s.numpy().view(np.int32), wants.view(np.int32)), np.nonzero(s.numpy() != wants)
    bad = np.nonzero(got8 != want8)
    assert bad[0].size == 0, [(int(i), int(j), float(x[i, j]), hex(got8[i, j]), hex(want8[i, j])) for i, j in zip(*bad)][:10]
    assert float(s[at["zero"]]) == 1.0 and (got8[at["zero"]] == 0).all()
    assert (got8 & 0x7F).max() == 0x7E                                           # the amax of a row lands on 448
    if dtype == torch.float32:
        assert float(s[at["sub"]]) == 1.0 and (got8[at["sub"]] == np.where(np.signbit(x[at["sub"]].numpy()), 0x80, 0)).all()
        assert float(s[at["out"]]) == float(np.float32(2.0 ** 12) / np.float32(448.0))
        assert (s[at["ties"]:at["ties"] + 4] == 1.0).all()
        t8 = got8[at["ties"]:at["ties"] + 4].reshape(-1)[1:]                     # (element 0 of each row is the 448 that pins the scale)
        assert ((t8 & 1) == 0).mean() > 0.9                                      # midpoints go to the even code
        assert (got8[at["sat"]] & 0x7F).max() == 0x7E and float(s[at["sat"]]) > 1.0
    n0 = got8[at["neg0"], ::2]
    assert (n0 == 0x80).all()                                                    # -0.0 kept


def test_quantise_any_shape_and_dequantise_is_idempotent():
    T = _T()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 5, 128, generator=g, dtype=torch.float64) * 7
    x8, s = T.quantize_kv_fp8_per_token(x)
    assert x8.shape == x.shape and s.shape == (2, 3, 5)
    y = T.dequantize_kv_fp8_per_token(x8, s)
    assert y.dtype == torch.float32 and (y - x.float()).abs().max() <= x.abs().amax() / 16
    y8, s2 = T.quantize_kv_fp8_per_token(y)
    assert torch.equal(y8.view(torch.uint8), x8.view(torch.uint8)) and torch.equal(s2, s)       # on its own output
    assert torch.equal(T.dequantize_kv_fp8_per_token(y8, s2), y)
    assert T.dequantize_kv_fp8_per_token(x8, s, torch.bfloat16).dtype == torch.bfloat16
    x1 = torch.randn(64, generator=g)
    a8, a = T.quantize_kv_fp8_per_token(x1)
    assert a8.shape == (64,) and a.shape == ()
    with pytest.raises(AssertionError):
        T.quantize_kv_fp8_per_token(torch.zeros(4, 64, dtype=torch.int32))
    with pytest.raises(AssertionError):
        T.dequantize_kv_fp8_per_token(x8, s[..., :4])


# ---------------------------------------------------------------- the kernels
def test_new_kernels_are_in_the_library_inside_the_decode_budget():
    """<T, D, SINK, TOKEN = true> overloads of the three decode kernel names (D = 64, 128; packed: also 256), two dtypes, plain
    and SINK, and <T, TOKEN = true> overloads of the three append names: workgroup 256, VGPR + AGPR <= 256, no scratch, no
    spills, LDS within 80 KiB."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj
    found, appends = {}, {}
    for k in codeobj.kernels():
        m = re.match(r"_ZN2fa\d+(fa_decode_(?:mod|paged|ragged)_kernel)INS_\d+(BF16|FP16)ELi(\d+)ELb([01])ELb1EEE", k["name"])
        if m:
            found[m.group(1), int(m.group(3))] = found.get((m.group(1), int(m.group(3))), 0) + 1
            assert k["wg"] == 256 and k["vgpr"] + k["agpr"] <= 256, (k["name"], k["vgpr"], k["agpr"])
            assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 81920, k["name"]
        m = re.match(r"_ZN2fa\d+(fa_kvcache_append(?:_paged|_ragged)?_kernel)INS_\d+(BF16|FP16)ELb1EEE", k["name"])
        if m:
            appends[m.group(1)] = appends.get(m.group(1), 0) + 1
            assert k["wg"] == 256 and k["scratch"] == 0 and k["spill"] == 0, k["name"]
    assert found == {("fa_decode_mod_kernel", 64): 4, ("fa_decode_mod_kernel", 128): 4, ("fa_decode_paged_kernel", 64): 4,
                     ("fa_decode_paged_kernel", 128): 4, ("fa_decode_ragged_kernel", 64): 4, ("fa_decode_ragged_kernel", 128): 4,
                     ("fa_decode_ragged_kernel", 256): 4}, found
    assert appends == {"fa_kvcache_append_kernel": 2, "fa_kvcache_append_paged_kernel": 2, "fa_kvcache_append_ragged_kernel": 2}, appends
