"""CPU tests of the FP8 KV-cache decoding boundary: include/mi355fa_kvcache_fp8.h declares exactly two entry points and
MI355FA_KV_FP8_E4M3, libmi355fa.so and the ctypes tables export them (a table of their own, KVCACHE_FP8_SIGNATURES, as the
soft-cap and ALiBi headers have: SIGNATURES is the table tests/test_host_scale.py enumerates), the ABI version and the
older headers are untouched, every argument error is refused before anything is launched, the workspace follows the
documented formula, the Python function refuses what it must, and quantize_kv_fp8 is the documented divide-clamp-RNE cast.
No compute is launched here (no GPU)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "mi355fa_kvcache_fp8.h")
NAMES = ["fa_fwd_kvcache_fp8", "fa_fwd_kvcache_fp8_workspace_bytes"]


def _functions():
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fa_[a-z0-9_]+)\s*\(", txt)))


def _lib():
    import _mi355fa as fa
    fa.lib.fa_debug_kvcache_splits.argtypes = [ctypes.c_int]
    fa.lib.fa_debug_kvcache_splits.restype = None
    return fa


def test_header_declares_the_fp8_entry_points():
    assert _functions() == NAMES
    txt = open(HDR).read()
    assert '#include "mi355fa_kvcache.h"' in txt
    assert re.search(r"#define\s+MI355FA_KV_FP8_E4M3\s+0\b", txt)
    assert "fa_debug" not in txt
    for older in ("mi355fa.h", "mi355fa_kvcache.h"):
        assert "fp8" not in open(os.path.join(ROOT, "include", older)).read().lower(), older


def test_library_and_ctypes_export_the_fp8_entry_points():
    fa = _lib()
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in fa.KVCACHE_FP8_SIGNATURES and name in fa.ALL_SIGNATURES, name
    # fa_fwd_kvcache + (k_descale, v_descale, descale_bstride) after cache_seqlens and kv_dtype after dtype
    a, b = fa.KVCACHE_FP8_SIGNATURES["fa_fwd_kvcache_fp8"][1], fa.SIGNATURES["fa_fwd_kvcache"][1]
    i = b.index(ctypes.c_float)
    assert a == b[:6] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong] + b[6:i] + [ctypes.c_int] + b[i:]
    assert len(a) == 27
    assert fa.KVCACHE_FP8_SIGNATURES["fa_fwd_kvcache_fp8_workspace_bytes"] == fa.SIGNATURES["fa_fwd_kvcache_workspace_bytes"]
    assert fa.KV_FP8_E4M3 == 0
    assert fa.lib.fa_abi_version() == 7


def _ptr():
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_bad_arguments_are_refused_before_launch():
    fa = _lib()
    L = fa.lib
    _buf, p = _ptr()
    fa.lib.fa_debug_kvcache_splits(4)      # a split count that needs a workspace at any shape
    try:
        B, H, Hkv, Sq, Sc, D = 2, 8, 2, 1, 1024, 64
        need = L.fa_fwd_kvcache_fp8_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D)
        assert need == 4 * B * H * Sq * (D + 2) * 4

        def call(q=p, kc=p, vc=p, kn=None, vn=None, sl=p, kd=p, vd=p, dbs=Hkv, o=p, ws=p, wsb=need, B=B, H=H, Hkv=Hkv,
                 Sq=Sq, Sc=Sc, Sn=0, D=D, dt=fa.BF16, kvdt=fa.KV_FP8_E4M3, scale=0.125, wl=-1, wr=-1, opts=None):
            return L.fa_fwd_kvcache_fp8(q, kc, vc, kn, vn, sl, kd, vd, dbs, o, None, ws, wsb, B, H, Hkv, Sq, Sc, Sn, D, dt,
                                        kvdt, scale, wl, wr, opts, None)

        for kw in ({"q": None}, {"kc": None}, {"vc": None}, {"sl": None}, {"o": None}, {"kn": p}, {"Sn": 3}):
            assert call(**kw) == -1, kw                                   # MI355FA_ERR_NULL
        for kw in ({"B": 0}, {"H": 0}, {"Sq": 0}, {"Sc": 0}, {"Sn": 2, "kn": p, "vn": p, "B": -1}, {"Sn": -1},
                   {"scale": 0.0}, {"scale": -1.0}, {"scale": float("nan")}, {"scale": float("inf")}):
            assert call(**kw) == -2, kw                                   # MI355FA_ERR_SHAPE
        assert call(kn=p, vn=p, Sn=0) == -2                               # k_new with S_new = 0
        for dbs in (1, Hkv - 1, -1, -Hkv):                                # neither 0 nor >= H_kv
            assert call(dbs=dbs) == -2, dbs
            assert b"descale_bstride" in L.fa_last_error()
        assert call(D=96) == -3                                           # MI355FA_ERR_HEAD_DIM
        assert call(dt=2) == -4                                           # MI355FA_ERR_DTYPE
        for kvdt in (1, 2, -1):
            assert call(kvdt=kvdt) == -4, kvdt
            assert b"kv_dtype" in L.fa_last_error()
        for kw in ({"q": p + 8}, {"kc": p + 8}, {"vc": p + 4}, {"kd": p + 2}, {"vd": p + 1}):
            assert call(**kw) == -5, kw                                   # MI355FA_ERR_ALIGN
        for kw in ({"Hkv": 0}, {"Hkv": 3}, {"H": 6, "Hkv": 4}):
            assert call(**kw) == fa.ERR_GROUP, kw
        for kw in ({"wl": -2}, {"wr": -3}):
            assert call(**kw) == fa.ERR_WINDOW, kw
        assert call(wsb=need - 1) == fa.ERR_WORKSPACE
        assert call(ws=None) == fa.ERR_WORKSPACE
        cu = ctypes.c_int(0)
        for opts in (fa.Opts.make(cu_seqlens_q=ctypes.addressof(cu), cu_seqlens_k=ctypes.addressof(cu), total_q=1, total_k=1),
                     fa.Opts.make(p_drop=0.25, seed=1), fa.Opts.make(q_scaled=p)):
            assert call(opts=ctypes.byref(opts)) == -2
        S3 = lambda *s: ctypes.cast((ctypes.c_longlong * 3)(*s), ctypes.POINTER(ctypes.c_longlong))
        # cache strides are bytes here and must be multiples of 16: a multiple of 8 is what the 16-bit call takes
        for bad in ((Sc * Hkv * D, D, Hkv * D + 8), (Sc * Hkv * D + 8, D, Hkv * D), (Sc * Hkv * D, D + 8, Hkv * D),
                    (Sc * Hkv * D, D, D - 16)):
            keep = S3(*bad)
            st = fa.Opts.make(k_strides=keep, v_strides=keep)
            assert call(opts=ctypes.byref(st)) == -6, bad                 # MI355FA_ERR_STRIDE
        keep = S3(Sc * Hkv * D, D, Hkv * D)                               # K and V with different row strides
        st2 = fa.Opts.make(k_strides=keep)
        assert call(opts=ctypes.byref(st2)) == -6
        assert b"sequence stride" in L.fa_last_error()
    finally:
        fa.lib.fa_debug_kvcache_splits(0)


def test_workspace_follows_the_documented_formula():
    fa = _lib()
    L = fa.lib
    try:
        for n in (1, 2, 7, 64):
            fa.lib.fa_debug_kvcache_splits(n)                             # the debug override pins the fp8 count too
            for (B, H, Hkv, Sq, Sc, D) in ((1, 32, 8, 1, 4096, 128), (3, 4, 4, 130, 777, 64), (8, 8, 1, 3, 64, 128)):
                want = 0 if n == 1 else n * B * H * Sq * (D + 2) * 4
                assert L.fa_fwd_kvcache_fp8_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D) == want
                assert L.fa_fwd_kvcache_fp8_workspace_bytes(B, H, Hkv, Sq, Sc, 5, D) == want
        fa.lib.fa_debug_kvcache_splits(0)
        # the fp8 rule: at most 256 workgroups (512 at D = 64) over (batch, K/V head, 32-row block, split),
        # n <= sqrt(S_cache / 64), at most 64 splits
        for (B, H, Hkv, Sq, Sc, D, n) in ((1, 32, 8, 1, 131072, 128, 32), (8, 32, 8, 1, 16384, 128, 4),
                                          (32, 32, 8, 1, 4096, 128, 1), (1, 32, 8, 1, 4096, 128, 8),
                                          (1, 32, 8, 1, 32768, 128, 22), (8, 32, 1, 1, 16384, 128, 16),
                                          (8, 32, 8, 1, 16384, 64, 8), (1, 4, 4, 1, 200, 64, 1),
                                          (1, 8, 1, 1, 1 << 20, 64, 64), (1, 32, 8, 130, 65536, 128, 2)):
            got = L.fa_fwd_kvcache_fp8_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D)
            assert got == (0 if n == 1 else n * B * H * Sq * (D + 2) * 4), (B, H, Hkv, Sq, Sc, D, got)
        assert L.fa_fwd_kvcache_fp8_workspace_bytes(1, 6, 4, 1, 64, 0, 64) == fa.ERR_GROUP
        assert L.fa_fwd_kvcache_fp8_workspace_bytes(1, 4, 4, 1, 64, 0, 96) == -3
        assert L.fa_fwd_kvcache_fp8_workspace_bytes(1, 4, 4, 0, 64, 0, 64) == -2
    finally:
        fa.lib.fa_debug_kvcache_splits(0)


def test_python_surface():
    import My_FlashAttention_optimized as M
    import _mi355fa_torch as ext
    assert str(inspect.signature(M.flash_attention_kvcache_fp8)) == (
        "(q, k_cache, v_cache, cache_seqlens, k_descale=None, v_descale=None, k_new=None, v_new=None, is_causal=False, "
        "window_size=(-1, -1), softmax_scale=None, return_lse=False)")
    assert str(inspect.signature(M.quantize_kv_fp8)) == "(x, descale=None)"
    assert hasattr(ext, "kvcache_fp8_forward")
    doc = M.flash_attention_kvcache_fp8.__doc__
    for phrase in ("float8_e4m3fn", "k_descale", "bottom-right", "L_b - S_q + i", "no backward", "LSE = -inf"):
        assert phrase in doc, phrase


def test_python_refuses_wrong_dtypes_shapes_and_grad():
    import My_FlashAttention_optimized as M
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    q, sl = mk(2, 8, 1, 64), torch.zeros(2, dtype=torch.int32)
    c8 = torch.zeros(2, 2, 128, 64).to(torch.float8_e4m3fn)
    for bad in (torch.float8_e4m3fnuz, torch.float8_e5m2, torch.uint8, torch.float16, torch.bfloat16):
        c = torch.zeros(2, 2, 128, 64).to(bad)
        with pytest.raises(AssertionError, match="float8_e4m3fn "):
            M.flash_attention_kvcache_fp8(q, c, c, sl)
        with pytest.raises(AssertionError, match="float8_e4m3fn "):
            M.flash_attention_kvcache_fp8(q, c8, c, sl)
    ok = torch.ones(2, 2)
    for bad in (torch.ones(2, 3), torch.ones(3), torch.ones(2, 2, 1), torch.ones(2, 2, dtype=torch.float64)):
        with pytest.raises(AssertionError, match="k_descale"):
            M.flash_attention_kvcache_fp8(q, c8, c8, sl, k_descale=bad, v_descale=ok)
        with pytest.raises(AssertionError, match="v_descale"):
            M.flash_attention_kvcache_fp8(q, c8, c8, sl, k_descale=ok, v_descale=bad)
    with pytest.raises(AssertionError, match="together"):
        M.flash_attention_kvcache_fp8(q, c8, c8, sl, k_new=mk(2, 2, 1, 64))
    with pytest.raises(AssertionError, match="together"):
        M.flash_attention_kvcache_fp8(q, c8, c8, sl, v_new=mk(2, 2, 1, 64))
    with pytest.raises(AssertionError, match="backward"):
        M.flash_attention_kvcache_fp8(q.clone().requires_grad_(True), c8, c8, sl)
    with pytest.raises(AssertionError, match="backward"):
        M.flash_attention_kvcache_fp8(q, c8, c8, sl, k_new=mk(2, 2, 1, 64).requires_grad_(True), v_new=mk(2, 2, 1, 64))
    with pytest.raises(AssertionError, match="device"):
        M.flash_attention_kvcache_fp8(q, c8, c8, sl, k_descale=ok, v_descale=torch.ones(2))
    with pytest.raises(AssertionError, match="window_right"):
        M.flash_attention_kvcache_fp8(q, c8, c8, sl, is_causal=True, window_size=(-1, 2))


def test_cpp_binding_refuses_bad_arguments():
    import _mi355fa_torch as ext
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    sl = torch.zeros(2, dtype=torch.int32)
    q, c8 = mk(2, 8, 1, 64), torch.zeros(2, 2, 128, 64).to(torch.float8_e4m3fn)
    cases = [((q, c8, c8, sl), {}, "device tensors"),
             ((q, mk(2, 2, 128, 64), mk(2, 2, 128, 64), sl), {}, "float8_e4m3fn"),
             ((q, c8.view(torch.uint8), c8.view(torch.uint8), sl), {}, "float8_e4m3fn"),
             ((q, c8[:, :1].expand(2, 3, 128, 64), c8[:, :1].expand(2, 3, 128, 64), sl), {}, "multiple"),
             ((q, c8, c8[:, :, :64], sl), {}, "same shape"),
             ((mk(2, 8, 1, 128), c8, c8, sl), {}, "head dim"),
             ((q, c8, c8, sl), {"k_new": mk(2, 2, 1, 64)}, "together"),
             ((q, c8, c8, sl), {"window_left": -4}, ">= -1")]
    for args, kw, msg in cases:
        with pytest.raises(AssertionError, match=msg):
            ext.kvcache_fp8_forward(*args, **kw)


def _expr(x, d):
    """the documented cast: d broadcast over [B, H_kv, S, D]"""
    return (x.float() / d.reshape(-1, x.shape[1], 1, 1)).clamp(-448, 448).to(torch.float8_e4m3fn)


def test_quantize_kv_fp8_is_divide_clamp_rne():
    import My_FlashAttention_optimized as M
    g = torch.Generator().manual_seed(3)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        x = (torch.randn(3, 2, 37, 64, generator=g) * torch.logspace(-4, 2, 64)).to(dtype)
        x8, d = M.quantize_kv_fp8(x)
        assert x8.dtype == torch.float8_e4m3fn and x8.shape == x.shape
        assert d.dtype == torch.float32 and d.shape == (3, 2)
        want_d = x.float().abs().amax(dim=(2, 3)) / 448
        assert torch.equal(d, want_d)
        assert torch.equal(x8.view(torch.uint8), _expr(x, d).view(torch.uint8))
        # the row maximum lands on +-448 exactly, and small values reach the subnormal codes
        u = x8.view(torch.uint8)
        assert ((u & 0x7F) == 0x7E).any() and (((u & 0x7F) >= 1) & ((u & 0x7F) <= 7)).any()
        # a given descale, (B, H_kv) and (H_kv,)
        for dd in (torch.rand(3, 2, generator=g) * 0.01 + 1e-3, torch.rand(2, generator=g) * 0.01 + 1e-3):
            y8, d2 = M.quantize_kv_fp8(x, dd)
            assert d2 is dd
            assert torch.equal(y8.view(torch.uint8), _expr(x, dd).view(torch.uint8))
    # all-zero heads get descale 1
    z8, dz = M.quantize_kv_fp8(torch.zeros(1, 2, 4, 64))
    assert torch.equal(dz, torch.ones(1, 2)) and (z8.view(torch.uint8) == 0).all()


def test_quantize_kv_fp8_saturates_and_keeps_signed_zero():
    import My_FlashAttention_optimized as M
    x = torch.tensor([1000.0, -1000.0, 448.0, 464.0, 465.0, 1e30, -0.0, 0.0, 2.0 ** -10, 2.0 ** -10 * 1.0001, 3 * 2.0 ** -10,
                      -(2.0 ** -9), 2.0 ** -11]).repeat(1, 1, 1, 1)
    one = torch.ones(1, 1)
    assert torch.isnan(x.to(torch.float8_e4m3fn).float()).any()            # torch's own cast does not saturate
    x8, _ = M.quantize_kv_fp8(x, one)
    assert not torch.isnan(x8.float()).any()
    #        1000   -1000  448   464   465   1e30  -0    0     tie->even(0)  above tie  tie->even(2)  -min   below half
    want = [0x7E, 0xFE, 0x7E, 0x7E, 0x7E, 0x7E, 0x80, 0x00, 0x00, 0x01, 0x02, 0x81, 0x00]
    assert x8.view(torch.uint8).flatten().tolist() == want


def test_quantize_kv_fp8_round_trips_every_finite_code():
    import My_FlashAttention_optimized as M
    codes = torch.tensor([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8)
    assert codes.numel() == 254
    vals = codes.view(torch.float8_e4m3fn).float()
    assert torch.isfinite(vals).all()
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        x = vals.to(dtype)
        assert torch.equal(x.float(), vals)                                # every e4m3 value is exact in fp16 and bf16
        x8, _ = M.quantize_kv_fp8(x.reshape(1, 1, 1, -1), torch.ones(1, 1))
        assert torch.equal(x8.view(torch.uint8).flatten(), codes)
