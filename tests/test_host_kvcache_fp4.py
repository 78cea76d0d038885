"""CPU tests of the MXFP4 KV-cache decoding boundary (include/mi355fa_kvcache_fp4.h, fp4_kvcache.py): quantize_kv_mxfp4 is the
documented quantiser, element for element against an independent numpy reference; its round trip is exact in the input's
dtype (the condition under which the kernel's conversions are exact) and idempotent; the header declares and the library
exports exactly the four entry points, with the older headers and the ABI version untouched; the workspace functions follow
the fp8 path's formula; and every argument error is refused with its code and text before anything is launched.  No compute
is launched here (no GPU)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import variantcheck as vck
from conftest import ROOT

HDR = os.path.join(ROOT, "include", "mi355fa_kvcache_fp4.h")
NAMES = ["fa_fwd_kvcache_fp4", "fa_fwd_kvcache_fp4_paged", "fa_fwd_kvcache_fp4_paged_workspace_bytes",
         "fa_fwd_kvcache_fp4_workspace_bytes"]
NULL, SHAPE, HEAD_DIM, DTYPE, ALIGN, STRIDE = -1, -2, -3, -4, -5, -6
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
TIE_CODES = [0, 2, 2, 4, 4, 6, 6]               # each tie goes to the neighbour whose mantissa bit is 0
DTYPES = [torch.float16, torch.bfloat16]


def _F():
    import fp4_kvcache as F
    return F


def _lib():
    import _mi355fa as fa
    return fa


# ---------------------------------------------------------------- the quantiser
def np_quantize(x):
    """The header's quantiser on a float64 array [..., D], by another route than fp4_kvcache.py's: frexp for the exponent,
    a nearest-grid-point search with the tie sent to the even code for the rounding.  Returns (codes [..., D], e [..., D/32])."""
    D = x.shape[-1]
    xb = x.reshape(-1, 32)
    amax = np.abs(xb).max(axis=1)
    _, ex = np.frexp(amax)                                   # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = np.clip(ex - 1 - 2 + 127, 0, 254)
    e[amax == 0] = 127
    y = np.abs(xb) / np.ldexp(1.0, e - 127)[:, None]        # exact: a power of two
    d = np.abs(y[..., None] - GRID)
    near = d == d.min(axis=-1, keepdims=True)                # one or two grid points
    lo, hi = near.argmax(axis=-1), 7 - near[..., ::-1].argmax(axis=-1)
    code = np.where(lo % 2 == 0, lo, hi)                     # a single nearest point: lo == hi; a tie: the even one of the two
    code = np.where(y > 6.0, 7, code)                        # (saturation: the search already gives 7)
    sign = np.signbit(xb) & (amax != 0)[:, None]
    code = code + 8 * sign
    return code.reshape(x.shape).astype(np.uint8), e.reshape(*x.shape[:-1], D // 32).astype(np.uint8)


def unpack(packed):
    p = packed.numpy()
    return np.stack([p & 0xF, p >> 4], axis=-1).reshape(*p.shape[:-1], p.shape[-1] * 2)


def cases(dtype):
    """[n, 32] blocks of `dtype`: the inputs the issue names"""
    fi = torch.finfo(dtype)
    tiny_sub = torch.tensor([1], dtype=torch.int16).view(dtype).item()          # the smallest subnormal
    rows = []
    codes = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    rows.append(codes + [-c for c in codes] + codes + [-c for c in codes])      # all 16 nibble values (amax 6: X = 0)
    for k in (-9, -3, 0, 2, 7):                                                  # every tie, times a power of two (amax 4 * 2^k)
        s = 2.0 ** k
        rows.append([4.0 * s] + [t * s for t in TIES] + [-t * s for t in TIES] + [0.0] * 17)
    rows.append([4.0, 6.0, 7.0, 7.5, 7.9, -7.0, -7.9, 6.5, 5.5, -6.5] + [1.0] * 22)     # saturation inside a block of X = 0
    rows.append([-0.0, 0.0, 1.0, -1.0] * 8)                                      # -0.0 beside nonzeros
    rows.append([0.0] * 32)                                                      # an all-zero block
    rows.append([-0.0] * 16 + [0.0] * 16)                                        # and one of signed zeros
    rows.append([fi.max, -fi.max, fi.max / 2, fi.max / 3, 1.0, 0.0] + [fi.max / 7] * 26)  # amax at the largest finite
    rows.append([tiny_sub, -tiny_sub, 0.0, 3 * tiny_sub] + [2 * tiny_sub] * 28)  # ... and at the subnormal end
    rows.append([tiny_sub] + [0.0] * 31)
    rows.append([fi.tiny, fi.tiny / 2, -fi.tiny * 1.5, 0.0] * 8)                 # around the smallest normal
    x = torch.tensor(rows, dtype=torch.float64).to(dtype)
    g = torch.Generator().manual_seed(1)
    rnd = (torch.randn(64, 32, generator=g) * torch.exp2(torch.randint(-20, 15, (64, 1), generator=g).float())).to(dtype)
    return torch.cat([x, rnd])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_quantiser_matches_the_numpy_reference_element_for_element(dtype):
    F = _F()
    x = cases(dtype)
    assert torch.isfinite(x.float()).all()
    packed, scales = F.quantize_kv_mxfp4(x)
    assert packed.dtype == torch.uint8 and packed.shape == (x.shape[0], 16)
    assert scales.dtype == torch.uint8 and scales.shape == (x.shape[0], 1)
    want_codes, want_e = np_quantize(x.double().numpy())
    got = unpack(packed)
    bad = np.argwhere(got != want_codes)
    assert bad.size == 0, (bad[:5], got[tuple(bad[0])], want_codes[tuple(bad[0])])
    assert (scales.numpy() == want_e).all()
    # and what the named rows must give, written out
    assert got[0].tolist() == list(range(16)) * 2 and scales[0].item() == 127
    for i, k in enumerate((-9, -3, 0, 2, 7)):
        row = got[1 + i]
        assert row[0] == 6 and scales[1 + i].item() == 127 + k
        assert row[1:8].tolist() == TIE_CODES and row[8:15].tolist() == [8 + c for c in TIE_CODES]
    assert got[6][:10].tolist() == [6, 7, 7, 7, 7, 15, 15, 7, 7, 15]             # 6.5 and 5.5 -> 6 (code 7), 7.x saturate
    assert got[7].tolist() == [8, 0, 6, 14] * 8 and scales[7].item() == 125      # -0.0 stays -0.0 (amax 1: X = -2)
    assert (got[8] == 0).all() and scales[8].item() == 127                      # the all-zero block
    assert (got[9] == 0).all() and scales[9].item() == 127                      # amax = 0: all nibbles 0, signed zeros included
    fi = torch.finfo(dtype)
    emax = int(np.floor(np.log2(fi.max)))
    assert scales[10].item() == emax - 2 + 127 and got[10][:2].tolist() == [7, 15]          # the largest finite saturates to +-6
    sub = {torch.float16: -24, torch.bfloat16: -133}[dtype]
    assert scales[11].item() == max(sub + 1 - 2 + 127, 0)                        # amax = 3 * the smallest subnormal
    assert scales[12].item() == max(sub - 2 + 127, 0)
    if dtype == torch.float16:
        assert got[12][0] == 6 and got[11][:4].tolist() == [4, 12, 0, 7]         # 2^-24 / 2^-26 = 4; amax 3 * 2^-24: X = -25
    else:
        # e clamps to 0: 2^-133 / 2^-127 rounds to 0, and the negative element keeps its sign
        assert (got[12] == 0).all() and ((got[11] & 7) == 0).all() and got[11][:4].tolist() == [0, 8, 0, 0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_round_trip_is_exact_in_the_inputs_dtype_and_idempotent(dtype):
    F = _F()
    x = cases(dtype)
    packed, scales = F.quantize_kv_mxfp4(x)
    wide = F.dequantize_kv_mxfp4(packed, scales, torch.float64)
    ref = GRID[unpack(packed) & 7] * np.where(unpack(packed) & 8, -1.0, 1.0) * \
        np.repeat(np.ldexp(1.0, scales.numpy().astype(np.int64) - 127), 32, axis=-1)
    assert np.array_equal(wide.numpy(), ref)                                     # dequantize is nibble * 2^(e - 127)
    back = F.dequantize_kv_mxfp4(packed, scales, dtype)
    assert back.dtype == dtype
    assert torch.equal(back.double(), wide), "a dequantised value is not representable in the input's dtype"
    assert np.array_equal(np.signbit(back.double().numpy()), np.signbit(ref))    # -0.0 stays -0.0
    p2, s2 = F.quantize_kv_mxfp4(back)
    # (a block that rounded to all zeros is re-quantised as an all-zero block: e = 127, and its zeros lose their sign)
    zero = (back.double().abs().amax(-1) == 0)
    assert torch.equal(p2[~zero], packed[~zero]) and torch.equal(s2[~zero], scales[~zero])
    assert (p2[zero] == 0).all() and (s2[zero] == 127).all()
    p3, s3 = F.quantize_kv_mxfp4(F.dequantize_kv_mxfp4(p2, s2, dtype))
    assert torch.equal(p3, p2) and torch.equal(s3, s2)
    # the packed dtypes torch has for the format are views of the same bytes
    assert torch.equal(F.dequantize_kv_mxfp4(packed.view(torch.float4_e2m1fn_x2), scales.view(torch.float8_e8m0fnu), dtype).double(), wide)
    # a [B, H_kv, S, D] tensor keeps its leading dimensions
    y = x[:24].reshape(2, 3, 1, 128)
    p4, s4 = F.quantize_kv_mxfp4(y)
    assert p4.shape == (2, 3, 1, 64) and s4.shape == (2, 3, 1, 4)
    assert torch.equal(p4.reshape(24, 16), packed[:24]) and torch.equal(s4.reshape(24, 1), scales[:24])


# ---------------------------------------------------------------- the C boundary
def test_header_declares_and_the_library_exports_the_four_entry_points():
    fa = _lib()
    txt, body, names = vck.header_functions(HDR)
    assert names == NAMES
    assert '#include "mi355fa_kvcache.h"' in txt and '#include "mi355fa_paged.h"' in txt
    assert re.search(r"#define\s+MI355FA_KV_MXFP4\s+1\b", txt) and fa.KV_MXFP4 == 1
    assert "fa_debug" not in txt
    for older in ("mi355fa.h", "mi355fa_kvcache.h", "mi355fa_kvcache_fp8.h", "mi355fa_paged.h", "mi355fa_ragged.h", "mi355fa_sink.h"):
        assert "fp4" not in open(os.path.join(ROOT, "include", older)).read().lower(), older
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in fa.KVCACHE_FP4_SIGNATURES and name in fa.ALL_SIGNATURES, name
    # the prototypes carry one ctypes type per declared parameter
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, body)
        assert len(fa.KVCACHE_FP4_SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    assert fa.lib.fa_abi_version() == 7 and fa.ABI_VERSION == 7
    # the format is fixed in the header
    for phrase in ("e2m1", "e8m0", "low nibble", "2^(e - 127)", "floor(log2(amax)) - 2", "clamp(X + 127, 0, 254)", "nearest even",
                   "saturating", "-0.0 stays -0.0", "D / 32"):
        assert phrase in txt, phrase


def test_workspace_agrees_with_the_fp8_formula():
    fa = _lib()
    L = fa.lib
    shapes = ((1, 32, 8, 1, 4096, 128), (8, 32, 8, 1, 16384, 128), (8, 32, 8, 1, 16384, 64), (3, 4, 4, 130, 768, 64),
              (1, 8, 1, 1, 1 << 20, 64), (32, 32, 8, 1, 4096, 128))
    try:
        for n in (0, 1, 2, 7):
            vck.splits(n)
            for (B, H, Hkv, Sq, Sc, D) in shapes:
                for Sn in (0, 5):
                    # the fp8 functions' formula, n * B * H * S_q * (D + 2) * 4: at a forced count the same bytes, and at
                    # the rule's own count (n = 0) the same wherever the two rules agree, which is D = 64
                    got = L.fa_fwd_kvcache_fp4_workspace_bytes(B, H, Hkv, Sq, Sc, Sn, D)
                    assert got >= 0 and got % (B * H * Sq * (D + 2) * 4) == 0
                    if n or D == 64:
                        assert got == L.fa_fwd_kvcache_fp8_workspace_bytes(B, H, Hkv, Sq, Sc, Sn, D)
                    if n:
                        assert got == (0 if n == 1 else n * B * H * Sq * (D + 2) * 4)
                    for page in (32, 128):
                        assert L.fa_fwd_kvcache_fp4_paged_workspace_bytes(B, H, Hkv, Sq, Sc // page, page, Sn, D) == got
        vck.splits(0)
        # the path's own rule: at most 512 workgroups over (batch, K/V head, 32-row block, split) at both head dims,
        # n <= sqrt(S_cache / 64), at most 64 splits
        for (B, H, Hkv, Sq, Sc, D, n) in ((1, 32, 8, 1, 4096, 128, 8), (1, 32, 8, 1, 32768, 128, 22), (8, 32, 8, 1, 4096, 128, 8),
                                          (8, 32, 8, 1, 16384, 128, 8), (8, 32, 8, 1, 16384, 64, 8), (32, 32, 8, 1, 4096, 128, 2),
                                          (1, 4, 4, 1, 200, 64, 1), (1, 8, 1, 1, 1 << 20, 64, 64), (64, 32, 8, 1, 4096, 128, 1)):
            got = L.fa_fwd_kvcache_fp4_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D)
            assert got == (0 if n == 1 else n * B * H * Sq * (D + 2) * 4), (B, H, Hkv, Sq, Sc, D, got)
    finally:
        vck.splits(0)
    assert L.fa_fwd_kvcache_fp4_workspace_bytes(1, 4, 4, 1, 64, 0, 256) == SHAPE
    assert L.fa_fwd_kvcache_fp4_workspace_bytes(1, 4, 4, 1, 64, 0, 96) == SHAPE
    assert L.fa_fwd_kvcache_fp4_paged_workspace_bytes(1, 4, 4, 1, 4, 16, 0, 64) == fa.ERR_PAGED
    assert L.fa_fwd_kvcache_fp4_workspace_bytes(1, 6, 4, 1, 64, 0, 64) == fa.ERR_GROUP


def test_bad_arguments_are_refused_before_launch():
    fa = _lib()
    L = fa.lib
    _buf, p = vck.aligned_ptr()
    S3 = lambda *s: ctypes.cast((ctypes.c_longlong * 3)(*s), ctypes.POINTER(ctypes.c_longlong))
    B, H, Hkv, Sq, Sc = 2, 8, 2, 1, 1024
    vck.splits(1)                                                               # no workspace needed
    try:
        def padded(q=p, kc=p, vc=p, ks=p, vs=p, kss=None, vss=None, sinks=None, D=128, kvdt=fa.KV_MXFP4, dt=fa.BF16, opts=None):
            return L.fa_fwd_kvcache_fp4(q, kc, vc, ks, vs, None, None, p, kss, vss, sinks, p, None, None, 0, B, H, Hkv, Sq, Sc,
                                        0, D, dt, kvdt, 0.125, -1, -1, opts, None)

        def paged(kc=p, ks=p, vs=p, kss=None, sinks=None, D=128, kvdt=fa.KV_MXFP4, page=64, table=p):
            return L.fa_fwd_kvcache_fp4_paged(p, kc, p, ks, vs, None, None, p, table, kss, None, sinks, p, None, None, 0, B, H, Hkv,
                                              Sq, 40, page, 16, 16, 0, D, fa.BF16, kvdt, 0.125, -1, -1, None, None)

        err = lambda: L.fa_last_error().decode()
        for call, fn in ((padded, "fa_fwd_kvcache_fp4"), (paged, "fa_fwd_kvcache_fp4_paged")):
            for D in (256, 96, 32):
                assert call(D=D) == SHAPE, (fn, D)
                assert err() == "%s: an MXFP4 cache takes head dim 64 or 128" % fn
            for kvdt in (0, 2, -1):
                assert call(kvdt=kvdt) == DTYPE, (fn, kvdt)
                assert err() == "%s: kv_dtype must be MI355FA_KV_MXFP4" % fn
            assert call(kc=p + 8) == ALIGN and "16-byte aligned" in err()
            for D, off in ((128, 2), (128, 1), (64, 1)):                        # scales: aligned to their row of D / 32 bytes
                assert call(ks=p + off, D=D) == ALIGN, (fn, D, off)
                assert err() == "%s: k_scale / v_scale must be aligned to their row of D / 32 bytes" % fn
                assert call(vs=p + off, D=D) == ALIGN, (fn, D, off)
            assert call(ks=None) == NULL
            assert call(sinks=p + 2) == ALIGN and "sinks" in err()
            rows = Sc if call is padded else 64
            keep = S3(Hkv * rows * 4, rows * 4, 0)                              # a scale row stride below D / 32
            assert call(kss=keep) == STRIDE and err() == "%s: the scale row stride must be at least D / 32 bytes" % fn
            keep = S3(Hkv * rows * 4, rows * 4, 6)                              # ... and one that is no multiple of it
            assert call(kss=keep) == STRIDE and "multiples of D / 32" in err()
            keep = S3(Hkv * rows * 4 + 2, rows * 4, 4)
            assert call(kss=keep) == STRIDE
        # cache strides are bytes and multiples of 16, the row at least D / 2
        for bad in ((Hkv * Sc * 64, Sc * 64, 72), (Hkv * Sc * 64 + 8, Sc * 64, 64), (Hkv * Sc * 64, Sc * 64, 48)):
            keep = S3(*bad)
            st = fa.Opts.make(k_strides=keep, v_strides=keep)
            assert padded(opts=ctypes.byref(st)) == STRIDE, bad
            assert "MXFP4 cache" in err()
        for page in (16, 0, 48, -32):
            assert paged(page=page) == fa.ERR_PAGED, page
            assert err() == "fa_fwd_kvcache_fp4_paged: page_size must be a positive multiple of 32"
        assert paged(table=None) == NULL
        assert paged(table=p + 2) == ALIGN
    finally:
        vck.splits(0)


def test_python_surface_and_refusals():
    F = _F()
    import _mi355fa_fp4_torch as ext
    assert F.__all__ == ["quantize_kv_mxfp4", "dequantize_kv_mxfp4", "flash_attention_kvcache_fp4", "flash_attention_kvcache_fp4_paged"]
    assert str(inspect.signature(F.flash_attention_kvcache_fp4)) == (
        "(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, k_new=None, v_new=None, is_causal=False, "
        "window_size=(-1, -1), softmax_scale=None, return_lse=False, sinks=None)")
    assert str(inspect.signature(F.flash_attention_kvcache_fp4_paged)) == (
        "(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, block_table, k_new=None, v_new=None, is_causal=False, "
        "window_size=(-1, -1), softmax_scale=None, return_lse=False, sinks=None)")
    assert str(inspect.signature(F.quantize_kv_mxfp4)) == "(x)"
    assert str(inspect.signature(F.dequantize_kv_mxfp4)) == "(packed, scales, dtype)"
    assert hasattr(ext, "kvcache_fp4_forward")
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    q, sl = mk(2, 8, 1, 64), torch.zeros(2, dtype=torch.int32)
    kc, ks = u8(2, 2, 128, 32), u8(2, 2, 128, 2)
    sinks = torch.zeros(8)
    call = F.flash_attention_kvcache_fp4
    with pytest.raises(AssertionError, match="sinks must not require grad"):
        call(q, kc, kc, ks, ks, sl, sinks=sinks.clone().requires_grad_(True))
    with pytest.raises(AssertionError, match="q must not require grad"):
        call(q.clone().requires_grad_(True), kc, kc, ks, ks, sl)
    with pytest.raises(AssertionError, match="k_new must not require grad"):
        call(q, kc, kc, ks, ks, sl, k_new=mk(2, 2, 1, 64).requires_grad_(True), v_new=mk(2, 2, 1, 64))
    with pytest.raises(AssertionError, match="together"):
        call(q, kc, kc, ks, ks, sl, k_new=mk(2, 2, 1, 64))
    with pytest.raises(AssertionError, match="float4_e2m1fn_x2"):
        call(q, kc.to(torch.float16), kc.to(torch.float16), ks, ks, sl)
    with pytest.raises(AssertionError, match="float8_e8m0fnu"):
        call(q, kc, kc, ks.to(torch.int8), ks.to(torch.int8), sl)
    with pytest.raises(AssertionError, match="D = 64 or 128"):
        call(mk(2, 8, 1, 256), u8(2, 2, 128, 128), u8(2, 2, 128, 128), u8(2, 2, 128, 8), u8(2, 2, 128, 8), sl)
    with pytest.raises(AssertionError, match="window_right"):
        call(q, kc, kc, ks, ks, sl, is_causal=True, window_size=(-1, 2))
    with pytest.raises(AssertionError, match="device tensors"):
        call(q, kc, kc, ks, ks, sl)                                             # CPU tensors reach the binding and stop there
    with pytest.raises(AssertionError, match="D / 32"):
        ext.kvcache_fp4_forward(q, kc, kc, u8(2, 2, 128, 4), u8(2, 2, 128, 4), sl, None, None, None, -1, -1, 0.0, None)
    bt = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(AssertionError, match="device tensor"):
        F.flash_attention_kvcache_fp4_paged(q, kc, kc, ks, ks, sl, bt)
    with pytest.raises(AssertionError, match="int32"):
        F.flash_attention_kvcache_fp4_paged(q, kc, kc, ks, ks, sl, bt.long())
