"""CPU tests of the soft-capped quantised-cache decoding boundary (include_quant/mi355fa_kvcache_quant_softcap.h;
quant_softcap_kvcache.py): the header declares exactly six entry points, three format constants and one struct, and the library
exports them with ctypes signatures of their own; the ABI version and every other header's function list are untouched; the
workspace functions return what the plain call of each format and geometry returns; every bad argument is refused before anything
is launched, by return code and fa_last_error() text, with two-fault cases for the order of the checks; the existing entry points
keep their own refusals of a cap over a quantised cache; the Python surface and refusals; the new kernels are in the library at the
expected count per (stem, D, format) and inside the decode kernels' budget.  No compute is launched (no GPU)."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

from conftest import ROOT
import variantcheck as vck

HDR = os.path.join(ROOT, "include_quant", "mi355fa_kvcache_quant_softcap.h")
NAMES = sorted(["fa_fwd_kvcache_quant_softcap", "fa_fwd_kvcache_quant_softcap_workspace_bytes", "fa_fwd_kvcache_quant_softcap_paged",
                "fa_fwd_kvcache_quant_softcap_paged_workspace_bytes", "fa_fwd_kvcache_quant_softcap_ragged",
                "fa_fwd_kvcache_quant_softcap_ragged_workspace_bytes"])
NULL, SHAPE, HEAD_DIM, DTYPE, ALIGN, STRIDE = -1, -2, -3, -4, -5, -6
E4M3, TOKEN, FP4 = 0, 1, 2
F8 = torch.float8_e4m3fn


def _lib():
    import _mi355fa as fa
    return fa


def _Q():
    import quant_softcap_kvcache as Q
    return Q


# ---------------------------------------------------------------- the C boundary
def test_header_library_and_ctypes_agree():
    fa = _lib()
    txt, body, functions = vck.header_functions(HDR)
    assert functions == NAMES
    for parent in ("mi355fa_softcap.h", "mi355fa_kvcache_fp8.h", "mi355fa_kvcache_fp8_token.h", "mi355fa_kvcache_fp4.h",
                   "mi355fa_ragged_fp4.h", "mi355fa_paged.h", "mi355fa_ragged.h"):
        assert '#include "../include/%s"' % parent in txt, parent
    for name, value in (("MI355FA_QUANT_E4M3", 0), ("MI355FA_QUANT_E4M3_TOKEN", 1), ("MI355FA_QUANT_MXFP4", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), body), name
    assert (fa.QUANT_E4M3, fa.QUANT_E4M3_TOKEN, fa.QUANT_MXFP4) == (0, 1, 2)
    m = re.search(r"typedef struct mi355fa_quant_cache \{(.*?)\} mi355fa_quant_cache;", body, re.S)
    members = re.findall(r"\*?\s*\**(\w+)\s*[,;]", m.group(1))
    assert members == [f[0] for f in fa.QuantCache._fields_], members
    assert body.count("typedef") == 1 and "fa_debug" not in txt and "sinks" not in body and "alibi" not in body
    for phrase in ("UNDER the tanh", "MI355FA_ERR_SOFTCAP", "MI355FA_ERR_SHAPE", "MI355FA_ERR_HEAD_DIM", "MI355FA_ERR_DTYPE",
                   "MI355FA_ERR_NULL", "The order of the checks", "before anything is enqueued", "at the same split count"):
        assert phrase in txt, phrase
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in fa.KVCACHE_QUANT_SOFTCAP_SIGNATURES and name in fa.ALL_SIGNATURES, name
        assert not any(name in t for t in (fa.KVCACHE_FP8_SIGNATURES, fa.KVCACHE_FP4_SIGNATURES, fa.RAGGED_FP4_SIGNATURES,
                                           fa.KVCACHE_FP8_TOKEN_SIGNATURES, fa.PAGED_SIGNATURES, fa.RAGGED_SIGNATURES,
                                           fa.SOFTCAP_SIGNATURES))
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, body)
        assert len(fa.KVCACHE_QUANT_SOFTCAP_SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    assert len(fa.KVCACHE_QUANT_SOFTCAP_SIGNATURES) == 6
    # fa_fwd_kvcache_softcap's order: softcap right behind scale; the struct in front of opts
    for name in NAMES:
        if not name.endswith("workspace_bytes"):
            args = re.search(r"\b%s\s*\(([^)]*)\)" % name, body).group(1)
            assert re.search(r"float scale,\s+float softcap,\s+int window_left", args), name
            assert re.search(r"const mi355fa_quant_cache\* cache,\s+const mi355fa_opts\* opts,\s+void\* stream$", args), name


def test_abi_and_every_other_function_list_are_unchanged():
    fa = _lib()
    assert fa.lib.fa_abi_version() == 7 and fa.ABI_VERSION == 7
    assert re.search(r"#define\s+MI355FA_ABI_VERSION\s+7\b", open(os.path.join(ROOT, "include", "mi355fa.h")).read())
    counts = {"mi355fa_kvcache.h": 2, "mi355fa_kvcache_fp8.h": 2, "mi355fa_kvcache_fp4.h": 4, "mi355fa_ragged_fp4.h": 2,
              "mi355fa_ragged.h": 2, "mi355fa_paged.h": 2, "mi355fa_softcap.h": 4, "mi355fa_alibi.h": 4, "mi355fa_sink.h": 4,
              "mi355fa_kvcache_fp8_token.h": 6}
    for name, n in counts.items():
        txt, _, functions = vck.header_functions(os.path.join(ROOT, "include", name))
        assert len(functions) == n, (name, functions)
        assert "quant_softcap" not in txt, name
    # include/ holds what it held (a recorded listing, tests/test_host_kvcache_fp8_token.py): the new header is the one file of a
    # directory of its own beside it
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(list(counts) + ["mi355fa.h", "mi355fa_local.h", "mi355fa_gqa.h"])
    assert os.listdir(os.path.join(ROOT, "include_quant")) == ["mi355fa_kvcache_quant_softcap.h"]


def test_workspace_is_the_plain_calls_of_each_format_and_geometry():
    fa = _lib()
    L = fa.lib
    W, WP, WR = (L.fa_fwd_kvcache_quant_softcap_workspace_bytes, L.fa_fwd_kvcache_quant_softcap_paged_workspace_bytes,
                 L.fa_fwd_kvcache_quant_softcap_ragged_workspace_bytes)
    plain = {E4M3: (L.fa_fwd_kvcache_fp8_workspace_bytes,
                    lambda *a: L.fa_fwd_kvcache_paged_workspace_bytes(*a, fa.PAGED_CACHE_FP8_E4M3),
                    lambda *a: L.fa_fwd_kvcache_ragged_workspace_bytes(*a, fa.PAGED_CACHE_FP8_E4M3)),
             TOKEN: (L.fa_fwd_kvcache_fp8_token_workspace_bytes, L.fa_fwd_kvcache_fp8_token_paged_workspace_bytes,
                     L.fa_fwd_kvcache_fp8_token_ragged_workspace_bytes),
             FP4: (L.fa_fwd_kvcache_fp4_workspace_bytes, L.fa_fwd_kvcache_fp4_paged_workspace_bytes,
                   L.fa_fwd_kvcache_fp4_ragged_workspace_bytes)}
    shapes = ((1, 32, 8, 1, 4096, 128), (8, 32, 8, 1, 16384, 128), (8, 32, 8, 1, 16384, 64), (3, 4, 4, 130, 768, 64),
              (1, 8, 1, 1, 1 << 20, 64), (32, 32, 8, 1, 4096, 128), (8, 16, 8, 1, 16384, 256), (3, 6, 2, 11, 704, 256))
    packed = ((8, 8, 32, 8, 128, 128, 128), (145, 32, 32, 8, 128, 128, 128), (1, 1, 4, 4, 1, 32, 64), (17, 300, 8, 1, 3, 32, 64),
              (8, 8, 16, 8, 128, 128, 256), (14, 6, 5, 1, 4, 96, 256))
    seen = set()
    try:
        for n in (0, 1, 2, 7):
            vck.splits(n)
            for fmt, (w, wp, wr) in plain.items():
                for (B, H, Hkv, Sq, Sc, D) in shapes:
                    if D == 256 and fmt != E4M3:
                        continue
                    for Sn in (0, 5):
                        got = W(fmt, B, H, Hkv, Sq, Sc, Sn, D)
                        assert got == w(B, H, Hkv, Sq, Sc, Sn, D) and got >= 0, (n, fmt, B, H, Hkv, Sq, Sc, D, got)
                        seen.add(got)
                        for page in (32, 128):
                            gp = WP(fmt, B, H, Hkv, Sq, Sc // page, page, Sn, D)
                            assert gp == wp(B, H, Hkv, Sq, Sc // page, page, Sn, D) and gp >= 0, (n, fmt, page)
                for (T, B, H, Hkv, MP, page, D) in packed:
                    got = WR(fmt, T, B, H, Hkv, MP, page, D)
                    assert got == wr(T, B, H, Hkv, MP, page, D) and got >= 32, (n, fmt, T, B, H, Hkv, MP, page, D, got)
    finally:
        vck.splits(0)
    assert len(seen) > 10
    err = lambda: L.fa_last_error().decode()
    for fmt in (TOKEN, FP4):                                                     # D = 256: the packed call only
        assert W(fmt, 1, 4, 4, 1, 64, 0, 256) == SHAPE and "with packed queries only" in err()
        assert WP(fmt, 8, 16, 8, 1, 128, 128, 0, 256) == SHAPE and WR(fmt, 8, 8, 16, 8, 128, 128, 256) > 0
    assert W(E4M3, 1, 4, 4, 1, 64, 0, 256) >= 0 and WP(E4M3, 8, 16, 8, 1, 128, 128, 0, 256) >= 0
    for fmt in (E4M3, TOKEN, FP4):
        for D in (96, 32, 512):
            assert W(fmt, 1, 4, 4, 1, 64, 0, D) == HEAD_DIM and WP(fmt, 1, 4, 4, 1, 4, 32, 0, D) == HEAD_DIM
            assert WR(fmt, 8, 8, 16, 8, 128, 128, D) == HEAD_DIM
        for page in (16, 0, 48):
            assert WP(fmt, 1, 4, 4, 1, 4, page, 0, 64) == fa.ERR_PAGED and WR(fmt, 8, 8, 16, 8, 128, page, 128) == fa.ERR_PAGED
        assert W(fmt, 1, 6, 4, 1, 64, 0, 64) == fa.ERR_GROUP
        assert WR(fmt, 0, 8, 16, 8, 128, 128, 128) == fa.ERR_RAGGED and WR(fmt, 8, 0, 16, 8, 128, 128, 128) == fa.ERR_RAGGED
    for bad in (-1, 3, 99):
        assert W(bad, 1, 4, 4, 1, 64, 0, 64) == DTYPE and err().endswith("(got %d)" % bad)
        assert WP(bad, 1, 4, 4, 1, 4, 32, 0, 64) == DTYPE and WR(bad, 8, 8, 16, 8, 128, 128, 128) == DTYPE
        assert W(bad, 1, 4, 4, 1, 64, 0, 96) == DTYPE                            # two faults: the format first


def test_bad_arguments_are_refused_before_launch():
    fa = _lib()
    L = fa.lib
    _buf, p = vck.aligned_ptr()
    S3 = lambda *s: ctypes.cast((ctypes.c_longlong * 3)(*s), ctypes.POINTER(ctypes.c_longlong))
    B, H, Hkv, Sq, Sc = 2, 8, 2, 1, 1024
    err = lambda: L.fa_last_error().decode()
    keep = []

    def cache(fmt, **kw):
        c = fa.QuantCache(format=fmt)
        if fmt != E4M3:
            c.k_scale = c.v_scale = p
        for k, v in kw.items():
            setattr(c, k, v)
        keep.append(c)
        return ctypes.byref(c)

    def padded(fmt=E4M3, c=0, q=p, kc=p, kn=None, vn=None, Sn=0, D=128, dt=fa.BF16, opts=None, ws=p, wsb=1 << 24, cap=30.0, scale=0.125,
               page=None, table=None, cu=None, T=None, wl=-1, **ckw):
        return L.fa_fwd_kvcache_quant_softcap(q, kc, p, kn, vn, p, p, None, ws, wsb, B, H, Hkv, Sq, Sc, Sn, D, dt, scale, cap, wl, -1,
                                              cache(fmt, **ckw) if c == 0 else c, opts, None)

    def paged(fmt=E4M3, c=0, q=p, kc=p, kn=None, vn=None, Sn=0, D=128, dt=fa.BF16, opts=None, ws=p, wsb=1 << 24, cap=30.0, scale=0.125,
              page=64, table=p, cu=None, T=None, wl=-1, **ckw):
        return L.fa_fwd_kvcache_quant_softcap_paged(q, kc, p, kn, vn, p, table, p, None, ws, wsb, B, H, Hkv, Sq, 40, page, 16, 16, Sn, D,
                                                    dt, scale, cap, wl, -1, cache(fmt, **ckw) if c == 0 else c, opts, None)

    def packed(fmt=E4M3, c=0, q=p, kc=p, kn=None, vn=None, Sn=0, D=128, dt=fa.BF16, opts=None, ws=p, wsb=1 << 24, cap=30.0, scale=0.125,
               page=64, table=p, cu=p, T=11, wl=-1, **ckw):
        return L.fa_fwd_kvcache_quant_softcap_ragged(q, kc, p, kn, vn, cu, p, table, p, None, ws, wsb, T, B, H, Hkv, 40, page, 16, 16, D,
                                                     dt, scale, cap, wl, -1, cache(fmt, **ckw) if c == 0 else c, opts, None)

    for n in (1, 4):
        vck.splits(n)
        try:
            for call, fn in ((padded, "fa_fwd_kvcache_quant_softcap"), (paged, "fa_fwd_kvcache_quant_softcap_paged"),
                             (packed, "fa_fwd_kvcache_quant_softcap_ragged")):
                rows = Sc if call is padded else 64
                # ---- this header's own refusals
                assert call(c=None) == NULL and err().startswith(fn + ": the mi355fa_quant_cache struct is NULL")
                for bad in (-1, 3, 7):
                    assert call(fmt=bad) == DTYPE and err().startswith(fn + ": format must be MI355FA_QUANT_E4M3 (0)") and err().endswith("(got %d)" % bad)
                for member in ("k_scale", "v_scale"):
                    assert call(E4M3, **{member: p}) == SHAPE and err().startswith(fn + ": k_scale / v_scale and their strides belong to")
                assert call(E4M3, k_scale_strides=S3(1, 1, 1)) == SHAPE
                for fmt in (TOKEN, FP4):
                    assert call(fmt, k_descale=p) == SHAPE and err() == fn + ": k_descale / v_descale / descale_bstride belong to MI355FA_QUANT_E4M3 (format %d)" % fmt
                    assert call(fmt, v_descale=p) == SHAPE and call(fmt, descale_bstride=Hkv) == SHAPE
                    assert call(fmt, k_scale=None) == NULL and err() == fn + ": format %d needs k_scale and v_scale" % fmt
                    assert call(fmt, v_scale=None) == NULL
                    if call is packed:
                        assert call(fmt, D=256, ws=None) == fa.ERR_WORKSPACE        # D = 256 passes every check up to the workspace
                    else:
                        assert call(fmt, D=256) == SHAPE and "takes head dim 256 with packed queries only (fa_fwd_kvcache_quant_softcap_ragged)" in err()
                if n > 1 or call is packed:                                          # (one split of a rectangular call needs no workspace)
                    assert call(E4M3, D=256, ws=None) == fa.ERR_WORKSPACE           # per-tensor e4m3: D = 256 in every geometry
                for fmt in (E4M3, TOKEN, FP4):
                    for D in (96, 32, 512):
                        assert call(fmt, D=D) == HEAD_DIM and err().startswith(fn + ": head dim"), (fn, fmt, D)
                    for cap in (0.0, -1.0, -0.0, float("inf"), float("nan")):
                        assert call(fmt, cap=cap) == fa.ERR_SOFTCAP and err() == fn + ": softcap must be finite and > 0", (fn, fmt, cap)
                    # ---- the parents' checks, by the shared code and with its texts
                    assert call(fmt, q=None) == NULL and err() == fn + ": NULL pointer"
                    assert call(fmt, kc=p + 8) == ALIGN and "16-byte aligned" in err()
                    assert call(fmt, kn=p) == NULL and "k_new and v_new" in err()
                    assert call(fmt, dt=2) == DTYPE
                    assert call(fmt, scale=0.0) < 0 and call(fmt, wl=-2) == fa.ERR_WINDOW
                    if call is not packed:
                        assert call(fmt, Sn=2) == NULL and err() == fn + ": S_new > 0 needs k_new and v_new"
                        assert call(fmt, kn=p, vn=p, Sn=0) == SHAPE
                    if call is not padded:
                        for page in (48, 16, 0):
                            assert call(fmt, page=page) == fa.ERR_PAGED and err() == fn + ": page_size must be a positive multiple of 32"
                        assert call(fmt, table=None) == NULL and "block_table" in err()
                        assert call(fmt, table=p + 2) == ALIGN
                    if call is packed:
                        assert call(fmt, cu=None) == NULL and "cu_seqlens_q" in err()
                        assert call(fmt, T=0) == fa.ERR_RAGGED and call(fmt, cu=p + 2) == ALIGN
                    if n > 1:   # every check passed: the workspace is the last
                        assert call(fmt, ws=None) == fa.ERR_WORKSPACE and call(fmt, wsb=16) == fa.ERR_WORKSPACE
                # the format's own members, as its own header refuses them
                bad16 = S3(Hkv * rows * 128, rows * 128, 136)                        # a cache row stride off 16 bytes
                for fmt, text in ((E4M3, "fp8 cache strides"), (TOKEN, "fp8 cache strides"), (FP4, "MXFP4 cache strides")):
                    assert call(fmt, opts=ctypes.byref(fa.Opts.make(k_strides=bad16, v_strides=bad16))) == STRIDE and text in err()
                assert call(E4M3, k_descale=p + 2) == ALIGN and "k_descale / v_descale must be 4-byte aligned" in err()
                assert call(E4M3, k_descale=p, descale_bstride=1) == SHAPE and "descale_bstride" in err()
                assert call(TOKEN, k_scale=p + 2) == ALIGN and err().startswith(fn + ": k_scale / v_scale must be 4-byte aligned")
                assert call(TOKEN, k_scale_strides=S3(Hkv * rows, rows, -1)) == STRIDE and err() == fn + ": the scale strides must be non-negative element strides (got -1)"
                assert call(FP4, k_scale=p + 2) == ALIGN and "aligned to their row of D / 32 bytes" in err()
                assert call(FP4, k_scale_strides=S3(Hkv * rows * 4, rows * 4, 2)) == STRIDE and "D / 32 bytes" in err()
                # ---- two faults at once: the order of the checks
                assert call(fmt=9, cap=0.0, q=None) == DTYPE                          # the format before everything
                assert call(TOKEN, k_descale=p, k_scale=None) == SHAPE               # a foreign member before a missing one
                assert call(FP4, k_scale=None, D=256) == NULL                        # missing scales before the head dim
                if call is not packed:
                    assert call(TOKEN, D=256, cap=0.0) == SHAPE                      # D = 256 before the cap
                assert call(E4M3, cap=0.0, q=None) == fa.ERR_SOFTCAP                 # the cap before the shared checks
                assert call(E4M3, cap=0.0, D=96) == fa.ERR_SOFTCAP
                assert call(E4M3, q=None, D=96) == NULL                              # then the parents' order: pointers, shape
                if call is not padded:
                    assert call(E4M3, cap=0.0, page=48) == fa.ERR_SOFTCAP            # the cap before the table
                    assert call(E4M3, page=48, q=None) == fa.ERR_PAGED               # the table before the shared checks
                if call is packed:
                    assert call(E4M3, cu=None, cap=0.0) == NULL and "cu_seqlens_q" in err()    # packed: cu_seqlens_q before the cap
                    assert call(fmt=9, cu=None) == DTYPE                             # and the struct before that
        finally:
            vck.splits(0)


def test_existing_entry_points_keep_their_refusals_of_a_cap_over_a_quantised_cache():
    """no existing call relies on launch_decode's refusal: the paged and packed 16-bit / e4m3 calls refuse in fa_api.hip, the
    MXFP4 and per-token calls have no softcap argument at all"""
    fa = _lib()
    L = fa.lib
    _buf, p = vck.aligned_ptr()
    mods = fa.PagedMods(softcap=30.0)
    err = lambda: L.fa_last_error().decode()
    rc = L.fa_fwd_kvcache_paged(p, p, p, None, None, p, p, p, None, p, 1 << 24, 2, 8, 2, 1, 40, 64, 16, 16, 0, 128, fa.BF16,
                                fa.PAGED_CACHE_FP8_E4M3, 0.125, -1, -1, ctypes.byref(mods), None, None)
    assert rc == fa.ERR_PAGED and "an fp8 cache takes sinks only" in err()
    rc = L.fa_fwd_kvcache_ragged(p, p, p, None, None, p, p, p, p, None, p, 1 << 24, 11, 2, 8, 2, 40, 64, 16, 16, 128, fa.BF16,
                                 fa.PAGED_CACHE_FP8_E4M3, 0.125, -1, -1, ctypes.byref(mods), None, None)
    assert rc == fa.ERR_PAGED and "an fp8 cache takes sinks only" in err()
    for table in (fa.KVCACHE_FP4_SIGNATURES, fa.RAGGED_FP4_SIGNATURES, fa.KVCACHE_FP8_TOKEN_SIGNATURES, fa.KVCACHE_FP8_SIGNATURES):
        for name, (_, args) in table.items():
            if not name.endswith("workspace_bytes"):
                assert args.count(ctypes.c_float) == 1, name                         # scale alone: no softcap
    import fp4_kvcache, fp4_ragged_kvcache, fp8_token_kvcache, paged_kvcache
    for f in (fp4_kvcache.flash_attention_kvcache_fp4, fp4_kvcache.flash_attention_kvcache_fp4_paged,
              fp4_ragged_kvcache.flash_attention_kvcache_fp4_ragged, fp8_token_kvcache.flash_attention_kvcache_fp8_token,
              fp8_token_kvcache.flash_attention_kvcache_fp8_token_paged, fp8_token_kvcache.flash_attention_kvcache_fp8_token_ragged):
        assert "softcap" not in inspect.signature(f).parameters, f.__name__
    q, sl, bt = torch.zeros(2, 8, 1, 64, dtype=torch.float16), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)
    pool = torch.zeros(8, 2, 64, 64, dtype=torch.uint8).view(F8)
    with pytest.raises(AssertionError, match="sinks only"):
        paged_kvcache.flash_attention_kvcache_paged(q, pool, pool, sl, bt, softcap=30.0)


# ---------------------------------------------------------------- the Python surface
def test_python_surface_and_refusals():
    Q = _Q()
    import _mi355fa_quant_softcap_torch as ext
    assert Q.__all__ == ["flash_attention_kvcache_quant_softcap", "flash_attention_kvcache_quant_softcap_paged",
                         "flash_attention_kvcache_quant_softcap_ragged"]
    sig = lambda f: str(inspect.signature(f))
    tail = ("k_scale=None, v_scale=None, k_descale=None, v_descale=None, k_new=None, v_new=None, is_causal=False, "
            "window_size=(-1, -1), softmax_scale=None, return_lse=False")
    assert sig(Q.flash_attention_kvcache_quant_softcap) == "(q, k_cache, v_cache, cache_seqlens, softcap, %s)" % tail
    assert sig(Q.flash_attention_kvcache_quant_softcap_paged) == "(q, k_cache, v_cache, cache_seqlens, block_table, softcap, %s)" % tail
    assert sig(Q.flash_attention_kvcache_quant_softcap_ragged) == (
        "(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, softcap, %s, out=None)" % tail)
    assert hasattr(ext, "kvcache_quant_softcap_forward") and hasattr(ext, "kvcache_quant_softcap_ragged_forward")
    # the recorded surfaces of the other modules are as they were
    import fp4_kvcache, fp4_ragged_kvcache, fp8_token_kvcache, paged_kvcache, ragged_kvcache
    assert fp4_kvcache.__all__ == ["quantize_kv_mxfp4", "dequantize_kv_mxfp4", "flash_attention_kvcache_fp4", "flash_attention_kvcache_fp4_paged"]
    assert fp4_ragged_kvcache.__all__ == ["flash_attention_kvcache_fp4_ragged"] and ragged_kvcache.__all__ == ["flash_attention_kvcache_ragged"]
    assert paged_kvcache.__all__ == ["flash_attention_kvcache_paged"] and len(fp8_token_kvcache.__all__) == 5
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    c8 = lambda *s: torch.zeros(*s, dtype=torch.uint8).view(F8)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    q, sl = mk(2, 8, 1, 64), torch.zeros(2, dtype=torch.int32)
    kc, ks = c8(2, 2, 128, 64), torch.ones(2, 2, 128)
    k4, s4 = u8(2, 2, 128, 32), u8(2, 2, 128, 2)
    kd = torch.ones(2, 2)
    call = Q.flash_attention_kvcache_quant_softcap
    # the three formats reach the binding, which stops at the CPU tensors
    for args, kw in (((q, kc, kc, sl, 30.0), {}), ((q, kc, kc, sl, 30.0), dict(k_descale=kd, v_descale=kd)),
                     ((q, kc, kc, sl, 30.0), dict(k_scale=ks, v_scale=ks)), ((q, k4, k4, sl, 30.0), dict(k_scale=s4, v_scale=s4))):
        with pytest.raises(AssertionError, match="device tensors"):
            call(*args, **kw)
    # anything else: the message names the three
    for kcx, kw in ((mk(2, 2, 128, 64), {}), (kc.view(torch.uint8), {}), (kc, dict(k_scale=s4[..., 0], v_scale=s4[..., 0])),
                    (k4, dict(k_scale=ks, v_scale=ks)), (kc, dict(k_scale=ks.half(), v_scale=ks.half())), (k4, {})):
        with pytest.raises(AssertionError, match="one of three.*per-tensor e4m3.*per-token e4m3.*MXFP4"):
            call(q, kcx, kcx, sl, 30.0, **kw)
    with pytest.raises(AssertionError, match="not both"):
        call(q, kc, kc, sl, 30.0, k_scale=ks, v_scale=ks, k_descale=kd)
    with pytest.raises(AssertionError, match="not both"):
        call(q, k4, k4, sl, 30.0, k_scale=s4, v_scale=s4, v_descale=kd)
    with pytest.raises(AssertionError, match="k_scale and v_scale must be given together"):
        call(q, kc, kc, sl, 30.0, k_scale=ks)
    for cap in (0.0, -3.0, float("inf"), float("nan")):
        with pytest.raises(AssertionError, match="softcap must be finite and > 0"):
            call(q, kc, kc, sl, cap)
    with pytest.raises(AssertionError, match="softcap must be a number"):
        call(q, kc, kc, sl, None)
    with pytest.raises(TypeError):
        call(q, kc, kc, sl)                                                     # the cap is required
    with pytest.raises(TypeError):
        call(q, kc, kc, sl, 30.0, sinks=torch.zeros(8))                         # at most one transform: no sinks here
    for name, kw in (("q", dict(q=q.clone().requires_grad_(True))), ("k_scale", dict(k_scale=ks.clone().requires_grad_(True), v_scale=ks)),
                     ("k_descale", dict(k_descale=kd.clone().requires_grad_(True))),
                     ("k_new", dict(k_new=mk(2, 2, 1, 64).requires_grad_(True), v_new=mk(2, 2, 1, 64)))):
        with pytest.raises(AssertionError, match=name + " must not require grad"):
            call(kw.pop("q", q), kc, kc, sl, 30.0, **kw)
    with pytest.raises(AssertionError, match="together"):
        call(q, kc, kc, sl, 30.0, k_new=mk(2, 2, 1, 64))
    with pytest.raises(AssertionError, match="the caches' shape without D"):
        call(q, kc, kc, sl, 30.0, k_scale=ks[:, :, :64], v_scale=ks)
    with pytest.raises(AssertionError, match="64 or 128"):
        call(mk(2, 8, 1, 256), c8(2, 2, 128, 256), c8(2, 2, 128, 256), sl, 30.0, k_scale=ks, v_scale=ks)
    with pytest.raises(AssertionError, match="64 or 128"):
        call(mk(2, 8, 1, 256), u8(2, 2, 128, 128), u8(2, 2, 128, 128), sl, 30.0, k_scale=u8(2, 2, 128, 8), v_scale=u8(2, 2, 128, 8))
    with pytest.raises(AssertionError, match="device tensors"):                  # per-tensor e4m3 takes D = 256
        call(mk(2, 8, 1, 256), c8(2, 2, 128, 256), c8(2, 2, 128, 256), sl, 30.0)
    with pytest.raises(AssertionError, match="64 or 128 or 256"):
        call(mk(2, 8, 1, 96), c8(2, 2, 128, 96), c8(2, 2, 128, 96), sl, 30.0)
    with pytest.raises(AssertionError, match="window_right"):
        call(q, kc, kc, sl, 30.0, is_causal=True, window_size=(-1, 2))
    with pytest.raises(AssertionError, match="softmax_scale must be finite"):
        call(q, kc, kc, sl, 30.0, softmax_scale=0.0)
    with pytest.raises(AssertionError, match="a per-token e4m3 or an MXFP4 cache takes head dim 64 or 128"):
        ext.kvcache_quant_softcap_forward(mk(2, 8, 1, 256), c8(2, 2, 128, 256), c8(2, 2, 128, 256), sl, None, 30.0, 1, ks, ks, None, None,
                                          None, None, -1, -1, 0.0)
    with pytest.raises(AssertionError, match="softcap must be finite"):
        ext.kvcache_quant_softcap_forward(q, kc, kc, sl, None, 0.0, 0, None, None, None, None, None, None, -1, -1, 0.0)
    with pytest.raises(AssertionError, match="belong to a per-tensor e4m3 cache"):
        ext.kvcache_quant_softcap_forward(q, kc, kc, sl, None, 30.0, 1, ks, ks, kd, None, None, None, -1, -1, 0.0)
    bt = torch.zeros(2, 4, dtype=torch.int32)
    pg = Q.flash_attention_kvcache_quant_softcap_paged
    with pytest.raises(AssertionError, match="device tensor"):
        pg(q, kc, kc, sl, bt, 30.0)
    with pytest.raises(AssertionError, match="int32"):
        pg(q, kc, kc, sl, bt.long(), 30.0)
    with pytest.raises(AssertionError, match="multiple of 32"):
        pg(q, c8(8, 2, 48, 64), c8(8, 2, 48, 64), sl, bt, 30.0)
    rg_ = Q.flash_attention_kvcache_quant_softcap_ragged
    qp, cu = mk(5, 8, 64), torch.tensor([0, 2, 5], dtype=torch.int32)
    kp, ksp = c8(8, 2, 64, 64), torch.ones(8, 2, 64)
    with pytest.raises(AssertionError, match="cu_seqlens_q must be a device tensor"):
        rg_(qp, kp, kp, cu, sl, bt, 30.0, k_scale=ksp, v_scale=ksp)
    with pytest.raises(AssertionError, match="cu_seqlens_q must be a device tensor"):    # D = 256 passes the wrapper's checks, every format
        rg_(mk(5, 8, 256), c8(8, 2, 64, 256), c8(8, 2, 64, 256), cu, sl, bt, 30.0, k_scale=ksp, v_scale=ksp)
    with pytest.raises(AssertionError, match="cu_seqlens_q must be a device tensor"):
        rg_(mk(5, 8, 256), u8(8, 2, 64, 128), u8(8, 2, 64, 128), cu, sl, bt, 30.0, k_scale=u8(8, 2, 64, 8), v_scale=u8(8, 2, 64, 8))
    with pytest.raises(AssertionError, match="64 or 128 or 256"):
        rg_(mk(5, 8, 96), c8(8, 2, 64, 96), c8(8, 2, 64, 96), cu, sl, bt, 30.0, k_scale=ksp, v_scale=ksp)
    with pytest.raises(AssertionError, match="multiple of 32"):
        rg_(qp, c8(8, 2, 48, 64), c8(8, 2, 48, 64), cu, sl, bt, 30.0)
    with pytest.raises(AssertionError, match="out must have q's dtype"):
        rg_(qp, kp, kp, cu, sl, bt, 30.0, out=torch.zeros(5, 8, 64, dtype=torch.bfloat16))
    with pytest.raises(AssertionError, match="one of three"):
        rg_(qp, kp.view(torch.uint8), kp.view(torch.uint8), cu, sl, bt, 30.0)
    with pytest.raises(AssertionError, match="device tensors"):
        ext.kvcache_quant_softcap_ragged_forward(qp, kp, kp, cu, sl, bt, 30.0, 0, None, None, None, None, None, None, -1, -1, 0.0, None)


# ---------------------------------------------------------------- the kernels
def test_new_kernels_are_in_the_library_inside_the_decode_budget():
    """<T, D, F, SOFTCAP = true> overloads of the three decode kernel names, F the cache format (fa::KvFormat 1 = kE4M3, 2 = kMXFP4,
    3 = kE4M3Token), two dtypes: kE4M3 at D = 64, 128, 256 in every geometry, the other two at D = 64, 128 and the packed kernel also
    at 256 -- workgroup 256, VGPR + AGPR <= 256, no scratch, no spills, LDS within 80 KiB.  No other kernel stem is new."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj
    found = {}
    for k in codeobj.kernels():
        m = re.match(r"_ZN2fa\d+(fa_decode_(?:mod|paged|ragged)_kernel)INS_\d+(BF16|FP16)ELi(\d+)ELNS_8KvFormatE(\d)ELb1EEE", k["name"])
        if m:
            key = (m.group(1), int(m.group(3)), int(m.group(4)))
            found[key] = found.get(key, 0) + 1
            assert k["wg"] == 256 and k["vgpr"] + k["agpr"] <= 256, (k["name"], k["vgpr"], k["agpr"])
            assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 81920, k["name"]
        assert not re.search(r"KvFormatE\dELb0E", k["name"]), k["name"]
    want = {}
    for stem in ("fa_decode_mod_kernel", "fa_decode_paged_kernel", "fa_decode_ragged_kernel"):
        for fmt in (1, 2, 3):
            for D in (64, 128, 256):
                if D != 256 or fmt == 1 or stem == "fa_decode_ragged_kernel":
                    want[stem, D, fmt] = 2
    assert found == want and sum(found.values()) == 46, found
