"""CPU tests of the KV-cache decoding boundary: include/mi355fa_kvcache.h declares exactly two entry points and
MI355FA_ERR_WORKSPACE, libmi355fa.so and _mi355fa.SIGNATURES export them, every argument error is refused before anything
is launched, the workspace follows the documented formula -- at the split count of the rule recorded in
tests/golden/decode_splits.json, for the padded, fp8, paged and packed calls alike --, and the Python function refuses what
it must.  No compute is launched here (no GPU)."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "mi355fa_kvcache.h")


def _functions():
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fa_[a-z_]+)\s*\(", txt)))


def _lib():
    import _mi355fa as fa
    fa.lib.fa_debug_kvcache_splits.argtypes = [ctypes.c_int]
    fa.lib.fa_debug_kvcache_splits.restype = None
    return fa


def test_header_declares_the_kvcache_entry_points():
    assert _functions() == ["fa_fwd_kvcache", "fa_fwd_kvcache_workspace_bytes"]
    txt = open(HDR).read()
    assert '#include "mi355fa_gqa.h"' in txt
    assert re.search(r"#define\s+MI355FA_ERR_WORKSPACE\s+\(-9\)", txt)
    # the debug override stays out of the public header
    assert "fa_debug" not in txt
    assert "kvcache" not in open(os.path.join(ROOT, "include", "mi355fa.h")).read()


def test_library_and_ctypes_export_the_kvcache_entry_points():
    fa = _lib()
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in _functions() + ["fa_debug_kvcache_splits"]:
        assert hasattr(raw, name), name
    for name in _functions():
        assert name in fa.SIGNATURES, "python binding misses " + name
    assert len(fa.SIGNATURES["fa_fwd_kvcache"][1]) == 23
    assert fa.ERR_WORKSPACE == -9
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
        need = L.fa_fwd_kvcache_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D)
        assert need == 4 * B * H * Sq * (D + 2) * 4

        def call(q=p, kc=p, vc=p, kn=None, vn=None, sl=p, o=p, ws=p, wsb=need, B=B, H=H, Hkv=Hkv, Sq=Sq, Sc=Sc, Sn=0,
                 D=D, dt=fa.BF16, wl=-1, wr=-1, opts=None):
            return L.fa_fwd_kvcache(q, kc, vc, kn, vn, sl, o, None, ws, wsb, B, H, Hkv, Sq, Sc, Sn, D, dt, 0.125, wl, wr,
                                    opts, None)

        for kw in ({"q": None}, {"kc": None}, {"vc": None}, {"sl": None}, {"o": None}, {"kn": p}, {"Sn": 3}):
            assert call(**kw) == -1, kw                                   # MI355FA_ERR_NULL
        for kw in ({"B": 0}, {"H": 0}, {"Sq": 0}, {"Sc": 0}, {"Sn": 2, "kn": p, "vn": p, "B": -1}, {"Sn": -1}):
            assert call(**kw) == -2, kw                                   # MI355FA_ERR_SHAPE
        assert call(kn=p, vn=p, Sn=0) == -2                               # k_new with S_new = 0
        assert call(D=96) == -3                                           # MI355FA_ERR_HEAD_DIM
        assert call(dt=2) == -4                                           # MI355FA_ERR_DTYPE
        assert call(q=p + 8) == -5                                        # MI355FA_ERR_ALIGN
        for kw in ({"Hkv": 0}, {"Hkv": 3}, {"H": 6, "Hkv": 4}):
            assert call(**kw) == fa.ERR_GROUP, kw
        for kw in ({"wl": -2}, {"wr": -3}):
            assert call(**kw) == fa.ERR_WINDOW, kw
        assert call(wsb=need - 1) == fa.ERR_WORKSPACE
        assert b"workspace" in L.fa_last_error()
        assert call(ws=None) == fa.ERR_WORKSPACE
        cu = ctypes.c_int(0)
        for opts in (fa.Opts.make(cu_seqlens_q=ctypes.addressof(cu), cu_seqlens_k=ctypes.addressof(cu), total_q=1, total_k=1),
                     fa.Opts.make(p_drop=0.25, seed=1), fa.Opts.make(q_scaled=p)):
            assert call(opts=ctypes.byref(opts)) == -2
        bad = fa.Opts.make()
        bad.size = 4
        assert call(opts=ctypes.byref(bad)) == -2
        kst = (ctypes.c_longlong * 3)(Sc * Hkv * D, D, Hkv * D + 3)      # a row stride that is not a multiple of 8
        st = fa.Opts.make(k_strides=ctypes.cast(kst, ctypes.POINTER(ctypes.c_longlong)))
        assert call(opts=ctypes.byref(st)) == -6                          # MI355FA_ERR_STRIDE
        kst2 = (ctypes.c_longlong * 3)(Sc * Hkv * D, D, Hkv * D)          # K and V with different row strides
        st2 = fa.Opts.make(k_strides=ctypes.cast(kst2, ctypes.POINTER(ctypes.c_longlong)))
        assert call(opts=ctypes.byref(st2)) == -6
        assert b"sequence stride" in L.fa_last_error()
    finally:
        fa.lib.fa_debug_kvcache_splits(0)


def test_workspace_follows_the_documented_formula():
    fa = _lib()
    L = fa.lib
    try:
        for n in (1, 2, 7, 64):
            fa.lib.fa_debug_kvcache_splits(n)
            for (B, H, Hkv, Sq, Sc, D) in ((1, 32, 8, 1, 4096, 128), (3, 4, 4, 130, 777, 64), (8, 8, 1, 3, 64, 128)):
                want = 0 if n == 1 else n * B * H * Sq * (D + 2) * 4
                assert L.fa_fwd_kvcache_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D) == want
                assert L.fa_fwd_kvcache_workspace_bytes(B, H, Hkv, Sq, Sc, 5, D) == want
        fa.lib.fa_debug_kvcache_splits(0)
        # the formula: at most 256 workgroups over (batch, K/V head, 32-row block, split), n <= sqrt(S_cache / 128), at
        # most 64 splits
        for (B, H, Hkv, Sq, Sc, D, n) in ((1, 32, 8, 1, 131072, 128, 32), (8, 32, 8, 1, 16384, 128, 4),
                                          (32, 32, 8, 1, 4096, 128, 1), (8, 32, 8, 1, 1024, 128, 2),
                                          (1, 32, 8, 1, 4096, 128, 5), (1, 4, 4, 1, 200, 64, 1),
                                          (64, 32, 8, 1, 8192, 128, 1), (1, 8, 1, 1, 1 << 20, 64, 64),
                                          (1, 32, 8, 130, 65536, 128, 2)):
            got = L.fa_fwd_kvcache_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D)
            assert got == (0 if n == 1 else n * B * H * Sq * (D + 2) * 4), (B, H, Hkv, Sq, Sc, D, got)
        # shape errors come back as the (negative) error codes
        assert L.fa_fwd_kvcache_workspace_bytes(1, 6, 4, 1, 64, 0, 64) == fa.ERR_GROUP
        assert L.fa_fwd_kvcache_workspace_bytes(1, 4, 4, 1, 64, 0, 96) == -3
        assert L.fa_fwd_kvcache_workspace_bytes(1, 4, 4, 0, 64, 0, 64) == -2
    finally:
        fa.lib.fa_debug_kvcache_splits(0)


def test_python_surface():
    import My_FlashAttention_optimized as M
    import _mi355fa_torch as ext
    assert str(inspect.signature(M.flash_attention_kvcache)) == (
        "(q, k_cache, v_cache, cache_seqlens, k_new=None, v_new=None, is_causal=False, window_size=(-1, -1), "
        "softmax_scale=None, return_lse=False)")
    assert hasattr(ext, "kvcache_forward")
    doc = M.flash_attention_kvcache.__doc__
    for phrase in ("bottom-right", "L_b - S_q + i", "cache_seqlens", "no backward", "LSE = -inf"):
        assert phrase in doc, phrase


def test_python_refuses_cpu_tensors_grad_and_causal_with_a_right_window():
    import My_FlashAttention_optimized as M
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    q, kc, vc, sl = mk(2, 8, 1, 64), mk(2, 2, 128, 64), mk(2, 2, 128, 64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(AssertionError, match="device"):
        M.flash_attention_kvcache(q, kc, vc, sl)
    with pytest.raises(AssertionError, match="backward"):
        M.flash_attention_kvcache(q.clone().requires_grad_(True), kc, vc, sl)
    with pytest.raises(AssertionError, match="backward"):
        M.flash_attention_kvcache(q, kc, vc.clone().requires_grad_(True), sl)
    with pytest.raises(AssertionError, match="window_right"):
        M.flash_attention_kvcache(q, kc, vc, sl, is_causal=True, window_size=(-1, 2))
    with pytest.raises(AssertionError, match="window"):
        M.flash_attention_kvcache(q, kc, vc, sl, window_size=(-5, 0))


def test_cpp_binding_refuses_bad_arguments():
    """The C++ launcher's own checks (no device needed): each case stops at its own message."""
    import _mi355fa_torch as ext
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    sl = torch.zeros(2, dtype=torch.int32)
    q, kc = mk(2, 8, 1, 64), mk(2, 2, 128, 64)
    cases = [((q, kc, kc, sl), {}, "device tensors"),
             ((q, mk(2, 3, 128, 64), mk(2, 3, 128, 64), sl), {}, "multiple"),
             ((q, kc, mk(2, 2, 64, 64), sl), {}, "same shape"),
             ((mk(2, 8, 1, 128), kc, kc, sl), {}, "head dim"),
             ((q, kc, kc, sl), {"k_new": mk(2, 2, 1, 64)}, "together"),
             ((q, kc, kc, sl), {"window_left": -4}, ">= -1")]
    for args, kw, msg in cases:
        with pytest.raises(AssertionError, match=msg):
            ext.kvcache_forward(*args, **kw)


def test_split_rule_is_the_recorded_one():
    """The workspace is linear in the split count, so the bytes the four workspace functions return over the grid of
    tests/paged_surface.py pin the rule at every point (recorded before the three spellings of it became one)."""
    import paged_surface as ps
    with open(os.path.join(ps.GOLDEN, "decode_splits.json")) as fh:
        want = json.load(fh)
    got = ps.split_grid()
    assert got["grid"] == want["grid"] == ps.GRID and got["page_size"] == want["page_size"]
    names = ["padded", "padded_fp8", "paged_16bit", "paged_fp8", "ragged_16bit", "ragged_fp8"]
    assert sorted(want) == sorted(names + ["grid", "page_size"])
    for name in names:
        assert len(want[name]) == 5 * 2 * 3 * 4 * 5 * 2
        bad = [(i, g, w) for i, (g, w) in enumerate(zip(got[name], want[name])) if g != w]
        assert not bad, (name, bad[:5])
    # the grid reaches one split and the cap of 64, and the fp8 rule differs from the 16-bit one somewhere
    assert 0 in want["padded"] and want["padded"] != want["padded_fp8"] and want["ragged_16bit"] != want["ragged_fp8"]
