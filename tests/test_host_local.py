"""CPU tests of the sliding-window (local) attention boundary: include/mi355fa_local.h declares exactly three entry
points, libmi355fa.so exports them, bad arguments are refused before anything is launched, and the Python surface
(signature, FLOP count) is as documented.  No compute is launched here (no GPU)."""
import ctypes
import inspect
import os
import re

import torch

from conftest import ROOT


def _local_header_functions():
    txt = open(os.path.join(ROOT, "include", "mi355fa_local.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fa_[a-z_]+)\s*\(", txt)))


def test_companion_header_declares_the_three_local_entry_points():
    assert _local_header_functions() == ["fa_bwd_dkv_local", "fa_bwd_dq_local", "fa_fwd_local"]
    txt = open(os.path.join(ROOT, "include", "mi355fa_local.h")).read()
    assert '#include "mi355fa.h"' in txt
    assert re.search(r"#define\s+MI355FA_ERR_WINDOW\s+\(-7\)", txt)


def test_library_exports_the_local_entry_points():
    import _mi355fa as fa
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in _local_header_functions():
        assert hasattr(raw, name), name
        assert name in fa.SIGNATURES, "python binding misses " + name
    assert fa.ERR_WINDOW == -7
    assert fa.lib.fa_abi_version() == 7


def _ptr():
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_bad_arguments_are_refused_before_launch():
    import _mi355fa as fa
    L = fa.lib
    _buf, p = _ptr()
    shape = (1, 2, 8, 8)                      # B, H, S_q, S_k
    fwd = lambda D, wl, wr, opts=None, q=p: L.fa_fwd_local(q, p, p, p, p, *shape, D, fa.BF16, 0.125, wl, wr, opts, None)
    dq = lambda D, wl, wr, opts=None, q=p: L.fa_bwd_dq_local(q, p, p, p, p, p, p, p, *shape, D, fa.FP16, 0.125, wl, wr, opts, None)
    dkv = lambda D, wl, wr, opts=None, q=p: L.fa_bwd_dkv_local(q, p, p, p, p, p, p, p, *shape, D, fa.FP16, 0.125, wl, wr, opts, None)
    for fn in (fwd, dq, dkv):
        assert fn(64, -2, 0) == fa.ERR_WINDOW
        assert b"window" in L.fa_last_error()
        assert fn(64, 3, -5) == fa.ERR_WINDOW
        assert fn(96, 4, 0) == -3                                        # MI355FA_ERR_HEAD_DIM
        assert fn(64, 4, 0, q=None) == -1                                # MI355FA_ERR_NULL
        drop = fa.Opts.make(p_drop=0.25, seed=1)
        assert fn(64, 4, 0, opts=ctypes.byref(drop)) == -2               # dropout with a window: MI355FA_ERR_SHAPE
        assert b"dropout" in L.fa_last_error() and b"window" in L.fa_last_error()
        bad = fa.Opts.make()
        bad.size = 4
        assert fn(64, 4, 0, opts=ctypes.byref(bad)) == -2                # options as for fa_*_ex


def _brute_pairs(Sq, Sk, wl, wr):
    i = torch.arange(Sq)[:, None]
    j = torch.arange(Sk)[None, :]
    vis = torch.ones(Sq, Sk, dtype=torch.bool)
    if wr >= 0:
        vis &= j <= i + wr
    if wl >= 0:
        vis &= j >= i - wl
    return int(vis.sum())


def test_local_attention_flops_counts_the_visible_pairs():
    import My_FlashAttention_optimized as M
    shapes = [(1, 1), (7, 7), (77, 77), (64, 200), (333, 129), (129, 700), (5, 40)]
    windows = [(0, 0), (1, 0), (63, 0), (-1, 0), (-1, -1), (300, -1), (-1, 17), (0, 300), (127, 129), (2, 3)]
    for Sq, Sk in shapes:
        for wl, wr in windows:
            n = _brute_pairs(Sq, Sk, wl, wr)
            assert M.local_attention_visible_pairs(Sq, Sk, wl, wr) == n, (Sq, Sk, wl, wr)
            assert M.local_attention_flops(2, 3, Sq, Sk, 64, wl, wr, "fwd") == 4 * 64 * 2 * 3 * n
            assert M.local_attention_flops(2, 3, Sq, Sk, 128, wl, wr, "fwd_bwd") == 3.5 * 4 * 128 * 2 * 3 * n
    # rows with no visible key: S_k < S_q under a causal band shifted right, and a window entirely past S_k
    assert _brute_pairs(300, 10, 0, 0) == 10 and M.local_attention_visible_pairs(300, 10, 0, 0) == 10
    assert M.local_attention_visible_pairs(300, 10, 2, -1) == _brute_pairs(300, 10, 2, -1)
    # (-1, 0) is causal, (-1, -1) full attention
    assert M.local_attention_visible_pairs(256, 256, -1, 0) == 256 * 257 // 2
    assert M.local_attention_visible_pairs(100, 300, -1, -1) == 100 * 300


def test_python_surface():
    import My_FlashAttention_optimized as M
    import _mi355fa_torch as ext
    assert str(inspect.signature(M.flash_attention_local)) == "(Q, K, V, window_left, window_right=0)"
    assert list(inspect.signature(M.local_attention_flops).parameters) == \
        ["B", "H", "S_q", "S_k", "D", "window_left", "window_right", "mode"]
    assert hasattr(M, "FlashAttentionLocalFunction")
    for name in ("flash_attention_local", "local_forward_launch", "local_backward_launch"):
        assert hasattr(ext, name), name
