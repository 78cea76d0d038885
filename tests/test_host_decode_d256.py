"""CPU tests of head dim 256 on the decode path: every workspace function of the decode family takes D = 256 and returns
the partial layout's size, n * B * H * S_q * (256 + 2) * 4 bytes; other head dims (96, 192, 512) are still refused with
MI355FA_ERR_HEAD_DIM; the training side (fa_supported, fa_fwd) still refuses 256; libmi355fa.so holds D = 256 instances of the
three decode stems and the two combine kernels inside the budget every decode kernel is held to (workgroup 256, at most 256
registers, no scratch, no spill, at most 80 KiB of declared LDS); the ABI version and the headers' function lists are what
they were.  No compute is launched here (no GPU)."""
import os
import re
import sys

import pytest

from conftest import ROOT
import raggedcheck as rgc
import variantcheck as vck

sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

B, H, HKV, SQ, SC = 3, 8, 2, 2, 4096
HEAD_DIM = -3   # MI355FA_ERR_HEAD_DIM


def _lib():
    import _mi355fa as fa
    return fa


@pytest.fixture
def formula_splits():
    yield
    vck.splits(0)


def _workspace(fa, D):
    """name -> f(): the workspace bytes of each decode call at head dim D (paged: 32 pages of 128 keys = S_cache)"""
    page, mp = 128, SC // 128
    return {
        "fa_fwd_kvcache_workspace_bytes": lambda: fa.lib.fa_fwd_kvcache_workspace_bytes(B, H, HKV, SQ, SC, 0, D),
        "fa_fwd_kvcache_fp8_workspace_bytes": lambda: fa.lib.fa_fwd_kvcache_fp8_workspace_bytes(B, H, HKV, SQ, SC, 0, D),
        "fa_fwd_kvcache_paged_workspace_bytes/16": lambda: fa.lib.fa_fwd_kvcache_paged_workspace_bytes(
            B, H, HKV, SQ, mp, page, 0, D, fa.PAGED_CACHE_16BIT),
        "fa_fwd_kvcache_paged_workspace_bytes/fp8": lambda: fa.lib.fa_fwd_kvcache_paged_workspace_bytes(
            B, H, HKV, SQ, mp, page, 0, D, fa.PAGED_CACHE_FP8_E4M3),
    }


@pytest.mark.parametrize("n", [2, 3, 7])
def test_workspace_functions_take_d256(n, formula_splits):
    fa = _lib()
    vck.splits(n)
    for name, f in _workspace(fa, 256).items():
        assert f() == n * B * H * SQ * (256 + 2) * 4, name
    # the packed call: the plan in front of the same partials, by packed row
    page, mp, T = 128, SC // 128, 11
    for cdt in (fa.PAGED_CACHE_16BIT, fa.PAGED_CACHE_FP8_E4M3):
        got = fa.lib.fa_fwd_kvcache_ragged_workspace_bytes(T, B, H, HKV, mp, page, 256, cdt)
        assert got == rgc.workspace_bytes(n, T, B, H, HKV, 256), cdt
        assert got - rgc.workspace_bytes(1, T, B, H, HKV, 256) == n * H * T * (256 + 2) * 4


def test_one_split_needs_no_partials_at_d256(formula_splits):
    fa = _lib()
    vck.splits(1)
    for name, f in _workspace(fa, 256).items():
        assert f() == 0, name


@pytest.mark.parametrize("D", [96, 192, 512])
def test_other_head_dims_are_still_refused(D, formula_splits):
    fa = _lib()
    vck.splits(2)
    for name, f in _workspace(fa, D).items():
        assert f() == HEAD_DIM, name
        assert fa.lib.fa_last_error().endswith(b"head dim must be 64 or 128"), name
    for cdt in (fa.PAGED_CACHE_16BIT, fa.PAGED_CACHE_FP8_E4M3):
        assert fa.lib.fa_fwd_kvcache_ragged_workspace_bytes(11, B, H, HKV, 32, 128, D, cdt) == HEAD_DIM


def test_training_side_still_refuses_d256():
    fa = _lib()
    for dt in (fa.FP16, fa.BF16):
        assert fa.lib.fa_supported(256, dt) == 0
        assert fa.lib.fa_supported(128, dt) == 1
    buf, p = vck.aligned_ptr()
    rc = fa.lib.fa_fwd(p, p, p, p, p, 1, 1, 8, 8, 256, fa.BF16, 0, 0.0625, None)
    assert rc == HEAD_DIM
    assert fa.lib.fa_last_error() == b"fa_fwd: head dim must be 64 or 128"


STEMS = {"fa_decode_mod_kernel": 12, "fa_decode_paged_kernel": 12, "fa_decode_ragged_kernel": 12,   # 6 variants x 2 dtypes
         "fa_decode_combine_kernel": 2, "fa_decode_combine_ragged_kernel": 2}


def test_library_holds_the_d256_decode_kernels_inside_the_budget():
    found = {s: 0 for s in STEMS}
    for k in codeobj.kernels():
        m = re.match(r"_ZN2fa\d+(\w+?_kernel)ILi256E", k["name"])   # fa::<stem><256, ...>
        if not m or m.group(1) not in STEMS:
            continue
        stem, short = m.group(1), codeobj.demangle_short(k["name"])
        found[stem] += 1
        assert k["wg"] == 256, short
        assert k["vgpr"] + k["agpr"] <= 256, (short, k["vgpr"], k["agpr"])
        assert k["scratch"] == 0 and k["spill"] == 0, (short, k["scratch"], k["spill"])
        assert k["lds"] <= 81920, (short, k["lds"])
    assert found == STEMS


def test_abi_and_function_lists_are_unchanged():
    fa = _lib()
    assert fa.lib.fa_abi_version() == 7 and fa.ABI_VERSION == 7
    inc = lambda n: os.path.join(ROOT, "include", n)
    lists = {
        "mi355fa_kvcache.h": ["fa_fwd_kvcache", "fa_fwd_kvcache_workspace_bytes"],
        "mi355fa_kvcache_fp8.h": ["fa_fwd_kvcache_fp8", "fa_fwd_kvcache_fp8_workspace_bytes"],
        "mi355fa_paged.h": ["fa_fwd_kvcache_paged", "fa_fwd_kvcache_paged_workspace_bytes"],
        "mi355fa_ragged.h": ["fa_fwd_kvcache_ragged", "fa_fwd_kvcache_ragged_workspace_bytes"],
        "mi355fa_softcap.h": ["fa_bwd_dkv_softcap", "fa_bwd_dq_softcap", "fa_fwd_kvcache_softcap", "fa_fwd_softcap"],
        "mi355fa_alibi.h": ["fa_bwd_dkv_alibi", "fa_bwd_dq_alibi", "fa_fwd_alibi", "fa_fwd_kvcache_alibi"],
    }
    for name, want in lists.items():
        assert vck.header_functions(inc(name))[2] == want, name
    sink = vck.header_functions(inc("mi355fa_sink.h"))[2]
    assert "fa_fwd_kvcache_sink" in sink and "fa_fwd_kvcache_fp8_sink" in sink
    # every decode header says that its call takes D = 256; mi355fa.h does not mention it
    for name in list(lists) + ["mi355fa_sink.h"]:
        assert "256" in vck.header_functions(inc(name))[0], name
    assert "D must be 64 or 128" in open(inc("mi355fa.h")).read()
