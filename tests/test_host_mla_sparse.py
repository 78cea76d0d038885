"""CPU tests of sparse (top-k indexed) MLA decoding (include_mla_sparse/mi355fa_kvcache_mla_sparse.h, mla_sparse_kvcache.py): the
refusals of the C call, the workspace function against the split rule, the new kernels' resources from the code objects, and
the gather of tests/mlasparsecheck.py on a hand-built example."""
import ctypes
import os
import re
import sys

import pytest
import torch

from conftest import ROOT
import mlasparsecheck as ms
import variantcheck as vck
from test_host_mla import splits_formula

NULL, SHAPE, DTYPE, ALIGN, STRIDE, WORKSPACE, PAGED = -1, -2, -4, -5, -6, -9, -12
FN = "fa_fwd_kvcache_mla_sparse"
ARGS = ("q", "kv", "new", "idx", "sl", "bt", "o", "lse", "ws", "wsb", "B", "H", "Sq", "topk", "pages", "page", "mp", "bts", "Snew",
        "dtype", "scale", "causal", "qs", "ks", "os", "xs")


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def _call(fa, p, **kw):
    a = dict(q=p, kv=p, new=None, idx=p, sl=p, bt=p, o=p, lse=p, ws=p, wsb=1 << 30, B=2, H=16, Sq=1, topk=64, pages=8, page=64, mp=4,
             bts=4, Snew=0, dtype=fa.BF16, scale=576 ** -0.5, causal=1, qs=None, ks=None, os=None, xs=None)
    a.update(kw)
    return fa.lib.fa_fwd_kvcache_mla_sparse(*[a[k] for k in ARGS], None)


ST = lambda *v: (ctypes.c_longlong * len(v))(*v)
REFUSALS = [                                                      # ("p+n": the aligned buffer's address plus n)
    (dict(q=None), NULL, "q is NULL (argument 1)"),
    (dict(idx=None), NULL, "indices is NULL (argument 4)"),
    (dict(Snew=1), NULL, "S_new > 0 needs kv_new (S_new 1)"),
    (dict(dtype=2), DTYPE, "dtype must be 0 (fp16) or 1 (bf16) (got 2)"),
    (dict(scale=0.0), SHAPE, "scale must be finite and > 0 (its bits are 0)"),
    (dict(topk=0), SHAPE, "topk must be in [1, 2^24] (got 0)"),
    (dict(topk=(1 << 24) + 1), SHAPE, "topk must be in [1, 2^24] (got 16777217)"),
    (dict(page=48), PAGED, "page_size must be a positive multiple of 32 (got 48)"),
    (dict(bts=3), PAGED, "block_table_stride must be at least max_pages_per_seq and below 2^31 (got 3)"),
    (dict(qs=ST(0, 580, 576)), STRIDE, "q_strides must be non-negative multiples of 8 elements (got 580)"),
    (dict(ks=ST(36864, 580)), STRIDE, "the row stride of kv_pool must be a multiple of 8 elements (16-byte rows) and at least 576 (got 580)"),
    (dict(xs=ST(64, -64)), STRIDE, "indices_strides must be non-negative and at most 2^40 elements (got -64)"),
    (dict(kv="p+4"), ALIGN, "kv_pool must be 16-byte aligned (ends in 4)"),
    (dict(idx="p+2"), ALIGN, "indices must be 4-byte aligned (ends in 2)"),
]


@pytest.mark.parametrize("kw,code,text", REFUSALS, ids=[t.split(" (")[0][:40] for _, _, t in REFUSALS])
def test_c_refusals_name_the_argument_and_carry_the_value(kw, code, text):
    import _mi355fa as fa
    buf, p = vck.aligned_ptr()
    kw = {k: p + int(v[2:]) if isinstance(v, str) else v for k, v in kw.items()}
    assert _call(fa, p, **kw) == code, fa.lib.fa_last_error()
    assert fa.lib.fa_last_error().decode() == FN + ": " + text


def test_workspace_bytes_follow_the_split_rule_and_the_forced_count():
    """the rule: mla_splits with topk in the place of S_cache over B * S_q * ceil(H / 32) workgroups per split"""
    import _mi355fa as fa
    ws = fa.lib.fa_fwd_kvcache_mla_sparse_workspace_bytes
    seen = set()
    for B, H, Sq, topk in [(1, 1, 1, 1), (8, 128, 1, 2048), (8, 16, 1, 2048), (3, 40, 3, 160), (1, 16, 2, 1 << 20), (600, 16, 1, 2048)]:
        n = splits_formula(B * Sq, H, 1, topk)
        seen.add(n)
        for S_new in (0, Sq):
            assert ws(B, H, Sq, topk, 4, 64, S_new) == (n * B * H * Sq * 514 * 4 if n > 1 else 0), (B, H, Sq, topk, n)
        for forced in (1, 7):
            vck.splits(forced)
            assert ws(B, H, Sq, topk, 4, 64, 0) == (forced * B * H * Sq * 514 * 4 if forced > 1 else 0)
        vck.splits(0)
    assert {1, 11, 64} <= seen
    buf, p = vck.aligned_ptr()
    vck.splits(3)
    need = ws(2, 16, 1, 64, 4, 64, 0)
    assert need == 3 * 2 * 16 * 514 * 4 and _call(fa, p, wsb=need - 1) == WORKSPACE
    assert fa.lib.fa_last_error().decode() == FN + ": workspace smaller than %s_workspace_bytes() (%d bytes)" % (FN, need)
    assert ws(2, 16, 1, 0, 4, 64, 0) == SHAPE
    assert fa.lib.fa_last_error().decode() == FN + "_workspace_bytes: topk must be in [1, 2^24] (got 0)"


def test_two_new_kernels_are_in_the_library_inside_the_decode_budget():
    """the <Topk, T> overload of fa_decode_paged_kernel over TopkParams, fp16 and bf16, and no other kernel with the tag:
    workgroup 256, VGPR + AGPR <= 256, no scratch, no spills, LDS within 80 KiB (the carve is dynamic: the source asserts it)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj
    found = []
    for k in codeobj.kernels():
        if "Topk" not in k["name"]:
            continue
        m = re.match(r"_ZN2fa22fa_decode_paged_kernelINS_4TopkENS_4(BF16|FP16)EEEvNS_10TopkParamsE$", k["name"])
        assert m, "a kernel with the sparse tag outside the expected set: " + k["name"]
        found.append(m.group(1))
        assert k["wg"] == 256 and k["vgpr"] + k["agpr"] <= 256, (k["name"], k["vgpr"], k["agpr"])
        assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 81920, k["name"]
    assert sorted(found) == ["BF16", "FP16"], found
    src = open(os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd", "csrc", "fa_decode_mla_sparse.hip")).read()
    assert 'static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU")' in src


def test_the_gather_on_three_keys():
    """L = 5, S_q = 2 (positions 3 and 4): list [4, -1, 1, 9, 1] keeps 4, 1, 1 without the mask; under causal query 0 loses 4"""
    kv = torch.arange(6.0)[None, :, None].expand(1, 6, 576).contiguous()
    idx = torch.tensor([[[4, -1, 1, 9, 1], [5, 3, 3, 0, 1 << 30]]], dtype=torch.int32)
    qf, rows, counts = ms.gather(torch.ones(1, 3, 2, 576), kv, idx, [5], False)
    assert qf.shape == (2, 3, 1, 576) and counts == [3, 3] and rows[:, :, 0].tolist() == [[4, 1, 1], [3, 3, 0]]
    qf, rows, counts = ms.gather(torch.ones(1, 3, 2, 576), kv, idx, [5], True)
    assert counts == [2, 3] and rows[:, :, 0].tolist() == [[1, 1, 0], [3, 3, 0]]


# ---------------------------------------------------------------- the conditions of tests/test_gpu_mla_sparse_deep.py
@pytest.mark.parametrize("kind", ms.DEAD)
@pytest.mark.parametrize("pattern", ms.PATTERNS)
def test_pattern_lists_have_their_live_and_dead_tiles(pattern, kind):
    """a dead tile has no visible entry for any query and is wholly of its kind, a live tile has one for every query beside
    junk; the 'past-L' runs are duplicate-free, at or past L and below the table's reach"""
    L, reach = ms.PAT_L, ms.PAT_MP * ms.PAT_PAGE
    for Sq in (1, 3):
        idx = ms.pattern_lists(L, Sq, pattern, kind, 7, reach)
        assert idx.shape == (1, Sq, 32 * len(pattern)) and idx.dtype == torch.int32
        vis = ms.visible(idx, [L], True).view(Sq, len(pattern), 32)
        tiles = idx.view(Sq, len(pattern), 32)
        for t, c in enumerate(pattern):
            n = vis[:, t].sum(-1)
            assert (n == 0).all() if c == "D" else ((n >= 1) & (n < 32)).all(), (pattern, kind, t)
            for i in range(Sq):
                e, pos = tiles[i, t], L - Sq + i
                if c == "L":
                    assert ((e < 0) | (e >= L)).any()
                elif kind == "past-L":
                    assert e.unique().numel() == 32 and (e >= L).all() and (e < reach).all()
                elif kind == "behind" and pos < L - 1:
                    assert ((e > pos) & (e < L)).all()
                else:
                    assert (e == {"minus-one": -1, "L": L, "huge": 1 << 30, "int-min": -(1 << 31), "behind": L}[kind]).all()


def test_split_boundaries_fall_inside_dead_runs_and_forced_counts_leave_empty_splits():
    """n = 2 and n = 3: for one pattern each every boundary nt * split / nsplit lies between two dead tiles, so a split starts
    and ends in skipped tiles (its prologue loads dead tiles, its step count starts at 0 behind them)"""
    inside = lambda pat, n: all(pat[ms.split_range(len(pat), s, n)[0] - 1] == "D" and pat[ms.split_range(len(pat), s, n)[0]] == "D"
                                for s in range(1, n))
    assert inside("LDDL", 2) and inside("LDDDDL", 3)
    assert [ms.split_range(4, s, 2) for s in range(2)] == [(0, 2), (2, 4)]
    assert [ms.split_range(6, s, 3) for s in range(3)] == [(0, 2), (2, 4), (4, 6)]
    # some split of every pattern is wholly dead at n = 2 or 3 or holds live tiles on both sides of a dead one
    for pat in ms.PATTERNS:
        nt = len(pat)
        assert [ms.split_range(nt, s, nt + 2) for s in range(nt + 2)].count((0, 0)) >= 1       # n = nt + 2: empty splits
        assert sum(b - a for a, b in (ms.split_range(nt, s, nt + 2) for s in range(nt + 2))) == nt


def test_the_deepseek_scale_of_the_gpu_test_is_far_from_the_default():
    import fa_oracle as fo
    import mlacheck as mc
    lens = [33, 129, 300]
    for dtype in mc.DT:
        q, kv = mc.make(len(lens), 16, 2, 320, dtype, seed=95, device="cpu")
        idx = ms.draw(lens, 2, 70, seed=96)
        _, O, LSE, counts, _ = ms.reference(q, kv, idx, lens, True, 192 ** -0.5)
        far = fo.rel_fro(ms.reference(q, kv, idx, lens, True)[1], O)
        assert far > mc.FAR and min(counts) > 20, (far, counts)
        assert torch.isfinite(O).all() and torch.isfinite(LSE).all()


def test_one_rope_slice_moves_the_lse_of_the_sparse_column_problem():
    """the reference-only condition of the sparse RoPE-slice test: the truth's LSE differs from the zero-q truth's by > 0.05"""
    import mlacheck as mc
    for dtype in mc.DT:
        for w in range(4):
            q, kv, idx = ms.column_problem("rope", w, dtype, "cpu")
            _, O, LSE, counts, _ = ms.reference(q, kv, idx, ms.COL_LENS, True)
            flat = ms.reference(torch.zeros_like(q), kv, idx, ms.COL_LENS, True)[2]
            assert (O == 0).all() and min(counts) > 10 and ((LSE - flat).abs() > 0.05).float().mean() > 0.9
