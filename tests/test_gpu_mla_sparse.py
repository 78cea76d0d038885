"""GPU tests of sparse (top-k indexed) MLA decoding over the paged latent cache (include_mla_sparse/mi355fa_kvcache_mla_sparse.h,
mla_sparse_kvcache.flash_attention_mla_kvcache_sparse).

Helpers, truth and bounds: tests/mlasparsecheck.py over tests/mlacheck.py.  1. fp64 parity: H of one row, half a head block and
a full block with a partial one, lists of 1, 33, 64 and 160 entries full of padding, garbage, duplicates and positions behind
the query, fill levels 0 (keyless rows) and 1 (single-key rows) to 300 under permuted tables with NaN outside the live keys,
forced splits.  2. every key of a tile in a page of its own.  3. the append.  4. bit identity across layouts.  5. graph replay."""
import pytest
import torch

import mlacheck as mc
import mlasparsecheck as ms
import variantcheck as vck
from mlacheck import BF16, D, DV

pytestmark = pytest.mark.gpu

FILLS = [0, 1, 31, 33, 129, 300]
S_PAD = 320                                  # the table's reach


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def call(q, pool, idx, lens, table, **kw):
    sl = lens if isinstance(lens, torch.Tensor) else torch.tensor(lens, dtype=torch.int32, device="cuda")
    return ms.S()(q, pool, idx, sl, table, return_lse=True, **kw)


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("topk", [1, 33, 64, 160])
@pytest.mark.parametrize("Sq", [1, 3])
@pytest.mark.parametrize("H", [1, 16, 40])
def test_parity_with_fp64_over_lists_fill_levels_pages_and_splits(H, Sq, topk, dtype):
    q, kv = mc.make(len(FILLS), H, Sq, S_PAD, dtype, seed=H * 10 + Sq)
    idx = ms.draw(FILLS, Sq, topk, seed=topk + Sq).cuda()
    for causal in (False, True):
        ref = ms.reference(q, kv, idx, FILLS, causal)
        for page in (32, 64):
            pool, table = mc.scatter(kv, FILLS, page, S_PAD // page, 3)
            for n in (0, 1, 3):
                vck.splits(n)
                got = call(q, pool, idx, FILLS, table, is_causal=causal)
                ms.held("sparse parity H%d Sq%d topk%d %s causal%d page%d n%d" % (H, Sq, topk, mc.IDS[mc.DT.index(dtype)], causal, page, n),
                        ref, got)
                assert mc.same(got, call(q, pool, idx, FILLS, table, is_causal=causal)), ("a repeated call gives the same bits", page, n)


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_every_key_of_a_tile_in_a_page_of_its_own(dtype):
    """64 entries a page apart (and a different row in each page) across a 65-page table, ascending in sequence 0 and
    descending in sequence 1: a descriptor shared by the 32 keys of a tile gets this wrong"""
    page, topk, H = 32, 64, 16
    lens = [topk * page + 1] * 2
    q, kv = mc.make(2, H, 1, 65 * page, dtype, seed=31)
    up = torch.arange(topk, dtype=torch.int32) * page + torch.arange(topk, dtype=torch.int32) % page
    idx = torch.stack([up, up.flip(0)])[:, None].cuda()
    pool, table = mc.scatter(kv, lens, page, 65, 5)
    ref = ms.reference(q, kv, idx, lens, False)
    for n in (1, 2):
        vck.splits(n)
        ms.held("sparse own-page %s n%d" % (mc.IDS[mc.DT.index(dtype)], n), ref, call(q, pool, idx, lens, table))


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_append_lands_before_attention_and_lists_may_name_the_new_rows(dtype):
    page, mp, Sq, H, topk = 32, 3, 3, 16, 40
    fills = [5, 30, 62]                              # inside a page, across a page edge, up to the edge of a fresh page
    after = [f + Sq for f in fills]
    q, kv = mc.make(len(fills), H, Sq, mp * page, dtype, seed=90)
    new = torch.randn(len(fills), Sq, D, generator=torch.Generator(device="cuda").manual_seed(91), device="cuda").to(dtype)
    full = kv.clone()
    for b, f in enumerate(fills):
        full[b, f:f + Sq] = new[b]
    pool, table = mc.scatter(kv, fills, page, mp, 11, alloc=after)
    want, _ = mc.scatter(full, after, page, mp, 11)
    idx = torch.stack([ms.draw([L], Sq, topk, seed=b, lead=(L - 1, L - 2, L - 3))[0] for b, L in enumerate(after)]).cuda()
    sl = torch.tensor(fills, dtype=torch.int32, device="cuda")
    ref = ms.reference(q, full, idx, after, True)
    for n in (0, 3):
        vck.splits(n)
        got_pool = pool.clone()
        out = ms.S()(q, got_pool, idx, sl, table, kv_new=new, is_causal=True, return_lse=True)
        assert torch.equal(got_pool.view(torch.int16), want.view(torch.int16)), "the pool after the append"
        assert sl.tolist() == fills, "cache_seqlens is not modified"
        ms.held("sparse append %s n%d" % (mc.IDS[mc.DT.index(dtype)], n), ref, out)


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_layouts_give_the_same_bits(dtype):
    lens, H, Sq, topk = [0, 33, 129, 300], 40, 3, 70
    q, kv = mc.make(len(lens), H, Sq, S_PAD, dtype, seed=80)
    idx = ms.draw(lens, Sq, topk, seed=81).cuda()
    pool, table = mc.scatter(kv, lens, 64, 5, 9)
    for n in (0, 3):
        vck.splits(n)
        ref = call(q, pool, idx, lens, table, is_causal=True)
        wide = torch.full((len(lens), Sq + 1, topk + 9), 7, dtype=torch.int32, device="cuda")   # 7: a visible position
        wide[:, :Sq, 4:4 + topk] = idx
        sliced = wide[:, :Sq, 4:4 + topk]
        assert not sliced.is_contiguous() and mc.same(ref, call(q, pool, sliced, lens, table, is_causal=True)), ("strided indices", n)
        qt = q.transpose(1, 2).contiguous().transpose(1, 2)                                      # a [B, S_q, H, 576] tensor
        assert not qt.is_contiguous() and mc.same(ref, call(qt, pool, idx, lens, table, is_causal=True)), ("transposed q", n)
        padded = torch.full((len(lens), H, Sq, DV + 64), float("nan"), dtype=dtype, device="cuda")
        o2, lse2 = call(q, pool, idx, lens, table, is_causal=True, out=padded[..., :DV])
        assert o2.data_ptr() == padded.data_ptr() and mc.same(ref, (padded[..., :DV], lse2)) and torch.isnan(padded[..., DV:]).all(), ("out=", n)


def test_captured_step_replays_while_indices_seqlens_and_table_change_in_place():
    page, mp, H, B, topk = 64, 5, 16, 3, 70
    q, kv = mc.make(B, H, 1, mp * page, BF16, seed=97)
    pool, table = mc.scatter(kv, [mp * page] * B, page, mp, 17)                 # every page of the table in use
    sl = torch.tensor([3, page - 1, 2 * page], dtype=torch.int32, device="cuda")
    idx = ms.draw(sl.tolist(), 1, topk, seed=1).cuda()
    step = lambda: ms.S()(q, pool, idx, sl, table, is_causal=True, return_lse=True)
    step()                                                                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for k, lens in enumerate(([4, page, 2 * page + 1], [page + 7, 300, 3 * page - 1], [0, 1, page])):
        table.copy_(table.roll(1, 0))                                           # sequence b now owns the pages of b - 1: in place
        kv = kv.roll(1, 0)
        sl.copy_(torch.tensor(lens, dtype=torch.int32))
        idx.copy_(ms.draw(lens, 1, topk, seed=2 + k))
        eager = step()
        graph.replay()
        torch.cuda.synchronize()
        assert mc.same(out, eager), lens
        ms.held("sparse replay %d" % k, ms.reference(q, kv, idx, lens, True), out)
