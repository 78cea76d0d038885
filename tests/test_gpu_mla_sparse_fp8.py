"""GPU tests of sparse (top-k indexed) MLA decoding over the paged FP8 latent cache
(mla_sparse_fp8_kvcache.flash_attention_mla_kvcache_sparse_fp8).

Truth: tests/mlasparsecheck.gather on the cache DEQUANTISED in fp64, then tests/mlacheck.truth on the gathered problem and, for
bf16, mlacheck.sdpa_level on the gathered rows cast to bf16; bounds: mlacheck.held's (quantisation error is no part of them).
Pools: tests/mlafp8check.scatter -- permuted tables, NaN bytes, NaN scales and NaN RoPE values everywhere nothing may read --
over rows of mlafp8check.with_scales, whose four blocks differ by large factors per key.  1. parity.  2. every key of a tile in
a page of its own.  3. one quarter's scale.  4. live and dead tiles.  5. the append.  6. layouts."""
import pytest
import torch

import mlacheck as mc
import mlafp8check as f8
import mlasparsecheck as ms
import variantcheck as vck
from mlacheck import BF16, DT, DV, IDS

pytestmark = pytest.mark.gpu

FILLS = [0, 1, 31, 33, 129, 300]
S_PAD = 320                                  # the table's reach
BROAD = 1 / 128                              # tests/test_gpu_mla_fp8.py: the softmax scale that keeps with_scales' rows broad


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def call(q, pool, idx, lens, table, n=0, **kw):
    import mla_sparse_fp8_kvcache
    vck.splits(n)
    sl = lens if isinstance(lens, torch.Tensor) else torch.tensor(lens, dtype=torch.int32, device="cuda")
    return mla_sparse_fp8_kvcache.flash_attention_mla_kvcache_sparse_fp8(q, pool, idx, sl, table, return_lse=True, **kw)


def reference(q, rows, idx, lens, causal, scale=None):
    """mlasparsecheck.reference over quantised rows [B, S, 656]: what mlasparsecheck.held needs beside a call's result"""
    kvd = f8.F().dequantize_mla_latent_fp8(rows, q.dtype, torch.float64)
    qf, g, counts = ms.gather(q, kvd, idx, lens, causal)
    O, LSE = mc.truth(qf, g, counts, False, scale)
    level = mc.sdpa_level(qf, g.to(q.dtype), counts, False, scale, O) if q.dtype == BF16 else None
    return qf, O, LSE, counts, level


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("topk", [1, 33, 160])
@pytest.mark.parametrize("Sq", [1, 3])
@pytest.mark.parametrize("H", [1, 40])
def test_parity_with_fp64_over_lists_fill_levels_pages_and_splits(H, Sq, topk, dtype):
    q, kv = mc.make(len(FILLS), H, Sq, S_PAD, dtype, seed=H * 10 + Sq)
    rows = f8.with_scales(kv, 20 + topk)
    idx = ms.draw(FILLS, Sq, topk, seed=topk + Sq).cuda()
    for causal in (False, True):
        ref = reference(q, rows, idx, FILLS, causal, BROAD)
        for page in (32, 64):
            stride = 672 if (page, H) == (64, 40) else f8.ROW            # one configuration with padded rows
            pool, table = f8.scatter(rows, dtype, FILLS, page, S_PAD // page, 3, row_stride=stride)
            for n in (0, 1, 3):
                tag = "sparse-fp8 parity H%d Sq%d topk%d %s causal%d page%d n%d" % (H, Sq, topk, IDS[DT.index(dtype)], causal, page, n)
                got = call(q, pool, idx, FILLS, table, n, is_causal=causal, softmax_scale=BROAD)
                ms.held(tag, ref, got)
                assert mc.same(got, call(q, pool, idx, FILLS, table, n, is_causal=causal, softmax_scale=BROAD)), (tag, "a repeated call")


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_every_key_of_a_tile_in_a_page_of_its_own(dtype):
    """64 entries a page apart (and a different row in each page) across a 65-page table, ascending in sequence 0 and
    descending in sequence 1: a descriptor or a scale shared by the 32 keys of a tile gets this wrong"""
    page, topk, H = 32, 64, 16
    lens = [topk * page + 1] * 2
    q, kv = mc.make(2, H, 1, 65 * page, dtype, seed=31)
    rows = f8.with_scales(kv, 32)
    up = torch.arange(topk, dtype=torch.int32) * page + torch.arange(topk, dtype=torch.int32) % page
    idx = torch.stack([up, up.flip(0)])[:, None].cuda()
    pool, table = f8.scatter(rows, dtype, lens, page, 65, 5)
    ref = reference(q, rows, idx, lens, False, BROAD)
    for n in (1, 2):
        ms.held("sparse-fp8 own-page %s n%d" % (IDS[DT.index(dtype)], n), ref, call(q, pool, idx, lens, table, n, softmax_scale=BROAD))


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("w", range(4))
def test_one_quarters_scale_moves_that_quarter_of_o_and_nothing_else(w, dtype):
    """q is zero on the latent columns, so the scores do not depend on the scales: block w's scales times 4 give the truth with
    columns [128 w, + 128) times 4, the other columns' bits and the LSE's bits as they were"""
    q, rows = f8.column_problem("vscale", w, dtype)
    idx = ms.draw(f8.COL_LENS, f8.COL_SQ, ms.COL_TOPK, seed=190 + w).cuda()
    big = f8.scaled_block(rows, w, 4.0)
    mine = torch.zeros(DV, dtype=torch.bool, device="cuda")
    mine[128 * w:128 * w + 128] = True
    ref, ref4 = reference(q, rows, idx, f8.COL_LENS, True), reference(q, big, idx, f8.COL_LENS, True)
    assert torch.equal(ref4[1][..., mine], 4 * ref[1][..., mine]) and torch.equal(ref4[1][..., ~mine], ref[1][..., ~mine])
    for n in (0, 3):
        got = []
        for name, r, x in (("base", ref, rows), ("x4", ref4, big)):
            pool, table = f8.scatter(x, dtype, f8.COL_LENS, f8.COL_PAGE, 5, seed=7)
            got.append(call(q, pool, idx, f8.COL_LENS, table, n, is_causal=True))
            ms.held("sparse-fp8 v-scale %d %s %s n%d" % (w, name, IDS[DT.index(dtype)], n), r, got[-1])
        (o, lse), (o4, lse4) = got
        assert torch.equal(lse.view(torch.int32), lse4.view(torch.int32)), n
        assert torch.equal(o[..., ~mine].view(torch.int16), o4[..., ~mine].view(torch.int16)), n
        assert not torch.equal(o[..., mine], o4[..., mine]), n


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("kind", ["minus-one", "past-L"])
@pytest.mark.parametrize("pattern", ["LDL", "DDDL", "DLDLDLD"])
def test_dead_tiles_are_passed_over_wherever_they_stand(pattern, kind, dtype):
    """the skip, the exchange slots' parity by steps taken, the scale slot across a skipped tile, and the NaN rows and scales
    behind L that a dead entry must not touch"""
    L, page, mp, Sq = ms.PAT_L, ms.PAT_PAGE, ms.PAT_MP, 2
    q, kv = mc.make(1, 16, Sq, S_PAD, dtype, seed=len(pattern) * 10 + Sq)
    rows = f8.with_scales(kv, 60 + len(pattern))
    pool, table = f8.scatter(rows, dtype, [L], page, mp, 3)
    idx = ms.pattern_lists(L, Sq, pattern, kind, 50, mp * page).cuda()
    ref = reference(q, rows, idx, [L], True, BROAD)
    for n in (0, 3):
        got = call(q, pool, idx, [L], table, n, is_causal=True, softmax_scale=BROAD)
        ms.held("sparse-fp8 skip %s %s %s n%d" % (pattern, kind, IDS[DT.index(dtype)], n), ref, got)
        assert mc.same(got, call(q, pool, idx, [L], table, n, is_causal=True, softmax_scale=BROAD)), ("a repeated call", n)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_append_quantises_bit_exactly_before_attention_and_only_its_rows(dtype):
    page, mp, Sq, H, topk = 32, 3, 3, 16, 40
    fills = [5, 30, 62]                              # inside a page, across a page edge, up to the edge of a fresh page
    after = [x + Sq for x in fills]
    q, kv = mc.make(len(fills), H, Sq, mp * page, dtype, seed=90)
    new = torch.randn(len(fills), Sq, mc.D, generator=torch.Generator(device="cuda").manual_seed(91), device="cuda").to(dtype)
    new[0, 0, 128:256] = 0                           # an all-zero block: scale 1.0
    new[1, 1, 300] = 900.0                           # an outlier sets its block's scale alone
    full = kv.clone()
    for b, x in enumerate(fills):
        full[b, x:x + Sq] = new[b]
    quant = lambda x: f8.F().quantize_mla_latent_fp8(x.cpu()).cuda()     # on the CPU: the correctly rounded amax / 448
    rows, rows_full = quant(kv), quant(full)
    pool, table = f8.scatter(rows, dtype, fills, page, mp, 11, alloc=after)
    want, _ = f8.scatter(rows_full, dtype, after, page, mp, 11)
    idx = torch.stack([ms.draw([L], Sq, topk, seed=b, lead=(L - 1, L - 2, L - 3))[0] for b, L in enumerate(after)]).cuda()
    sl = torch.tensor(fills, dtype=torch.int32, device="cuda")
    ref = reference(q, rows_full, idx, after, True)
    for n in (0, 3):
        mine = pool.clone()
        out = call(q, mine, idx, sl, table, n, kv_new=new, is_causal=True)
        assert torch.equal(mine, want), ("the pool after the append differs at", (mine != want).nonzero()[:4].tolist())
        assert sl.tolist() == fills, "cache_seqlens is not modified"
        ms.held("sparse-fp8 append %s n%d" % (IDS[DT.index(dtype)], n), ref, out)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_layouts_give_the_same_bits(dtype):
    lens, H, Sq, topk = [0, 33, 129, 300], 40, 3, 70
    q, kv = mc.make(len(lens), H, Sq, S_PAD, dtype, seed=80)
    idx = ms.draw(lens, Sq, topk, seed=81).cuda()
    pool, table = f8.scatter(f8.with_scales(kv, 82), dtype, lens, 64, 5, 9)
    for n in (0, 3):
        ref = call(q, pool, idx, lens, table, n, is_causal=True)
        wide = torch.full((len(lens), Sq + 1, topk + 9), 7, dtype=torch.int32, device="cuda")   # 7: a visible position
        wide[:, :Sq, 4:4 + topk] = idx
        sliced = wide[:, :Sq, 4:4 + topk]
        assert not sliced.is_contiguous() and mc.same(ref, call(q, pool, sliced, lens, table, n, is_causal=True)), ("strided indices", n)
        qt = q.transpose(1, 2).contiguous().transpose(1, 2)                                      # a [B, S_q, H, 576] tensor
        assert not qt.is_contiguous() and mc.same(ref, call(qt, pool, idx, lens, table, n, is_causal=True)), ("transposed q", n)
        padded = torch.full((len(lens), H, Sq, DV + 64), float("nan"), dtype=dtype, device="cuda")
        o2, lse2 = call(q, pool, idx, lens, table, n, is_causal=True, out=padded[..., :DV])
        assert o2.data_ptr() == padded.data_ptr() and mc.same(ref, (padded[..., :DV], lse2)) and torch.isnan(padded[..., DV:]).all(), ("out=", n)
