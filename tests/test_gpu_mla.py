"""GPU tests of MLA decoding over a paged latent cache (include_mla/mi355fa_kvcache_mla.h, mla_kvcache.flash_attention_mla_kvcache).

Helpers, truth and bounds: tests/mlacheck.py.  1. fp64 parity over head counts that give a mostly empty row block (H = 1), one
block (16), two full blocks and a partial one (24 x S_q 3 = 72 rows) and four blocks (128), S_q 1 .. 3, fill levels of 0 .. 22
tiles so that every split meets empty, odd and even shares, forced splits, three page sizes under a permuted table, NaN
everywhere outside the live keys and out-of-range table entries past the fill.  2. one quarter of the head dim at a time: a
swapped, dropped or doubly counted quarter fails.  3. bit identity across layouts, and a pool beyond 4 GiB.  4. the append.  5. other softmax scales.
6. a captured step replayed while cache_seqlens and block_table change in place.  Shapes are the smallest that reach each path."""
import pytest
import torch

import fa_oracle as fo
import mlacheck as mc
import variantcheck as vck
from mlacheck import BF16, D, DV

pytestmark = pytest.mark.gpu

FILLS = [0, 1, 31, 32, 33, 64, 65, 96, 129, 300, 687]
SPLITS = (0, 1, 2, 3, 7)
PAGES = (32, 64, 128)
S_PAD = 704                                  # 22 tiles: the fill levels' padded cache


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def call(q, pool, lens, table, **kw):
    sl = lens if isinstance(lens, torch.Tensor) else torch.tensor(lens, dtype=torch.int32, device="cuda")
    return mc.M()(q, pool, sl, table, return_lse=True, **kw)


# ---- 1. fp64 parity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("Sq", [1, 2, 3])
@pytest.mark.parametrize("H", [1, 16, 24, 128])
def test_parity_with_fp64_at_every_fill_level_split_and_page_size(H, Sq, dtype):
    q, kv = mc.make(len(FILLS), H, Sq, S_PAD, dtype, seed=H * 10 + Sq)
    for causal in (False, True):
        O, LSE = mc.truth(q, kv, FILLS, causal)
        level = mc.sdpa_level(q, kv, FILLS, causal, None, O) if dtype == BF16 else None
        for page in PAGES:
            pool, table = mc.scatter(kv, FILLS, page, mc.pages_of(S_PAD, page), 3)
            for n in SPLITS:
                vck.splits(n)
                got = call(q, pool, FILLS, table, is_causal=causal)
                mc.held("parity H%d Sq%d %s causal%d page%d n%d" % (H, Sq, mc.IDS[mc.DT.index(dtype)], causal, page, n), q, *got, O,
                        LSE, FILLS, level)
                assert mc.same(got, call(q, pool, FILLS, table, is_causal=causal)), ("a split count repeats its own bits", page, n)


# ---- 2. one quarter at a time ----------------------------------------------------------------------------------------------
QL, QH, QS, QP = [65, 300], 16, 2, 64


def quarter_problem(dtype, seed):
    q, kv = mc.make(len(QL), QH, QS, 320, dtype, seed=seed)
    return q, kv


def run_quarter(tag, q, kv, dtype):
    O, LSE = mc.truth(q, kv, QL, True)
    level = mc.sdpa_level(q, kv, QL, True, None, O) if dtype == BF16 else None
    pool, table = mc.scatter(kv, QL, QP, 5, 7)
    out = None
    for n in (1, 3):
        vck.splits(n)
        out = call(q, pool, QL, table, is_causal=True)
        mc.held("%s n%d" % (tag, n), q, *out, O, LSE, QL, level)
    return out, O


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("w", range(4))
def test_one_latent_quarter_alone(w, dtype):
    q0, kv0 = quarter_problem(dtype, 40 + w)
    q, kv = torch.zeros_like(q0), torch.zeros_like(kv0)
    cols = slice(128 * w, 128 * w + 128)
    q[..., cols], kv[..., cols] = q0[..., cols] * 2, kv0[..., cols]
    (o, _), _ = run_quarter("latent quarter %d" % w, q, kv, dtype)
    rest = torch.ones(DV, dtype=torch.bool)
    rest[cols] = False
    assert (o[..., rest.cuda()] == 0).all() and (o[..., cols] != 0).any()


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("w", range(4))
def test_one_rope_slice_alone(w, dtype):
    """V is the latent part, all zero here: O = 0 exactly and the scores show in LSE alone (q amplified so that a dropped slice,
    LSE = log of the key count, is far outside its tolerance)."""
    q0, kv0 = quarter_problem(dtype, 50 + w)
    q, kv = torch.zeros_like(q0), torch.zeros_like(kv0)
    cols = slice(DV + 16 * w, DV + 16 * w + 16)
    q[..., cols], kv[..., cols] = q0[..., cols] * 8, kv0[..., cols]
    (o, lse), _ = run_quarter("rope slice %d" % w, q, kv, dtype)
    assert (o == 0).all()
    _, flat = mc.truth(torch.zeros_like(q), kv, QL, True)
    assert (lse.double() - flat)[~torch.isinf(flat)].abs().max() > 0.05       # the reference-only condition: the slice matters


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("w", range(4))
def test_a_zero_latent_quarter_of_the_cache_gives_a_zero_quarter_of_o(w, dtype):
    q, kv = quarter_problem(dtype, 60 + w)
    cols = slice(128 * w, 128 * w + 128)
    kv[..., cols] = 0
    (o, _), _ = run_quarter("zero quarter %d" % w, q, kv, dtype)
    assert (o[..., cols] == 0).all()


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_rope_columns_of_the_cache_are_no_part_of_v(dtype):
    q, kv = quarter_problem(dtype, 70)
    q[..., DV:] = 0
    big = kv.clone()
    big[..., DV:] = (torch.randn_like(kv[..., DV:].float()) * 1000).to(dtype)
    kv[..., DV:] = 0
    for n in (1, 3):
        vck.splits(n)
        outs = []
        for x in (kv, big):
            pool, table = mc.scatter(x, QL, QP, 5, 7)
            outs.append(call(q, pool, QL, table, is_causal=True))
        assert mc.same(*outs), n
    run_quarter("rope columns zero", q, kv, dtype)


# ---- 3. bit identity -------------------------------------------------------------------------------------------------------
IL, IH, IS = [0, 33, 129, 300, 384], 24, 3          # 384: the whole table


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_layouts_give_the_same_bits(dtype):
    q, kv = mc.make(len(IL), IH, IS, 384, dtype, seed=80)
    for n in (0, 3):
        vck.splits(n)
        pool, table = mc.scatter(kv, IL, 64, 6, 9)
        ref = call(q, pool, IL, table, is_causal=True)
        # the identity table on the gathered pool
        ipool, itable = mc.scatter(kv, IL, 64, 6, 9, identity=True)
        assert mc.same(ref, call(q, ipool, IL, itable, is_causal=True)), ("identity table", n)
        # the padded cache as a pool of B pages of 384 rows
        padded = kv.clone()
        for b, L in enumerate(IL):
            padded[b, L:] = float("nan")
        ptable = torch.arange(len(IL), dtype=torch.int32, device="cuda")[:, None]
        assert mc.same(ref, call(q, padded, IL, ptable, is_causal=True)), ("padded as a pool", n)
        # strided q: a transposed view, a slice of a wider tensor
        qt = q.transpose(1, 2).contiguous().transpose(1, 2)
        assert not qt.is_contiguous() and mc.same(ref, call(qt, pool, IL, table, is_causal=True)), ("transposed q", n)
        qw = torch.full((len(IL), IH, IS, 640), float("nan"), dtype=dtype, device="cuda")
        qw[..., 32:32 + D] = q
        assert mc.same(ref, call(qw[..., 32:32 + D], pool, IL, table, is_causal=True)), ("sliced q", n)
        # a pool with row stride 640
        spool, stable = mc.scatter(kv, IL, 64, 6, 9, row_stride=640)
        assert spool.stride(1) == 640 and torch.equal(stable, table)
        assert mc.same(ref, call(q, spool, IL, stable, is_causal=True)), ("row stride 640", n)
        # out= through its strides
        wide = torch.full((len(IL), IS, IH, DV + 64), float("nan"), dtype=dtype, device="cuda")
        view = wide[..., :DV].transpose(1, 2)
        o2, lse2 = mc.M()(q, pool, torch.tensor(IL, dtype=torch.int32, device="cuda"), table, is_causal=True, return_lse=True, out=view)
        assert o2.data_ptr() == wide.data_ptr() and mc.same(ref, (view, lse2)) and torch.isnan(wide[..., DV:]).all(), ("out=", n)


def test_a_pool_beyond_4_gib_is_addressed_through_64_bit_page_bases():
    """the sequences' pages at the top of a 4.3 GB pool (uninitialised below them): the bits of the same step on a small pool,
    the appended rows included"""
    page, mp, H, Sq = 64, 3, 16, 2
    lens = [63, 129]
    q, kv = mc.make(len(lens), H, Sq, mp * page, BF16, seed=85)
    new = torch.randn(len(lens), Sq, D, generator=torch.Generator(device="cuda").manual_seed(86), device="cuda").to(BF16)
    small, table = mc.scatter(kv, lens, page, mp, 21, alloc=[L + Sq for L in lens])
    n_big = (1 << 32) // (page * D * 2) + 40
    shift = n_big - small.shape[0]
    assert shift * page * D * 2 > 1 << 32
    big = torch.empty(n_big, page, D, dtype=BF16, device="cuda")
    live = (table >= 0) & (table < small.shape[0])
    tbig = torch.where(live, table + shift, torch.full_like(table, -1))
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for n in (0, 3):
        vck.splits(n)
        big[shift:] = small
        ps = small.clone()
        want = mc.M()(q, ps, sl, table, kv_new=new, is_causal=True, return_lse=True)
        got = mc.M()(q, big, sl, tbig, kv_new=new, is_causal=True, return_lse=True)
        assert mc.same(want, got), n
        assert torch.equal(big[shift:].view(torch.int16), ps.view(torch.int16)) and not torch.equal(ps.view(torch.int16), small.view(torch.int16))
    del big
    torch.cuda.empty_cache()


# ---- 4. the append ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_append_lands_byte_for_byte_through_the_table(dtype):
    page, mp, Sq, H = 32, 3, 3, 16
    #        inside a page, across a page edge, into a fresh page, past the table (rows 96, 97 dropped), an out-of-range entry
    fills = [5, 30, 64, 95, 31]
    alloc = [8, 33, 67, 96, 31]                     # sequence 4 has no second page: its entry there is out of range
    q, kv = mc.make(len(fills), H, Sq, mp * page, dtype, seed=90)
    new = torch.randn(len(fills), Sq, D, generator=torch.Generator(device="cuda").manual_seed(91), device="cuda").to(dtype)
    pool, table = mc.scatter(kv, fills, page, mp, 11, alloc=alloc)
    assert not (0 <= int(table[4, 1]) < pool.shape[0])
    want = pool.clone()
    lens_after = []
    for b, f in enumerate(fills):
        for i in range(Sq):
            r = f + i
            pg = int(table[b, r // page]) if r < mp * page else -1
            if 0 <= pg < pool.shape[0]:
                want[pg, r % page] = new[b, i]
        lens_after.append(min(f + Sq, mp * page))
    sl = torch.tensor(fills, dtype=torch.int32, device="cuda")
    for n in (0, 3):
        vck.splits(n)
        got_pool = pool.clone()
        out = mc.M()(q, got_pool, sl, table, kv_new=new, is_causal=True, return_lse=True)
        assert torch.equal(got_pool.view(torch.int16), want.view(torch.int16)), "the pool after the append"
        assert sl.tolist() == fills, "cache_seqlens is not modified"
        assert mc.same(out, call(q, want.clone(), lens_after, table, is_causal=True)), "attention sees the new rows"
    # against fp64 on the sequences whose rows all landed (sequence 4 lost rows to its out-of-range entry: unspecified)
    full = kv.clone()
    for b, f in enumerate(fills):
        full[b, f:min(f + Sq, mp * page)] = new[b, :min(Sq, mp * page - f)]
    keep = [0, 1, 2, 3]
    O, LSE = mc.truth(q[keep], full[keep], [lens_after[b] for b in keep], True)
    level = mc.sdpa_level(q[keep], full[keep], [lens_after[b] for b in keep], True, None, O) if dtype == BF16 else None
    mc.held("append", q[keep], out[0][keep], out[1][keep], O, LSE, [lens_after[b] for b in keep], level)


# ---- 5. the softmax scale --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("scale,qmul", [(192 ** -0.5, 1.0), (1.0, 0.125)], ids=["deepseek", "one"])
def test_other_softmax_scales(scale, qmul, dtype):
    lens = [33, 129, 300]
    q, kv = mc.make(len(lens), 16, 2, 320, dtype, seed=95)
    q = (q.float() * qmul).to(dtype)
    O, LSE = mc.truth(q, kv, lens, True, scale)
    assert fo.rel_fro(mc.truth(q, kv, lens, True)[0], O) > mc.FAR             # reference only: the scale matters here
    level = mc.sdpa_level(q, kv, lens, True, scale, O) if dtype == BF16 else None
    pool, table = mc.scatter(kv, lens, 64, 5, 13)
    for n in (0, 3):
        vck.splits(n)
        mc.held("scale %.4f n%d" % (scale, n), q, *call(q, pool, lens, table, is_causal=True, softmax_scale=scale), O, LSE, lens, level)


# ---- 6. graph replay -------------------------------------------------------------------------------------------------------
def test_captured_step_replays_while_seqlens_and_table_change_in_place():
    page, mp, H, Sq = 64, 3, 16, 1
    B = 3
    q, kv = mc.make(B, H, Sq, mp * page, BF16, seed=97)
    new = torch.randn(B, Sq, D, generator=torch.Generator(device="cuda").manual_seed(98), device="cuda").to(BF16)
    full = [mp * page] * B
    pool0, table = mc.scatter(kv, full, page, mp, 17)                           # every page of the table in use
    sl = torch.tensor([3, page - 1, 2 * page], dtype=torch.int32, device="cuda")
    pool = pool0.clone()
    step = lambda p: mc.M()(q, p, sl, table, kv_new=new, is_causal=True, return_lse=True)
    step(pool0.clone())                                                         # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(pool)
    gen = torch.Generator().manual_seed(99)
    for lens in ([4, page, 2 * page + 1], [page + 7, 2 * page - 1, 3 * page - 1], [0, 1, page]):
        perm = torch.randperm(pool.shape[0], generator=gen).cuda()              # old page -> new page, all in place
        moved = torch.empty_like(pool0)
        moved[perm] = pool0
        pool0 = moved
        pool.copy_(pool0)
        table.copy_(perm[table.long()].to(torch.int32))
        sl.copy_(torch.tensor(lens, dtype=torch.int32))
        eager_pool = pool0.clone()
        eager = step(eager_pool)
        graph.replay()
        torch.cuda.synchronize()
        assert mc.same(out, eager), lens
        assert torch.equal(pool.view(torch.int16), eager_pool.view(torch.int16)) and not torch.equal(eager_pool.view(torch.int16), pool0.view(torch.int16))
        pool0 = eager_pool
