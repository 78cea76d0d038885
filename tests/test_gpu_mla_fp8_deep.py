"""MLA decoding over a paged FP8 latent cache, the structural pass: csrc/fa_decode_mla_fp8.hip writes out its own loop, so
none of the 16-bit kernel's structural tests (tests/test_gpu_mla.py) reach it.

Helpers: tests/mlafp8check.py over tests/mlacheck.py; truth fp64 on the DEQUANTISED cache; bounds mlacheck.held's, unchanged.
Every pool is mlafp8check.scatter's: a permuted table, poison (NaN bytes, NaN scales, NaN RoPE) outside the live rows,
out-of-range entries past a sequence's pages.  tests/test_host_mla_fp8.py holds the reference-only conditions on the CPU.

A. One column group at a time (lens 65 / 300: one page and a tile of a second, five pages with a partial tile; S_q 2 so that a
   row block holds both queries; one split and three).  The kernel permutes the contraction index -- k-step 2 j + e reads columns
   32 j + 16 h + 8 e of a quarter on the K side AND the Q side, and writes V at chunk 4 j + 2 h + e -- and applies one scale per
   (wave, key) twice, to the scores and to its copy of P.  The single mistake each test fails under:
     latent quarter alone   a quarter read from or written to another wave's columns, a scale taken from another block
                            (O != 0 outside the quarter, or far off inside it)
     RoPE slice alone       a dropped or swapped RoPE slice (LSE = log of the key count), a scale applied to the RoPE k-step
                            or a NaN-free 0 * scale turned into something else (O != 0)
     zero quarter           a V tile or an accumulator shared between quarters; a scale of 2^20 leaking into another quarter
     RoPE no part of V      bytes [528, 656) of a row reaching the V tile
     one quarter's scale    a scale applied to the scores only or to P only: the scores here come from RoPE alone, so LSE
                            and the other three quarters keep their bits and quarter w follows its own truth; a permutation
                            mistake that cancels between Q and K survives on the V side alone and shows in 'latent quarter'
B. The accumulator's units (`unit`, the row's largest p * scale so far).  One sequence of 8 tiles + 5 keys per ramp, the block
   scales constant within a tile: ascending (unit grows every tile), descending (unit * corr carries), saw-tooth (alternates),
   a spike, the four blocks on different ramps (the four waves' units differ), and both monotone ramps with q non-zero on the
   latent columns (corr != 1 together with a moving unit).  One split and two (a split starts with unit = 0 mid-ramp).
   Fails under: unit never rescaled (oacc *= corr alone), resc = corr * unit_new / unit, the final `oacc *= unit` dropped.
   The range test draws scales 2^e per (key, block) over the widest e the dtype holds (fp16 +-7, bf16 +-119).
C. Geometry the 16-bit kernel is already held to: H 128 over every fill level of 0 .. 22 tiles, pages of 32 / 64 / 128, five
   split counts (a row block that spans queries, splits with empty shares); a deep table at THREE tiles per page (FastDiv by
   3 is no shift; fails under tpp.div replaced by a shift, or a descriptor cut at the wrong row of a page) with the append;
   DeepSeek's softmax scale; a pool beyond 4 GiB (fails under a 32-bit page base); a captured step replayed.
Shapes are the smallest that reach each path."""
import pytest
import torch

import mlacheck as mc
import mlafp8check as f8
import variantcheck as vck
from mlacheck import BF16, DT, DV, IDS

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def ids(dtype):
    return IDS[DT.index(dtype)]


def call(q, pool, lens, table, n=0, **kw):
    vck.splits(n)
    sl = lens if isinstance(lens, torch.Tensor) else torch.tensor(lens, dtype=torch.int32, device="cuda")
    return f8.F().flash_attention_mla_kvcache_fp8(q, pool, sl, table, return_lse=True, **kw)


# ---- A. one column group at a time ---------------------------------------------------------------------------------------------
def run_columns(tag, q, rows, ns=(1, 3)):
    """the column problem (q, rows) at each split count against its truth; {n: (o, lse)}"""
    L = f8.COL_LENS
    _, O, LSE, level = f8.reference(q, rows, L, True)
    pool, table = f8.scatter(rows, q.dtype, L, f8.COL_PAGE, 5, seed=7)
    out = {}
    for n in ns:
        out[n] = call(q, pool, L, table, n, is_causal=True)
        mc.held("fp8 %s %s n%d" % (tag, ids(q.dtype), n), q, *out[n], O, LSE, L, level)
    return out


def quarter(w):
    inside = torch.zeros(DV, dtype=torch.bool, device="cuda")
    inside[128 * w:128 * w + 128] = True
    return inside


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("w", range(4))
def test_one_latent_quarter_alone(w, dtype):
    q, rows = f8.column_problem("latent", w, dtype)
    for n, (o, _) in run_columns("latent quarter %d" % w, q, rows).items():
        assert (o[..., ~quarter(w)] == 0).all() and (o[..., quarter(w)] != 0).any(), n


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("w", range(4))
def test_one_rope_slice_alone(w, dtype):
    """all 512 bytes 0x00 under random scales: O = 0 exactly, the scores show in LSE alone (tests/test_host_mla_fp8.py: the slice
    moves LSE by more than 0.05, far outside its tolerance)"""
    q, rows = f8.column_problem("rope", w, dtype)
    for n, (o, _) in run_columns("rope slice %d" % w, q, rows).items():
        assert (o == 0).all(), n


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("w", range(4))
def test_a_zero_latent_quarter_of_the_cache_gives_a_zero_quarter_of_o(w, dtype):
    q, rows = f8.column_problem("zero", w, dtype)
    for n, (o, _) in run_columns("zero quarter %d" % w, q, rows).items():
        assert (o[..., quarter(w)] == 0).all() and (o[..., ~quarter(w)] != 0).any(), n


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_rope_bytes_of_the_cache_are_no_part_of_v(dtype):
    q, rows = f8.column_problem("ropev", 0, dtype)
    big = rows.clone()
    big[..., f8.ROPE_OFF:] = (torch.randn(*rows.shape[:-1], 64, device="cuda") * 1000).to(dtype).view(torch.uint8)
    rows[..., f8.ROPE_OFF:] = 0
    got = run_columns("rope bytes zero", q, rows)
    pool, table = f8.scatter(big, dtype, f8.COL_LENS, f8.COL_PAGE, 5, seed=7)
    for n in got:
        assert mc.same(got[n], call(q, pool, f8.COL_LENS, table, n, is_causal=True)), n


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("w", range(4))
def test_one_quarters_scale_moves_that_quarter_of_o_and_nothing_else(w, dtype):
    q, rows = f8.column_problem("vscale", w, dtype)
    base = run_columns("v-side scale %d base" % w, q, rows)
    got = run_columns("v-side scale %d" % w, q, f8.scaled_block(rows, w, 0.125))
    for n in base:
        (o, lse), (o2, lse2) = base[n], got[n]
        assert torch.equal(lse.view(torch.int32), lse2.view(torch.int32)), n
        assert torch.equal(o[..., ~quarter(w)].view(torch.int16), o2[..., ~quarter(w)].view(torch.int16)), n
        assert not torch.equal(o[..., quarter(w)], o2[..., quarter(w)]), n


# ---- B. the accumulator's units --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("case", f8.RAMP_CASES)
def test_scale_ramps_over_the_tiles(case, dtype):
    L = [f8.RAMP_L]
    q, rows = f8.ramp_problem(case, dtype)
    _, O, LSE, level = f8.reference(q, rows, L, False)
    pool, table = f8.scatter(rows, dtype, L, 64, 5, seed=4)
    for n in (1, 2):
        o, lse = call(q, pool, L, table, n)
        mc.held("fp8 ramp %s %s n%d" % (case, ids(dtype), n), q, o, lse, O, LSE, L, level)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_scales_over_the_whole_range_the_dtype_holds(dtype):
    q, rows = f8.range_problem(dtype, f8.RANGE_E[dtype])
    L = f8.RANGE_LENS
    _, O, LSE, level = f8.reference(q, rows, L, True)
    pool, table = f8.scatter(rows, dtype, L, 64, 5, seed=6)
    for n in (1, 3):
        o, lse = call(q, pool, L, table, n, is_causal=True)
        assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all(), n
        mc.held("fp8 scale range %s n%d" % (ids(dtype), n), q, o, lse, O, LSE, L, level)


# ---- C. geometry and features ------------------------------------------------------------------------------------------------------
FILLS = [0, 1, 31, 32, 33, 64, 65, 96, 129, 300, 687]
S_PAD = 704


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("Sq", [2, 3])
def test_parity_at_128_heads_over_fill_levels_pages_and_splits(Sq, dtype, causal):
    H = 128
    q, kv = mc.make(len(FILLS), H, Sq, S_PAD, dtype, seed=H * 10 + Sq)
    rows = f8.F().quantize_mla_latent_fp8(kv)
    _, O, LSE, level = f8.reference(q, rows, FILLS, causal)
    for page in (32, 64, 128):
        pool, table = f8.scatter(rows, dtype, FILLS, page, mc.pages_of(S_PAD, page), seed=3)
        for n in (0, 1, 2, 3, 7):
            got = call(q, pool, FILLS, table, n, is_causal=causal)
            mc.held("fp8 parity H128 Sq%d %s causal%d page%d n%d" % (Sq, ids(dtype), causal, page, n), q, *got, O, LSE, FILLS, level)
            assert mc.same(got, call(q, pool, FILLS, table, n, is_causal=causal)), ("a repeated call gives other bits", page, n)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("Sq", [1, 2, 4])
def test_deep_table_at_three_tiles_per_page(Sq, dtype):
    """44 .. 49 tiles of keys after the append, ends at 5, 0, 17, 31, 1 and 0 keys into a tile: the steady state of the lookup
    pipeline with a division by three, and the pool byte for byte afterwards"""
    page, S = 96, 49 * 32
    after = [43 * 32 + 5, 45 * 32, 45 * 32 + 17, 46 * 32 + 31, 47 * 32 + 1, 49 * 32]
    assert [mc.pages_of(L, 32) for L in after] == [44, 45, 46, 47, 48, 49]
    fills = [L - Sq for L in after]
    q, kv = mc.make(len(after), 16, Sq, S, dtype, seed=31 + Sq)
    kv_new = torch.stack([kv[b, f:f + Sq] for b, f in enumerate(fills)])
    quant = lambda x: f8.F().quantize_mla_latent_fp8(x.cpu()).cuda()             # on the CPU: the bits the append writes
    rows = quant(kv)
    mp = mc.pages_of(S, page)
    pool, table = f8.scatter(rows, dtype, fills, page, mp, seed=9, alloc=after)
    want, _ = f8.scatter(rows, dtype, after, page, mp, seed=9)
    _, O, LSE, level = f8.reference(q, rows, after, True)
    for n in (0, 1):
        mine = pool.clone()
        o, lse = call(q, mine, fills, table, n, kv_new=kv_new, is_causal=True)
        mc.held("fp8 deep table Sq%d %s n%d" % (Sq, ids(dtype), n), q, o, lse, O, LSE, after, level)
        assert torch.equal(mine, want), ("bytes differ at", (mine != want).nonzero()[:4].tolist())


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_the_deepseek_scale(dtype):
    lens, scale = [33, 129, 300], 192 ** -0.5
    q, kv = mc.make(len(lens), 16, 2, 320, dtype, seed=95)
    rows = f8.F().quantize_mla_latent_fp8(kv)
    _, O, LSE, level = f8.reference(q, rows, lens, True, scale)
    pool, table = f8.scatter(rows, dtype, lens, 64, 5, seed=13)
    for n in (0, 3):
        o, lse = call(q, pool, lens, table, n, is_causal=True, softmax_scale=scale)
        mc.held("fp8 scale %.4f %s n%d" % (scale, ids(dtype), n), q, o, lse, O, LSE, lens, level)


def test_a_pool_beyond_4_gib_is_addressed_through_64_bit_page_bases():
    """the sequences' pages at the top of a 4.3 GB pool (uninitialised below them): the bits of the same step on a small pool,
    the appended bytes included"""
    page, mp, H, Sq = 64, 3, 16, 2
    lens = [63, 129]
    q, kv = mc.make(len(lens), H, Sq, mp * page, BF16, seed=85)
    new = torch.randn(len(lens), Sq, mc.D, generator=torch.Generator(device="cuda").manual_seed(86), device="cuda").to(BF16)
    small, table = f8.scatter(f8.F().quantize_mla_latent_fp8(kv), BF16, lens, page, mp, seed=21, alloc=[L + Sq for L in lens])
    n_big = (1 << 32) // (page * f8.ROW) + 40
    shift = n_big - small.shape[0]
    assert shift * page * f8.ROW > 1 << 32
    big = torch.empty(n_big, page, f8.ROW, dtype=torch.uint8, device="cuda")
    live = (table >= 0) & (table < small.shape[0])
    tbig = torch.where(live, table + shift, torch.full_like(table, -1))
    for n in (0, 3):
        big[shift:] = small
        ps = small.clone()
        want = call(q, ps, lens, table, n, kv_new=new, is_causal=True)
        got = call(q, big, lens, tbig, n, kv_new=new, is_causal=True)
        assert mc.same(want, got), n
        assert torch.equal(big[shift:], ps) and not torch.equal(ps, small)
    del big
    torch.cuda.empty_cache()


def test_captured_step_replays_while_seqlens_and_table_change_in_place():
    page, mp, H, Sq, B = 64, 3, 16, 1, 3
    q, kv = mc.make(B, H, Sq, mp * page, BF16, seed=97)
    new = torch.randn(B, Sq, mc.D, generator=torch.Generator(device="cuda").manual_seed(98), device="cuda").to(BF16)
    pool0, table = f8.scatter(f8.F().quantize_mla_latent_fp8(kv), BF16, [mp * page] * B, page, mp, seed=17)   # every page in use
    sl = torch.tensor([3, page - 1, 2 * page], dtype=torch.int32, device="cuda")
    pool = pool0.clone()
    step = lambda p: f8.F().flash_attention_mla_kvcache_fp8(q, p, sl, table, kv_new=new, is_causal=True, return_lse=True)
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
        assert torch.equal(pool, eager_pool) and not torch.equal(eager_pool, pool0)
        pool0 = eager_pool
