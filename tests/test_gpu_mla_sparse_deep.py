"""Sparse (top-k indexed) MLA decoding, the structural pass: csrc/fa_decode_mla_sparse.hip writes out its own loop and its own
three-stage gather pipeline, so none of the dense kernel's structural tests (tests/test_gpu_mla.py) reach it.

Helpers, truth and bounds: tests/mlasparsecheck.py over tests/mlacheck.py, unchanged.  Every pool is mlacheck.scatter's: a
permuted table, NaN outside the live rows, out-of-range entries past a sequence's pages.  tests/test_host_mla_sparse.py holds
the conditions on the lists and the truths on the CPU.

A. One column group at a time under draw()'s lists of 70 entries (three tiles, the last partial): lens 65 / 300, S_q 2, the
   formula's split count and three.  Fails under: a quarter's pieces loaded from another wave's columns or written to another
   chunk of the V tile (latent quarter alone), a dropped or swapped RoPE slice (RoPE slice alone: LSE), a V tile or accumulator
   shared between waves (zero quarter), the RoPE piece reaching the V tile (RoPE no part of V).
B. The skip path `if (live == 0u) continue;`.  Lists by a per-tile pattern of live and dead tiles, every kind of invisible
   entry: one dead tile between live ones (the slot parity flips against t), two (kept), dead tiles first (the prologue loads
   them), the whole prologue dead, dead tiles in the steady state, alternating, trailing; at one split, at two and three (the
   boundaries of LDDL and LDDDDL lie inside dead runs), and at more splits than tiles (empty splits).  Fails under: slot parity
   taken from t instead of the steps taken (a race: the repeated call), a skipped tile that still counts into m / l, the
   pipeline registers not advanced on a skipped step (`continue` ahead of the three loads), a dead entry's page looked up.
   One visible entry in a list of 2048: O is that key's latent row bit for bit wherever in the list it stands.
C. Long lists (2048 and 2017 entries over 2100 keys: 64 tiles, the steady state of the pipeline and a partial last tile), pages
   of 96 and 160 keys (pdiv is a multiplication, not a shift: fails under `idx >> log2(page)`), every key of a tile in a
   96-key page of its own, DeepSeek's softmax scale, a pool beyond 4 GiB (fails under a 32-bit row address).
Shapes are the smallest that reach each path."""
import pytest
import torch

import mlacheck as mc
import mlasparsecheck as ms
import variantcheck as vck
from mlacheck import BF16, D, DV

pytestmark = pytest.mark.gpu

FILLS = [0, 1, 31, 33, 129, 300]
S_PAD = 320


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def ids(dtype):
    return mc.IDS[mc.DT.index(dtype)]


def call(q, pool, idx, lens, table, n=0, **kw):
    vck.splits(n)
    sl = lens if isinstance(lens, torch.Tensor) else torch.tensor(lens, dtype=torch.int32, device="cuda")
    return ms.S()(q, pool, idx, sl, table, return_lse=True, **kw)


# ---- A. one column group at a time ---------------------------------------------------------------------------------------------
def run_columns(tag, q, kv, idx, ns=(0, 3)):
    L = ms.COL_LENS
    ref = ms.reference(q, kv, idx, L, True)
    pool, table = mc.scatter(kv, L, ms.COL_PAGE, 5, 7)
    out = {}
    for n in ns:
        out[n] = call(q, pool, idx, L, table, n, is_causal=True)
        ms.held("sparse %s %s n%d" % (tag, ids(q.dtype), n), ref, out[n])
    return out


def quarter(w):
    inside = torch.zeros(DV, dtype=torch.bool, device="cuda")
    inside[128 * w:128 * w + 128] = True
    return inside


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("w", range(4))
def test_one_latent_quarter_alone(w, dtype):
    for n, (o, _) in run_columns("latent quarter %d" % w, *ms.column_problem("latent", w, dtype)).items():
        assert (o[..., ~quarter(w)] == 0).all() and (o[..., quarter(w)] != 0).any(), n


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("w", range(4))
def test_one_rope_slice_alone(w, dtype):
    """V is all zero: O = 0 exactly, the scores show in LSE alone (tests/test_host_mla_sparse.py: the slice moves it by > 0.05)"""
    for n, (o, _) in run_columns("rope slice %d" % w, *ms.column_problem("rope", w, dtype)).items():
        assert (o == 0).all(), n


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("w", range(4))
def test_a_zero_latent_quarter_of_the_cache_gives_a_zero_quarter_of_o(w, dtype):
    for n, (o, _) in run_columns("zero quarter %d" % w, *ms.column_problem("zero", w, dtype)).items():
        assert (o[..., quarter(w)] == 0).all() and (o[..., ~quarter(w)] != 0).any(), n


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_rope_columns_of_the_cache_are_no_part_of_v(dtype):
    q, kv, idx = ms.column_problem("ropev", 0, dtype)
    big = kv.clone()
    big[..., DV:] = (torch.randn_like(kv[..., DV:].float()) * 1000).to(dtype)
    kv[..., DV:] = 0
    got = run_columns("rope columns zero", q, kv, idx)
    pool, table = mc.scatter(big, ms.COL_LENS, ms.COL_PAGE, 5, 7)
    for n in got:
        assert mc.same(got[n], call(q, pool, idx, ms.COL_LENS, table, n, is_causal=True)), n


# ---- B. the skip path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("pattern", ms.PATTERNS)
def test_dead_tiles_are_passed_over_wherever_they_stand(pattern, dtype):
    L, page, mp, nt = ms.PAT_L, ms.PAT_PAGE, ms.PAT_MP, len(pattern)
    for Sq in (1, 3):
        q, kv = mc.make(1, 16, Sq, S_PAD, dtype, seed=len(pattern) * 10 + Sq)
        pool, table = mc.scatter(kv, [L], page, mp, 3)
        for k, kind in enumerate(ms.DEAD):
            if kind == "behind" and Sq == 1:
                continue                                   # a single query has no position behind it: the kind does not exist
            idx = ms.pattern_lists(L, Sq, pattern, kind, 50 + k, mp * page).cuda()
            ref = ms.reference(q, kv, idx, [L], True)
            for n in (1, 2, 3, nt + 2):
                got = call(q, pool, idx, [L], table, n, is_causal=True)
                ms.held("sparse skip %s %s Sq%d %s n%d" % (pattern, kind, Sq, ids(dtype), n), ref, got)
                assert mc.same(got, call(q, pool, idx, [L], table, n, is_causal=True)), ("a repeated call gives other bits", kind, Sq, n)


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_one_visible_entry_somewhere_in_a_list_of_2048(dtype):
    """every entry -1 but one, at list index 0, 31, 32, 1023 and 2047 (one sequence each): a one-key softmax gives the key's
    latent row back bit for bit"""
    where, topk, L, H = [0, 31, 32, 1023, 2047], 2048, 300, 16
    B = len(where)
    q, kv = mc.make(B, H, 1, S_PAD, dtype, seed=61)
    key = [17, 299, 0, 64, 191]
    idx = torch.full((B, 1, topk), -1, dtype=torch.int32)
    for b in range(B):
        idx[b, 0, where[b]] = key[b]
    idx = idx.cuda()
    pool, table = mc.scatter(kv, [L] * B, 64, 5, 3)
    ref = ms.reference(q, kv, idx, [L] * B, True)
    for n in (1, 0, 7):
        o, lse = call(q, pool, idx, [L] * B, table, n, is_causal=True)
        ms.held("sparse one entry %s n%d" % (ids(dtype), n), ref, (o, lse))
        if n == 1:
            want = torch.stack([kv[b, key[b], :DV] for b in range(B)])[:, None, None].expand(B, H, 1, DV)
            assert torch.equal(o.view(torch.int16), want.contiguous().view(torch.int16))


# ---- C. long lists, pages that are no powers of two, the scale, a large pool ----------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("topk", [2048, 2017])
def test_long_lists(topk, dtype):
    L, H = 2100, 16
    q, kv = mc.make(2, H, 1, 2112, dtype, seed=71)
    g = torch.Generator().manual_seed(72)
    idx = torch.stack([torch.randperm(L, generator=g)[:topk], torch.arange(L - 1, L - 1 - topk, -1)])[:, None].to(torch.int32).cuda()
    ref = ms.reference(q, kv, idx, [L, L], False)
    for page in (64, 160):
        pool, table = mc.scatter(kv, [L, L], page, mc.pages_of(L, page), 5)
        for n in (0, 1):
            ms.held("sparse long topk%d %s page%d n%d" % (topk, ids(dtype), page, n), ref, call(q, pool, idx, [L, L], table, n))


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("topk", [33, 160])
@pytest.mark.parametrize("page", [96, 160])
def test_pages_of_96_and_160_keys(page, topk, dtype):
    H, Sq = 16, 3
    q, kv = mc.make(len(FILLS), H, Sq, S_PAD, dtype, seed=page + topk)
    idx = ms.draw(FILLS, Sq, topk, seed=topk + Sq).cuda()
    pool, table = mc.scatter(kv, FILLS, page, mc.pages_of(S_PAD, page), 3)
    for causal in (False, True):
        ref = ms.reference(q, kv, idx, FILLS, causal)
        for n in (0, 3):
            got = call(q, pool, idx, FILLS, table, n, is_causal=causal)
            ms.held("sparse page%d topk%d %s causal%d n%d" % (page, topk, ids(dtype), causal, n), ref, got)


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_every_key_of_a_tile_in_a_96_key_page_of_its_own(dtype):
    """64 entries a page apart and a different row in each page, ascending in sequence 0 and descending in sequence 1"""
    page, topk, H = 96, 64, 16
    lens = [topk * page + 1] * 2
    q, kv = mc.make(2, H, 1, 65 * page, dtype, seed=31)
    up = torch.arange(topk, dtype=torch.int32) * page + (torch.arange(topk, dtype=torch.int32) * 7) % page
    idx = torch.stack([up, up.flip(0)])[:, None].cuda()
    pool, table = mc.scatter(kv, lens, page, 65, 5)
    ref = ms.reference(q, kv, idx, lens, False)
    for n in (1, 2):
        ms.held("sparse own-page96 %s n%d" % (ids(dtype), n), ref, call(q, pool, idx, lens, table, n))


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_the_deepseek_scale(dtype):
    lens, scale = [33, 129, 300], 192 ** -0.5
    q, kv = mc.make(len(lens), 16, 2, 320, dtype, seed=95)
    idx = ms.draw(lens, 2, 70, seed=96).cuda()
    ref = ms.reference(q, kv, idx, lens, True, scale)
    pool, table = mc.scatter(kv, lens, 64, 5, 13)
    for n in (0, 3):
        ms.held("sparse scale %.4f %s n%d" % (scale, ids(dtype), n), ref,
                call(q, pool, idx, lens, table, n, is_causal=True, softmax_scale=scale))


def test_a_pool_beyond_4_gib_is_addressed_through_64_bit_row_addresses():
    """the sequences' pages at the top of a 4.3 GB pool (uninitialised below them), lists that name their rows and the appended
    ones: the bits of the same step on a small pool, the appended rows included"""
    page, mp, H, Sq, topk = 64, 3, 16, 2, 70
    lens = [63, 129]
    after = [L + Sq for L in lens]
    q, kv = mc.make(len(lens), H, Sq, mp * page, BF16, seed=85)
    new = torch.randn(len(lens), Sq, D, generator=torch.Generator(device="cuda").manual_seed(86), device="cuda").to(BF16)
    idx = torch.stack([ms.draw([L], Sq, topk, seed=b, lead=(L - 1, L - 2))[0] for b, L in enumerate(after)]).cuda()
    small, table = mc.scatter(kv, lens, page, mp, 21, alloc=after)
    n_big = (1 << 32) // (page * D * 2) + 40
    shift = n_big - small.shape[0]
    assert shift * page * D * 2 > 1 << 32
    big = torch.empty(n_big, page, D, dtype=BF16, device="cuda")
    live = (table >= 0) & (table < small.shape[0])
    tbig = torch.where(live, table + shift, torch.full_like(table, -1))
    for n in (0, 3):
        big[shift:] = small
        ps = small.clone()
        want = call(q, ps, idx, lens, table, n, kv_new=new, is_causal=True)
        got = call(q, big, idx, lens, tbig, n, kv_new=new, is_causal=True)
        assert mc.same(want, got), n
        assert torch.equal(big[shift:].view(torch.int16), ps.view(torch.int16)) and not torch.equal(ps.view(torch.int16), small.view(torch.int16))
    del big
    torch.cuda.empty_cache()
