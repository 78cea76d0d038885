"""GPU tests of soft-capped decoding over the quantised KV caches (include_quant/mi355fa_kvcache_quant_softcap.h;
quant_softcap_kvcache.py), padded and paged; tests/test_gpu_ragged_quant_softcap.py has the packed call.  The truth is fp64
attention with the cap on the fp64 dequantised cache (tests/quantcapcheck.py), so quantisation error is not in the comparison;
every (sequence, head) of O is held on its own to 1e-3 fp16 / 8e-3 bf16, LSE row by row, and O must be at least CAP_MATTERS from
the uncapped attention on the sequences with at least 300 keys.

Shapes (tests/variantcheck.py decode_case's, on a cache of whole tiles): B 3, H 8 / H_kv 2 and H 6 / H_kv 2 (an odd group), S_q 1,
2 and 11 (g x S_q = 44: two 32-row blocks, the second partial), a 704-row cache at fill levels 0 / 300 / 650 with 2 appended keys,
forced split counts 0 (the formula) / 1 / 3 / 7, no mask, causal and the window (100, 0), caps 15 / 30 / 50, pages of 32, 96 and
128 keys under a permuted table and one table of 45 tiles at 3 tiles per page, D 64 / 128 and, per-tensor e4m3, 256."""
import pytest
import torch

import quantcapcheck as qc
import variantcheck as vck
from quantcapcheck import BF16, DT, F16, FORMATS, IDS

pytestmark = pytest.mark.gpu

B, SC, SNEW = 3, 704, 2
FILLS = [0, 300, 650]
LENS = [f + SNEW for f in FILLS]
NOMASK, CAUSAL, WINDOW = (False, (-1, -1)), (True, (-1, -1)), (False, (100, 0))
# (S_q, H, H_kv, mask, cap, forced splits): every value of each at least once, the two row blocks under every mask
COMBOS = [(1, 8, 2, NOMASK, 50.0, 0), (2, 6, 2, CAUSAL, 30.0, 1), (11, 8, 2, WINDOW, 15.0, 3), (11, 6, 2, CAUSAL, 50.0, 7),
          (11, 8, 2, NOMASK, 30.0, 0), (1, 6, 2, WINDOW, 15.0, 7)]
FMT_D = [(f, D) for f in FORMATS for D in ((64, 128, 256) if f == "e4m3" else (64, 128))]
FMT_D_IDS = ["%s-d%d" % fd for fd in FMT_D]


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def step(fmt, Sq, H, Hkv, D, dtype, cap, seed, **kw):
    """q, the cache before the step, k_new / v_new, and the cache after it as the PLAIN call of the format appends them"""
    q, c = qc.make(fmt, B, H, Hkv, Sq, SC, D, dtype, cap, seed=seed, **kw)
    kn, vn = qc.new_rows(B, Hkv, SNEW, D, dtype, seed + 1)
    after = c.clone()
    vck.splits(1)
    qc.plain_padded(q, after, qc.sl_of(FILLS), k_new=kn, v_new=vn)
    return q, c, kn, vn, after


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("fmt,D", FMT_D, ids=FMT_D_IDS)
def test_matches_fp64_per_sequence_and_head(fmt, D, dtype):
    sl = qc.sl_of(FILLS)
    for i, (Sq, H, Hkv, (causal, window), cap, n) in enumerate(COMBOS):
        q, c, kn, vn, after = step(fmt, Sq, H, Hkv, D, dtype, cap, seed=100 * D + i)
        gt = qc.truth(q, after, LENS, cap, causal, window)
        vck.splits(n)
        runs = []
        for _ in range(2):
            got = c.clone()
            runs.append(qc.padded(q, got, sl, cap, k_new=kn, v_new=vn, is_causal=causal, window_size=window))
            for name, a, w in zip(("k", "v", "k_scale", "v_scale"), got.tensors(), after.tensors()):
                assert torch.equal(qc.bits(a), qc.bits(w)), ("the appended rows have the plain call's bits", name, i)
        assert qc.same(*runs), ("two launches, the same bits", i)
        qc.check("%s d%d combo %d" % (fmt, D, i), q, *runs[0], gt, LENS)
        pre = qc.padded(q, after, qc.sl_of(LENS), cap, is_causal=causal, window_size=window)
        assert qc.same(runs[0], pre), ("the step equals the call without append on the pre-filled cache", i)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("kind", ["natural", "times3", "per_head"])
def test_k_descale_goes_under_the_tanh(kind, D, dtype):
    """distinct per-(B, H_kv) descales of about 0.01 (amax / 448), the same times 3, and one (H_kv,) vector: a kernel that leaves
    k_descale out of the capped coefficient, or applies it behind the tanh, fails all three"""
    kw = dict(descale_mul=3.0) if kind == "times3" else dict(per_head=True) if kind == "per_head" else {}
    cap, Sq, H, Hkv = 30.0, 2, 8, 2
    q, c = qc.make("e4m3", B, H, Hkv, Sq, SC, D, dtype, cap, seed=7 + D, **kw)
    assert c.kd.shape == ((Hkv,) if kind == "per_head" else (B, Hkv))
    lens = [2, 302, 652]
    pools, table = qc.scatter(c, lens, 32, SC // 32)
    for n, (causal, window) in ((1, NOMASK), (3, CAUSAL)):
        vck.splits(n)
        gt = qc.truth(q, c, lens, cap, causal, window)
        o, lse = qc.padded(q, c, qc.sl_of(lens), cap, is_causal=causal, window_size=window)
        qc.check("k_descale %s d%d n%d" % (kind, D, n), q, o, lse, gt, lens)
        assert qc.same(qc.paged(q, pools, qc.sl_of(lens), table, cap, is_causal=causal, window_size=window), (o, lse)), n


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_per_token_scales_spanning_twelve_octaves(D, dtype):
    """rows with amax 2^-6 .. 2^6 (fp8tokencheck.make), against the truth only; and with every row scale 1.0 the bits of the
    per-tensor call with NULL descales"""
    import fp8tokencheck as tk
    cap, Sq, H, Hkv = 30.0, 2, 8, 2
    lens = [2, 302, 652]
    sl = qc.sl_of(lens)
    q, k8, v8, ks, vs = tk.make(B, H, Hkv, Sq, SC, D, dtype, seed=D)
    c = qc.Cache("token", k8, v8, ks, vs)
    ones = qc.Cache("token", k8, v8, torch.ones_like(ks), torch.ones_like(vs))
    flat = qc.Cache("e4m3", k8, v8)
    for n, (causal, window) in ((0, NOMASK), (1, CAUSAL), (3, WINDOW), (7, CAUSAL)):
        vck.splits(n)
        o, lse = qc.padded(q, c, sl, cap, is_causal=causal, window_size=window)
        qc.check("token span d%d n%d" % (D, n), q, o, lse, qc.truth(q, c, lens, cap, causal, window), lens, matters=False)
        assert qc.same(qc.padded(q, ones, sl, cap, is_causal=causal, window_size=window),
                       qc.padded(q, flat, sl, cap, is_causal=causal, window_size=window)), ("unit scales", n)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("fmt,D", FMT_D, ids=FMT_D_IDS)
@pytest.mark.parametrize("page", [32, 96, 128])
def test_paged_has_the_bits_of_the_padded_call_on_the_gathered_cache(page, fmt, D, dtype):
    cap, Sq, H, Hkv = 50.0, 11, 6, 2
    mp = -(-SC // page)
    q, c = qc.make(fmt, B, H, Hkv, Sq, SC, D, dtype, cap, seed=page + D)
    pools, table = qc.scatter(c, LENS, page, mp, seed=page)
    flat = qc.gather(pools, table)
    sl = qc.sl_of(LENS)
    gt = qc.truth(q, c, LENS, cap, True)
    for n in (0, 1, 3, 7):
        vck.splits(n)
        o, lse = qc.paged(q, pools, sl, table, cap, is_causal=True)
        assert qc.same((o, lse), qc.padded(q, flat, sl, cap, is_causal=True)), (page, n)
        if n in (0, 3):
            qc.check("paged %s d%d page %d n%d" % (fmt, D, page, n), q, o, lse, gt, LENS)


@pytest.mark.parametrize("fmt,D,dtype", [("e4m3", 256, BF16), ("e4m3", 64, F16), ("token", 128, F16), ("fp4", 128, BF16), ("fp4", 64, F16)])
def test_deep_table_of_45_tiles_at_3_tiles_per_page(fmt, D, dtype):
    """the steady state of the table lookup pipeline: 15 pages of 96 keys per sequence, every split over many pages"""
    cap, Sq, H, Hkv, page, mp = 30.0, 2, 8, 2, 96, 15
    lens = [1440, 1, 1345]
    q, c = qc.make(fmt, B, H, Hkv, Sq, mp * page, D, dtype, cap, seed=D)
    pools, table = qc.scatter(c, lens, page, mp, seed=9)
    flat = qc.gather(pools, table)
    sl = qc.sl_of(lens)
    for n, (causal, window) in ((1, NOMASK), (3, WINDOW), (0, CAUSAL)):
        vck.splits(n)
        o, lse = qc.paged(q, pools, sl, table, cap, is_causal=causal, window_size=window)
        qc.check("deep %s d%d n%d" % (fmt, D, n), q, o, lse, qc.truth(q, c, lens, cap, causal, window), lens, matters=window == (-1, -1))
        assert qc.same((o, lse), qc.padded(q, flat, sl, cap, is_causal=causal, window_size=window)), n


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_paged_append_writes_the_plain_calls_bits(fmt, dtype):
    """the pools after a capped paged step hold the bytes (and scales) the format's plain paged call appends; the two new rows of
    sequence 0 (fill 31) straddle a page of 32 keys"""
    cap, Sq, H, Hkv, D, page = 30.0, 2, 8, 2, 128, 32
    fills = [31, 300, 650]
    lens = [f + SNEW for f in fills]
    q, c = qc.make(fmt, B, H, Hkv, Sq, SC, D, dtype, cap, seed=3)
    kn, vn = qc.new_rows(B, Hkv, SNEW, D, dtype, 4)
    pools, table = qc.scatter(c, fills, page, SC // page, seed=2, alloc=lens)
    want = pools.clone()
    vck.splits(1)
    qc.plain_paged(q, want, qc.sl_of(fills), table, k_new=kn, v_new=vn, is_causal=True)
    for n in (1, 3):
        vck.splits(n)
        got = pools.clone()
        o, lse = qc.paged(q, got, qc.sl_of(fills), table, cap, k_new=kn, v_new=vn, is_causal=True)
        for name, a, w in zip(("k", "v", "k_scale", "v_scale"), got.tensors(), want.tensors()):
            assert torch.equal(qc.bits(a), qc.bits(w)), (name, n)
        after = qc.gather(want, table)
        qc.check("paged append %s n%d" % (fmt, n), q, o, lse, qc.truth(q, after, lens, cap, True), lens)


@pytest.mark.parametrize("geometry", ["padded", "paged"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_graph_captured_step_replays_after_lengths_and_table_change(fmt, geometry):
    cap, Sq, H, Hkv, D, dtype, page = 50.0, 1, 8, 2, 128, BF16, 64
    q, c = qc.make(fmt, B, H, Hkv, Sq, SC, D, dtype, cap, seed=11)
    pools, table = qc.scatter(c, [SC] * B, page, SC // page, seed=4)
    sl = qc.sl_of([300, 650, 2])
    if geometry == "padded":
        call = lambda: qc.padded(q, c, sl, cap, is_causal=True)
    else:
        call = lambda: qc.paged(q, pools, sl, table, cap, is_causal=True)
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for lens in ([652, 0, 302], [33, 704, 64]):
        sl.copy_(qc.sl_of(lens))
        if geometry == "paged":
            table.copy_(table.roll(1, 0))                                       # every sequence now reads another one's pages
        graph.replay()
        torch.cuda.synchronize()
        assert qc.same(out, call()), lens
        now = c if geometry == "padded" else qc.gather(pools, table)
        qc.check("replay %s %s" % (fmt, geometry), q, *out, qc.truth(q, now, lens, cap, True), lens)
