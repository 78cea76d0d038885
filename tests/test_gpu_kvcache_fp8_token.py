"""GPU tests of decoding attention over an e4m3 KV cache with one fp32 scale per cached token and K/V head
(include/mi355fa_kvcache_fp8_token.h; fp8_token_kvcache.py), padded and paged; tests/test_gpu_ragged_fp8_token.py has the packed
call.  The truth is fp64 attention on the fp64 dequantised cache, float(byte) * scale, so quantisation error is not in the
comparison; every (sequence, head) of O is held on its own to the bounds of tests/test_gpu_kvcache_fp8.py's per-head test
(fp8tokencheck.BOUND) and LSE to its check_lse.

Shapes: B 4, H 8, H_kv 2 (and MQA once), S_q 1, 3 and 9 (g * S_q = 36: two row blocks), fill levels of 1, 4, 5 and 9 tiles of 32
keys, one length that is no multiple of 32 and one empty sequence, pages of 32 and 64 keys under a permuted table, forced splits
1, 2, 3 and the formula's count.  Tables past 9 tiles, other page sizes and strided pools: tests/test_gpu_fp8_token_deep.py."""
import pytest
import torch

import fp8tokencheck as tk
import pagedcheck as pc
import variantcheck as vck
from fp8tokencheck import BF16, DT, F16, F8, IDS

pytestmark = pytest.mark.gpu

B, H, HKV, SC = 4, 8, 2, 320
TILES = [32, 128, 160, 288]          # 1, 4, 5 and 9 tiles
ODD = [275, 0, 160, 128]             # a length that is no multiple of 32, an empty sequence
MASKS = [(False, (-1, -1)), (True, (-1, -1)), (False, (40, 8))]
SPLITS = (1, 2, 3, 0)


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def _M():
    import My_FlashAttention_optimized as M
    return M


def sl_of(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")


def paged_of(c, lens, page, seed=5, alloc=None):
    """(kp, vp, ksp, vsp, table) of the padded caches and scales c = (k8, v8, ks, vs)"""
    mp = SC // page
    n = sum(pc.pages_of(L, page) for L in (alloc or lens)) + 3
    return tk.scatter(*c, lens, page, n, mp, seed, alloc=alloc)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq", [1, 3, 9])
def test_matches_fp64_per_sequence_and_head(Sq, D, dtype):
    lens = ODD if Sq == 3 else TILES
    q, *c = tk.make(B, H, HKV, Sq, SC, D, dtype, seed=Sq + D)
    sl = sl_of(lens)
    pools = paged_of(c, lens, 32 if Sq == 9 else 64)
    for i, (causal, window) in enumerate(MASKS):
        n = SPLITS[(i + Sq) % 4]
        vck.splits(n)
        o, lse = tk.padded(q, *c, sl, is_causal=causal, window_size=window)
        tk.check("padded n%d %s" % (n, (causal, window)), q, o, lse, *c, lens, causal, window)
        po, plse = tk.paged(q, *pools[:4], sl, pools[4], is_causal=causal, window_size=window)
        assert tk.same((po, plse), (o, lse)), ("paged = padded on the gathered cache", n, causal, window)
        if 0 in lens:
            assert (o[lens.index(0)] == 0).all() and torch.isneginf(lse[lens.index(0)]).all()


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_mqa_softmax_scale_and_sinks(dtype):
    D, Sq = 128, 3
    q, *c = tk.make(B, H, 1, Sq, SC, D, dtype, seed=11)
    sl = sl_of(ODD)
    o, lse = tk.padded(q, *c, sl, is_causal=True, softmax_scale=0.05)
    tk.check("mqa scale", q, o, lse, *c, ODD, True, (-1, -1), scale=0.05)
    sinks = torch.tensor([0.5, -1.0, 3.0, 0.0, 8.0, -4.0, 1.5, 2.5], device="cuda")
    pools = paged_of(c, ODD, 64)
    for n in (1, 3):
        vck.splits(n)
        so, slse = tk.padded(q, *c, sl, is_causal=True, sinks=sinks)
        tk.check("sinks n%d" % n, q, so, slse, *c, ODD, True, (-1, -1), sinks=sinks)
        assert tk.same(tk.paged(q, *pools[:4], sl, pools[4], is_causal=True, sinks=sinks), (so, slse))
        plain = tk.padded(q, *c, sl, is_causal=True)
        assert tk.same(tk.padded(q, *c, sl, is_causal=True, sinks=torch.full((H,), float("-inf"), device="cuda")), plain), n


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("L", [64, 288])
def test_small_v_rows_keep_their_precision(L, dtype):
    """sequence 1's V rows all have amax 2^-6 (v_scale ~ 2^-14.8), the others 2^4: a kernel that folds v_scale into the fp16
    probabilities loses sequence 1"""
    D, Sq = 128, 3
    lens = [L, L, 160, 288]
    q, *c = tk.make(B, H, HKV, Sq, SC, D, dtype, seed=L, v_span={0: (4.0, 4.0), 1: (-6.0, -6.0), 2: (4.0, 4.0), 3: (4.0, 4.0)})
    assert float(c[3][1].max()) < 2.0 ** -14 and float(c[3][0].min()) > 2.0 ** -5
    for n in (1, 2):
        vck.splits(n)
        o, lse = tk.padded(q, *c, sl_of(lens))
        tk.check("small rows n%d" % n, q, o, lse, *c, lens)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_unit_scales_give_the_bits_of_the_per_tensor_kernel(D, dtype):
    Sq, lens = 3, ODD
    q, k8, v8, ks, vs = tk.make(B, H, HKV, Sq, SC, D, dtype, seed=21, span=(-2.0, 0.0))
    k8.view(torch.uint8).bitwise_and_(0xBF)                                      # |k| < 2 as values: moderate scores
    ones = torch.ones_like(ks)
    sl = sl_of(lens)
    pools = paged_of((k8, v8, ones, ones), lens, 64)
    for n in SPLITS:
        vck.splits(n)
        ref = _M().flash_attention_kvcache_fp8(q, k8, v8, sl, is_causal=True, return_lse=True)
        assert tk.same(tk.padded(q, k8, v8, ones, ones, sl, is_causal=True), ref), ("padded", n)
        assert tk.same(tk.paged(q, *pools[:4], sl, pools[4], is_causal=True), ref), ("paged", n)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_transposed_cache_and_scales_are_read_in_place(dtype):
    D, Sq = 64, 3
    q, k8, v8, ks, vs = tk.make(B, H, HKV, Sq, SC, D, dtype, seed=31)
    sl = sl_of(TILES)
    tr = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)                # [B, S, H_kv, ..] storage
    kt, vt, kst, vst = tr(k8), tr(v8), tr(ks), tr(vs)
    assert not kt.is_contiguous() and not kst.is_contiguous() and kst.stride(2) == HKV
    for n in (1, 3):
        vck.splits(n)
        assert tk.same(tk.padded(q, kt, vt, kst, vst, sl, is_causal=True), tk.padded(q, k8, v8, ks, vs, sl, is_causal=True)), n


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("page", [32, 64])
def test_rows_past_the_fill_level_and_unnamed_pages_are_never_read(page, dtype):
    D, Sq, lens = 128, 3, ODD
    q, k8, v8, ks, vs = tk.make(B, H, HKV, Sq, SC, D, dtype, seed=41)
    sl = sl_of(lens)
    clean = {}
    for n in (1, 2):
        vck.splits(n)
        clean[n] = tk.padded(q, k8, v8, ks, vs, sl)
    for b, L in enumerate(lens):
        k8.view(torch.uint8)[b, :, L:] = 0xFF
        v8.view(torch.uint8)[b, :, L:] = 0xFF
        ks[b, :, L:] = float("nan")
        vs[b, :, L:] = float("nan")
    for n in (1, 2):
        vck.splits(n)
        base = tk.padded(q, k8, v8, ks, vs, sl)
        assert torch.isfinite(base[0]).all() and tk.same(base, clean[n]), n
        kp, vp, ksp, vsp, table = paged_of((k8, v8, ks, vs), lens, page)
        kp.view(torch.uint8)[pc.unused_pages(table, lens, page, kp.shape[0])] = 0xFF
        for b, L in enumerate(lens):                                             # the tail of each sequence's last page
            if L % page:
                pg = int(table[b, L // page])
                kp.view(torch.uint8)[pg, :, L % page:] = 0xFF
                vp.view(torch.uint8)[pg, :, L % page:] = 0xFF
        assert tk.same(tk.paged(q, kp, vp, ksp, vsp, sl, table), base), n


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Snew", [1, 3])
def test_append_writes_the_quantisers_bytes_and_scale_bits(Snew, D, dtype):
    Sq, page = Snew, 32
    fills = [31, 126, 0, 285]                                                    # 31 + 3 and 126 + 3 cross a page edge
    lens = [f + Snew for f in fills]
    q, k8, v8, ks, vs = tk.make(B, H, HKV, Sq, SC, D, dtype, seed=51 + Snew)
    g = torch.Generator(device="cuda").manual_seed(61)
    kn = tk.rows((B, HKV, Snew, D), -6.0, 6.0, g).to(dtype)
    vn = tk.rows((B, HKV, Snew, D), -6.0, 6.0, g).to(dtype)
    kn[1, 0, 0] = 0                                                              # an all-zero new row
    vn[2, 1, -1] = 0
    (kq, kqs), (vq, vqs) = (tuple(t.cuda() for t in tk.T().quantize_kv_fp8_per_token(x.cpu())) for x in (kn, vn))   # on the CPU
    assert float(kqs[1, 0, 0]) == 1.0 and (kq[1, 0, 0].view(torch.uint8) == 0).all()
    for b, f in enumerate(fills):                                                # poison at and past the fill level
        k8.view(torch.uint8)[b, :, f:] = 0xFF
        v8.view(torch.uint8)[b, :, f:] = 0xFF
        ks[b, :, f:] = float("nan")
        vs[b, :, f:] = float("nan")
    want = [t.clone() for t in (k8, v8, ks, vs)]
    for b, f in enumerate(fills):
        for t, new in zip(want, (kq, vq, kqs, vqs)):
            t[b, :, f:f + Snew] = new[b]
    bits = lambda t: t.view(torch.uint8) if t.dtype == F8 else t.view(torch.int32)
    sl = sl_of(fills)
    for n in (1, 2):
        vck.splits(n)
        got = [t.clone() for t in (k8, v8, ks, vs)]
        res = tk.padded(q, *got, sl, k_new=kn, v_new=vn, is_causal=True)
        for name, a, w in zip(("k_cache", "v_cache", "k_scale", "v_scale"), got, want):
            assert torch.equal(bits(a), bits(w)), ("padded", name, n, int((bits(a) != bits(w)).sum()))
        pre = tk.padded(q, *want, sl_of(lens), is_causal=True)
        assert tk.same(res, pre), ("the step equals the call without append on the pre-filled cache", n)
        tk.check("append n%d" % n, q, *res, *want, lens, True)
        # paged: the same rows through the table; sequence 3's last entry is outside the pool, so its rows there are dropped
        kp, vp, ksp, vsp, table = paged_of((k8, v8, ks, vs), fills, page, alloc=lens)
        table[3, (lens[3] - 1) // page] = kp.shape[0] + 7
        exp = [t.clone() for t in (kp, vp, ksp, vsp)]
        for bb, f in enumerate(fills):
            for j in range(Snew):
                pg = int(table[bb, (f + j) // page])
                if 0 <= pg < kp.shape[0]:
                    for t, new in zip(exp, (kq, vq, kqs, vqs)):
                        bits(t)[pg, :, (f + j) % page] = bits(new)[bb, :, j]
        big = [pc.guarded(t, 2) for t in (kp, vp)]
        sbig = [torch.full((t.shape[0] + 4, *t.shape[1:]), float("nan"), device="cuda") for t in (ksp, vsp)]
        for sb, t in zip(sbig, (ksp, vsp)):
            sb[2:-2] = t
        views = [big[0][1], big[1][1], sbig[0][2:-2], sbig[1][2:-2]]
        pres = tk.paged(q, *views, sl, table, k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        assert pc.guards_intact(big[0][0], 2) and pc.guards_intact(big[1][0], 2)
        assert all(torch.isnan(sb[:2]).all() and torch.isnan(sb[-2:]).all() for sb in sbig)
        for name, a, w in zip(("k_pool", "v_pool", "k_scale", "v_scale"), views, exp):
            assert torch.equal(bits(a), bits(w)), ("paged", name, n, int((bits(a) != bits(w)).sum()))
        for bb in range(3):                                                      # the sequences whose rows all landed
            assert tk.same((pres[0][bb:bb + 1], pres[1][bb:bb + 1]), (res[0][bb:bb + 1], res[1][bb:bb + 1])), ("paged step", n, bb)


def test_graph_captured_step_replays_after_lengths_table_and_scales_change():
    D, Sq, dtype, page = 128, 1, BF16, 64
    q, *c = tk.make(B, H, HKV, Sq, SC, D, dtype, seed=71)
    kp, vp, ksp, vsp, table = paged_of(c, [SC] * B, page)
    sl = sl_of(TILES)
    call = lambda: tk.paged(q, kp, vp, ksp, vsp, sl, table, is_causal=True)
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for step, lens in enumerate((ODD, [320, 1, 33, 64])):
        sl.copy_(sl_of(lens))
        table.copy_(table.roll(1, 0))                                           # every sequence now reads another one's pages
        ksp.mul_(1.5)
        vsp.mul_(0.75 if step else 3.0)
        graph.replay()
        torch.cuda.synchronize()
        eager = call()
        assert tk.same(out, eager), lens
        Kg, Vg = pc.gather(kp, table), pc.gather(vp, table)
        tk.check("replay %d" % step, q, *out, Kg, Vg, tk.gather_scales(ksp, table), tk.gather_scales(vsp, table), lens, True)
