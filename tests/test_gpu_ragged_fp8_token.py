"""GPU tests of packed variable-length decoding over per-token-scaled e4m3 pools (fa_fwd_kvcache_fp8_token_ragged;
fp8_token_kvcache.flash_attention_kvcache_fp8_token_ragged), D = 64, 128 and 256.  The truth, the bounds and the helpers are
tests/fp8tokencheck.py's.  Shapes: B 4, H 8, H_kv 2, S_b from {1, 3, 9} (g * S_b = 36: two row blocks) with one sequence that
brings no query, fill levels of 1, 4, 5 and 9 tiles (D = 256, two tiles per step: 1, 2, 3 and 5), a length that is no
multiple of 32 and an empty cache, pages of 32 and 64 keys under a permuted table, forced splits 1, 2, 3 and the formula's."""
import pytest
import torch

import fp8tokencheck as tk
import pagedcheck as pc
import raggedcheck as rg
import variantcheck as vck
from fp8tokencheck import BF16, DT, F16, F8, IDS

pytestmark = pytest.mark.gpu

B, H, HKV, SC = 4, 8, 2, 320
LENS = {64: [32, 128, 160, 288], 128: [275, 0, 160, 288], 256: [32, 64, 96, 160]}
S = [9, 3, 1, 3]
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


def problem(D, dtype, seed, page, lens, S=S, alloc=None, **kw):
    """per-sequence queries qs[b] [1, H, S_b, D], the padded caches and scales c, and their pools under a permuted table"""
    Smax = max(S)
    q, *c = tk.make(B, H, HKV, Smax, SC, D, dtype, seed=seed, **kw)
    qs = [q[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)]
    n = sum(pc.pages_of(L, page) for L in (alloc or lens)) + 3
    pools = tk.scatter(*c, lens, page, n, SC // page, seed, alloc=alloc)
    return qs, c, pools


def check_each(tag, qs, res, c, lens, causal=True, window=(-1, -1), **kw):
    for b, (q, (o, lse)) in enumerate(zip(qs, res)):
        if q.shape[2]:
            tk.check("%s b%d" % (tag, b), q, o, lse, *(t[b:b + 1] for t in c), lens[b:b + 1], causal, window, **kw)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_matches_fp64_and_the_paged_call_sequence_by_sequence(D, dtype):
    lens, page = LENS[D], 32 if D == 64 else 64
    qs, c, (kp, vp, ksp, vsp, table) = problem(D, dtype, 3 + D, page, lens)
    sl = sl_of(lens)
    sinks = torch.tensor([0.5, -1.0, 3.0, 0.0, 8.0, -4.0, 1.5, 2.5], device="cuda")
    for i, (causal, window) in enumerate([(False, (-1, -1)), (True, (-1, -1)), (False, (40, 8))]):
        n = SPLITS[(i + D // 64) % 4]
        vck.splits(n)
        res = tk.packed(qs, kp, vp, ksp, vsp, sl, table, is_causal=causal, window_size=window)
        check_each("packed d%d n%d" % (D, n), qs, res, c, lens, causal, window)
        if D != 256:                                                            # the paged call on each sequence alone
            for b, q in enumerate(qs):
                one = tk.paged(q, kp, vp, ksp, vsp, sl[b:b + 1], table[b:b + 1], is_causal=causal, window_size=window)
                assert tk.same(res[b], one), ("packed = paged on the sequence alone", D, n, b, causal, window)
    vck.splits(2)
    res = tk.packed(qs, kp, vp, ksp, vsp, sl, table, is_causal=True, sinks=sinks, softmax_scale=0.07)
    check_each("packed sinks d%d" % D, qs, res, c, lens, True, (-1, -1), scale=0.07, sinks=sinks)
    plain = tk.packed(qs, kp, vp, ksp, vsp, sl, table, is_causal=True)
    minus = tk.packed(qs, kp, vp, ksp, vsp, sl, table, is_causal=True, sinks=torch.full((H,), float("-inf"), device="cuda"))
    assert all(tk.same(a, b) for a, b in zip(plain, minus))


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_a_sequence_without_queries_small_v_rows_and_padding_rows(dtype):
    D, page = 256, 64
    lens, S0 = [64, 288, 160, 96], [3, 0, 1, 9]
    qs, c, (kp, vp, ksp, vsp, table) = problem(D, dtype, 17, page, lens, S=S0,
                                               v_span={0: (-6.0, -6.0), 1: (4.0, 4.0), 2: (4.0, 4.0), 3: (4.0, 4.0)})
    for n in (1, 3):
        vck.splits(n)
        res = tk.packed(qs, kp, vp, ksp, vsp, sl_of(lens), table, total_q=sum(S0) + 5, is_causal=True)
        check_each("small rows d256 n%d" % n, qs, res, c, lens)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_unit_scales_give_the_bits_of_the_per_tensor_packed_kernel(D, dtype):
    import ragged_kvcache as R
    lens = LENS[D]
    qs, (k8, v8, ks, vs), _ = problem(D, dtype, 23, 64, lens, span=(-2.0, 0.0))
    k8.view(torch.uint8).bitwise_and_(0xBF)
    ones = torch.ones_like(ks)
    kp, vp, ksp, vsp, table = tk.scatter(k8, v8, ones, ones, lens, 64, 20, SC // 64, 9, fill_scale=1.0)
    sl, cu = sl_of(lens), rg.cu_of(S, device="cuda")
    qp = rg.pack(qs, sum(S), fill=0.0)
    for n in SPLITS:
        vck.splits(n)
        ref = R.flash_attention_kvcache_ragged(qp, kp, vp, cu, sl, table, is_causal=True, return_lse=True)
        got = tk.T().flash_attention_kvcache_fp8_token_ragged(qp, kp, vp, ksp, vsp, cu, sl, table, is_causal=True, return_lse=True)
        assert tk.same(got, ref), (D, n)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 256])
def test_packed_append_writes_the_quantisers_bytes_and_scale_bits(D, dtype):
    page = 32
    fills = [30, 126, 0, 150]                                                    # 30 + 9 rows cross a page edge
    lens = [f + s for f, s in zip(fills, S)]
    qs, (k8, v8, ks, vs), _ = problem(D, dtype, 29, page, fills, alloc=lens)
    g = torch.Generator(device="cuda").manual_seed(31)
    kn = [tk.rows((1, HKV, s, D), -6.0, 6.0, g).to(dtype) for s in S]
    vn = [tk.rows((1, HKV, s, D), -6.0, 6.0, g).to(dtype) for s in S]
    kn[1][0, 0, 0] = 0                                                          # an all-zero new row
    for b, f in enumerate(fills):
        k8.view(torch.uint8)[b, :, f:] = 0xFF
        v8.view(torch.uint8)[b, :, f:] = 0xFF
        ks[b, :, f:] = float("nan")
        vs[b, :, f:] = float("nan")
    bits = lambda t: t.view(torch.uint8) if t.dtype == F8 else t.view(torch.int32)
    want = [t.clone() for t in (k8, v8, ks, vs)]
    quant = lambda x: tuple(t.cuda() for t in tk.T().quantize_kv_fp8_per_token(x.cpu()))
    for b, f in enumerate(fills):
        (kq, kqs), (vq, vqs) = quant(kn[b]), quant(vn[b])
        for t, new in zip(want, (kq, vq, kqs, vqs)):
            t[b, :, f:f + S[b]] = new[0]
    n_pages = sum(pc.pages_of(L, page) for L in lens) + 3
    kp, vp, ksp, vsp, table = tk.scatter(k8, v8, ks, vs, fills, page, n_pages, SC // page, 7, alloc=lens)
    exp = tk.scatter(*want, lens, page, n_pages, SC // page, 7, alloc=lens)
    assert torch.equal(exp[4], table)
    # (scatter leaves the rows past lens[b] of a sequence's last page as the fill; the initial pools hold the poison there)
    for b, L in enumerate(lens):
        if L % page:
            pg = int(table[b, L // page])
            for e, t in zip(exp[:4], (kp, vp, ksp, vsp)):
                bits(e)[pg, :, L % page:] = bits(t)[pg, :, L % page:]
    for n in (1, 2):
        vck.splits(n)
        got = [t.clone() for t in (kp, vp, ksp, vsp)]
        res = tk.packed(qs, *got, sl_of(fills), table, k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        for name, a, w in zip(("k_pool", "v_pool", "k_scale", "v_scale"), got, exp[:4]):
            assert torch.equal(bits(a), bits(w)), (name, n, int((bits(a) != bits(w)).sum()))
        pre = tk.packed(qs, *exp[:4], sl_of(lens), table, is_causal=True)
        assert all(tk.same(a, b) for a, b in zip(res, pre)), n
        check_each("packed append d%d n%d" % (D, n), qs, res, want, lens)


def test_packed_graph_replays_after_everything_changes_in_place():
    D, dtype, page = 256, F16, 64
    qs, c, (kp, vp, ksp, vsp, table) = problem(D, dtype, 37, page, [SC] * B)
    sl, total = sl_of(LENS[D]), sum(S)
    cu = rg.cu_of(S, device="cuda")
    qp = rg.pack(qs, total, fill=0.0)
    call = lambda: tk.T().flash_attention_kvcache_fp8_token_ragged(qp, kp, vp, ksp, vsp, cu, sl, table, is_causal=True, return_lse=True)
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for lens, S1 in (([275, 0, 160, 288], [3, 9, 1, 3]), ([320, 1, 33, 64], [1, 1, 13, 1])):
        sl.copy_(sl_of(lens))
        cu.copy_(rg.cu_of(S1, device="cuda"))
        table.copy_(table.roll(1, 0))
        ksp.mul_(1.5)
        vsp.mul_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert tk.same(out, call()), lens
        cg = (pc.gather(kp, table), pc.gather(vp, table), tk.gather_scales(ksp, table), tk.gather_scales(vsp, table))
        q1 = rg.unpack(qp, S1)
        res = list(zip(rg.unpack(out[0], S1), rg.unpack_lse(out[1], S1)))
        check_each("packed replay", q1, res, cg, lens)
