"""GPU tests of soft-capped packed variable-length decoding over the quantised pools (fa_fwd_kvcache_quant_softcap_ragged;
quant_softcap_kvcache.flash_attention_kvcache_quant_softcap_ragged), D = 64, 128 and 256 in all three formats.  The truth, the
bounds and the helpers are tests/quantcapcheck.py's.  Shapes: B 5 with S_b = [1, 0, 5, 11, 40] (g x 11 = 44 and g x 40 = 160 rows:
two and five row blocks, one sequence that brings no query) and padding rows past cu[B], H 8 / H_kv 2 and H 6 / H_kv 2, key counts
302 / 64 / 652 / 2 / 704 in a 704-row cache, pages of 32 keys under a permuted table, forced splits 0 / 1 / 3 / 7, no mask, causal
and the window (100, 0), caps 15 / 30 / 50."""
import pytest
import torch

import quantcapcheck as qc
import raggedcheck as rg
import variantcheck as vck
from quantcapcheck import BF16, DT, F16, FORMATS, IDS

pytestmark = pytest.mark.gpu

B, SC, PAGE = 5, 704, 32
S = [1, 0, 5, 11, 40]
LENS = [302, 64, 652, 2, 704]
PAD = 3                                  # rows past cu[B]
NOMASK, CAUSAL, WINDOW = (False, (-1, -1)), (True, (-1, -1)), (False, (100, 0))
COMBOS = [(8, NOMASK, 50.0, 0), (6, CAUSAL, 30.0, 3), (8, WINDOW, 15.0, 7), (6, CAUSAL, 15.0, 1)]
FMT_D = [(f, D) for f in FORMATS for D in (64, 128, 256)]
FMT_D_IDS = ["%s-d%d" % fd for fd in FMT_D]


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def problem(fmt, H, D, dtype, cap, seed, lens=LENS, S=S, alloc=None):
    """per-sequence queries qs[b] [1, H, S_b, D], the padded cache c and its pools under a permuted table"""
    q, c = qc.make(fmt, B, H, 2, max(S), SC, D, dtype, cap, seed=seed)
    qs = [q[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)]
    pools, table = qc.scatter(c, lens, PAGE, SC // PAGE, seed=seed, alloc=alloc)
    return qs, c, pools, table


def check_each(tag, qs, res, c, lens, cap, causal, window):
    for b, (q, (o, lse)) in enumerate(zip(qs, res)):
        if q.shape[2]:
            one = c.rows(b, c.k.shape[2])
            qc.check("%s b%d" % (tag, b), q, o, lse, qc.truth(q, one, lens[b:b + 1], cap, causal, window), lens[b:b + 1])


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("fmt,D", FMT_D, ids=FMT_D_IDS)
def test_matches_fp64_and_the_paged_call_sequence_by_sequence(fmt, D, dtype):
    sl = qc.sl_of(LENS)
    for i, (H, (causal, window), cap, n) in enumerate(COMBOS):
        qs, c, pools, table = problem(fmt, H, D, dtype, cap, 10 * D + i)
        vck.splits(n)
        res = qc.packed(qs, pools, sl, table, cap, total_q=sum(S) + PAD, is_causal=causal, window_size=window)
        again = qc.packed(qs, pools, sl, table, cap, total_q=sum(S) + PAD, is_causal=causal, window_size=window)
        assert all(qc.same(a, b) for a, b in zip(res, again)), ("two launches, the same bits", i)
        check_each("packed %s d%d combo %d" % (fmt, D, i), qs, res, c, LENS, cap, causal, window)
        if D != 256:                                                            # the paged call on each sequence alone
            for b, q in enumerate(qs):
                if q.shape[2]:
                    one = qc.paged(q, pools.for_seq(b), sl[b:b + 1], table[b:b + 1], cap, is_causal=causal, window_size=window)
                    assert qc.same(res[b], one), ("packed = paged on the sequence alone", fmt, D, n, b)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("fmt,D", [("e4m3", 256), ("token", 64), ("fp4", 256), ("fp4", 128), ("token", 256)])
def test_packed_append_writes_the_plain_calls_bits_and_out_is_written_in_place(fmt, D, dtype):
    cap, H = 30.0, 8
    fills = [L - s for L, s in zip(LENS, S)]                                     # 704 - 40 + 40 ends on the table's last row
    fills[3] = 30                                                                # 30 + 11 rows cross a page edge
    lens = [f + s for f, s in zip(fills, S)]
    qs, c, pools, table = problem(fmt, H, D, dtype, cap, 5 + D, lens=fills, alloc=lens)
    g = torch.Generator(device="cuda").manual_seed(6)
    kn = [torch.randn(1, 2, s, D, generator=g, device="cuda").to(dtype) for s in S]
    vn = [torch.randn(1, 2, s, D, generator=g, device="cuda").to(dtype) for s in S]
    total = sum(S) + PAD
    qp, knp, vnp = (rg.pack(t, total, fill=0.0) for t in (qs, kn, vn))
    cu, sl = rg.cu_of(S, device="cuda"), qc.sl_of(fills)
    want = pools.clone()
    vck.splits(1)
    qc.plain_packed(qp, want, cu, sl, table, k_new=knp, v_new=vnp, is_causal=True)
    for n in (1, 3):
        vck.splits(n)
        got = pools.clone()
        out = torch.full((total, H, D), 7.0, dtype=dtype, device="cuda")
        o, lse = qc.Q().flash_attention_kvcache_quant_softcap_ragged(qp, got.k, got.v, cu, sl, table, cap, k_new=knp, v_new=vnp,
                                                                    is_causal=True, return_lse=True, out=out, **got.kw())
        assert o.data_ptr() == out.data_ptr() and (out[sum(S):] == 7.0).all(), "out is written in place, the padding rows are not"
        for name, a, w in zip(("k", "v", "k_scale", "v_scale"), got.tensors(), want.tensors()):
            assert torch.equal(qc.bits(a), qc.bits(w)), (name, n)
        res = list(zip(rg.unpack(o, S), rg.unpack_lse(lse, S)))
        check_each("packed append %s d%d n%d" % (fmt, D, n), qs, res, qc.gather(want, table), lens, cap, True, (-1, -1))


@pytest.mark.parametrize("fmt,D", [("e4m3", 128), ("token", 256), ("fp4", 64)])
def test_packed_graph_replays_after_everything_changes_in_place(fmt, D):
    cap, H, dtype = 50.0, 8, BF16
    qs, c, pools, table = problem(fmt, H, D, dtype, cap, 37, lens=[SC] * B)
    sl, total = qc.sl_of(LENS), sum(S) + PAD
    cu = rg.cu_of(S, device="cuda")
    qp = rg.pack(qs, total, fill=0.0)
    call = lambda: qc.Q().flash_attention_kvcache_quant_softcap_ragged(qp, pools.k, pools.v, cu, sl, table, cap, is_causal=True,
                                                                      return_lse=True, **pools.kw())
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for lens, S1 in (([652, 0, 302, 64, 2], [11, 3, 40, 1, 2]), ([704, 1, 33, 64, 300], [1, 1, 13, 1, 41])):
        sl.copy_(qc.sl_of(lens))
        cu.copy_(rg.cu_of(S1, device="cuda"))
        table.copy_(table.roll(1, 0))
        graph.replay()
        torch.cuda.synchronize()
        eager = call()
        n = sum(S1)
        assert torch.equal(qc.bits(out[0][:n]), qc.bits(eager[0][:n])) and torch.equal(qc.bits(out[1][:, :n]), qc.bits(eager[1][:, :n])), lens
        q1 = rg.unpack(qp, S1)
        res = list(zip(rg.unpack(out[0], S1), rg.unpack_lse(out[1], S1)))
        check_each("packed replay %s" % fmt, q1, res, qc.gather(pools, table), lens, cap, True, (-1, -1))
