"""GPU tests of packed variable-length decoding over paged MXFP4 pools (include/mi355fa_ragged_fp4.h; fp4_ragged_kvcache.py),
D = 64, 128 and 256.

The truth, the inputs, the bounds and the pool builders are those of tests/test_gpu_kvcache_fp4.py, by import: fp64 attention
on the dequantised cache, every (sequence, head) on its own held to relative Frobenius 1e-3 (fp16) / 8e-3 (bf16), LSE by
check_lse; make4's inputs keep every conversion exact, so the error is the 16-bit kernel's.  The packed layout comes from
tests/raggedcheck.py.  Shapes are the smallest that reach each path: a 32-key tile, four tiles (one workgroup step at
D <= 128, two at D = 256), five and seven tiles (odd shares: the D = 256 pair that only joins the barrier), 32 MFMA rows per
row block (g = 8 with S_b = 5 is 40 rows, two blocks)."""
import pytest
import torch

import raggedcheck as rg
import variantcheck as vck
import test_gpu_kvcache_fp4 as t4
from test_gpu_kvcache_fp4 import BF16, DT, F16, FF, IDS, MASKS

pytestmark = pytest.mark.gpu

S = [1, 0, 3, 5, 1, 2]                      # query counts: decode rows, an idle sequence, drafts
LENS = [1, 31, 32, 33, 129, 200]            # L_b: one tile, its edges, five tiles, seven tiles
PAD = 2                                     # total_q is two rows larger than cu[B]
TQ = sum(S) + PAD
SENTINEL = 1234.0
GEOMS = [(4, 2), (5, 1), (8, 1)]


def _R():
    import fp4_ragged_kvcache as R
    return R


def _F():
    import fp4_kvcache as F
    return F


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def cuda_cu(S):
    return rg.cu_of(S, device="cuda")


def step(H, Hkv, D, dtype, page, seed, lens=LENS, S=S, extra=0):
    """q per sequence and packed, the padded byte tensors [B, H_kv, reach, .] (rows at or past L_b + extra poisoned) and their
    pools under a permuted table, with pages for lens[b] + extra rows"""
    B = len(S)
    MP = -(-(max(lens) + extra) // page) + 1
    reach = MP * page
    qb, kc, vc, ks, vs = t4.make4(B, H, Hkv, max(max(S), 1), reach, D, dtype, seed=seed)
    q_seq = [qb[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)]
    q = rg.pack(q_seq, sum(S) + PAD, fill=0.0)
    owned = [L + extra for L in lens]
    pad = [t.clone() for t in (kc, vc, ks, vs)]
    for b, L in enumerate(lens):
        for t in pad:
            t[b, :, L:] = FF
    NP = sum(-(-L // page) for L in owned) + 4
    pools, table = t4.scatter4(pad, owned, page, NP, MP, seed=seed + 1)
    return dict(q=q, q_seq=q_seq, pad=pad, pools=pools, table=table, NP=NP, MP=MP, page=page, B=B)


def truths(st, lens, wl, wr, sinks, S=S):
    """the fp64 (O, LSE) of every sequence that has rows, computed once and shared by the split counts"""
    pad = st["pad"]
    K, V = t4.deq64(pad[0], pad[2]), t4.deq64(pad[1], pad[3])
    return {b: t4.truth(st["q_seq"][b], K[b:b + 1], V[b:b + 1], [lens[b]], wl, wr, sinks) for b in range(len(S)) if S[b]}


def check_step(tag, st, o, lse, refs, S=S):
    for b, (ob, lb) in enumerate(zip(rg.unpack(o, S), rg.unpack_lse(lse, S))):
        if S[b]:
            t4.check("%s b=%d" % (tag, b), st["q_seq"][b], ob, lb, *refs[b])


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("H,Hkv", GEOMS)
def test_matches_fp64_per_head(H, Hkv, D, dtype):
    R = _R()
    cu, sl = cuda_cu(S), torch.tensor(LENS, dtype=torch.int32, device="cuda")
    sinks = torch.linspace(-1.0, 3.0, H, device="cuda", dtype=torch.float32)
    for page in (32, 96):
        st = step(H, Hkv, D, dtype, page, seed=H + D + page)
        table = t4.wide(st["table"])
        for is_causal, window in MASKS:
            wl, wr = t4.window_of(is_causal, window)
            for sk in (None, sinks):
                refs = truths(st, LENS, wl, wr, sk)
                for n in (1, 2, 3):
                    vck.splits(n)
                    out = torch.full((TQ, H, D), SENTINEL, dtype=dtype, device="cuda")
                    o, lse = R.flash_attention_kvcache_fp4_ragged(st["q"], *st["pools"], cu, sl, table, is_causal=is_causal,
                                                                  window_size=window, return_lse=True, sinks=sk, out=out)
                    torch.cuda.synchronize()
                    assert o.data_ptr() == out.data_ptr() and lse.shape == (H, TQ)
                    assert (o[TQ - PAD:] == SENTINEL).all(), "a padding row of out was written"
                    tag = "page=%d causal=%s window=%s sinks=%s n=%d" % (page, is_causal, window, sk is not None, n)
                    check_step(tag, st, o, lse, refs)
    # LSE's padding rows: the binding allocates LSE, so the raw call shows them untouched
    import _mi355fa as fa
    vck.splits(2)
    lse = torch.full((H, TQ), SENTINEL, device="cuda")
    o = torch.full((TQ, H, D), SENTINEL, dtype=dtype, device="cuda")
    need = fa.lib.fa_fwd_kvcache_fp4_ragged_workspace_bytes(TQ, st["B"], H, Hkv, st["MP"], st["page"], D)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    tab = st["table"]
    P = lambda t: t.data_ptr()
    rc = fa.lib.fa_fwd_kvcache_fp4_ragged(P(st["q"]), *(P(t) for t in st["pools"]), None, None, P(cu), P(sl), P(tab), None, None,
                                          None, P(o), P(lse), P(ws), need, TQ, st["B"], H, Hkv, st["NP"], st["page"], st["MP"],
                                          st["MP"], D, int(dtype == BF16), fa.KV_MXFP4, D ** -0.5, -1, -1, None,
                                          torch.cuda.current_stream().cuda_stream)
    fa.check(rc, "fa_fwd_kvcache_fp4_ragged")
    torch.cuda.synchronize()
    assert (lse[:, TQ - PAD:] == SENTINEL).all() and (o[TQ - PAD:] == SENTINEL).all()
    check_step("raw n=2", st, o, lse, truths(st, LENS, -1, -1, None))


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("append", [False, True], ids=["plain", "append"])
def test_rows_of_a_sequence_have_the_bits_of_the_paged_call(append, D, dtype):
    R, F = _R(), _F()
    H, Hkv, page = 8, 2, 32
    extra = max(S) if append else 0
    st = step(H, Hkv, D, dtype, page, seed=31 + D, extra=extra)
    fills = LENS
    cu, sl = cuda_cu(S), torch.tensor(fills, dtype=torch.int32, device="cuda")
    kn_seq = vn_seq = None
    kw = {}
    if append:
        kn_b, vn_b = t4.append_inputs(len(S), Hkv, max(S), D, dtype, 32)
        kn_seq = [kn_b[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)]
        vn_seq = [vn_b[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)]
        kw = dict(k_new=rg.pack(kn_seq, TQ, fill=0.0), v_new=rg.pack(vn_seq, TQ, fill=0.0))
    for n in (1, 2, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            mine, theirs = [t.clone() for t in st["pools"]], [t.clone() for t in st["pools"]]
            o, lse = R.flash_attention_kvcache_fp4_ragged(st["q"], *mine, cu, sl, st["table"], is_causal=is_causal,
                                                          window_size=window, return_lse=True, **kw)
            ob, lb = rg.unpack(o, S), rg.unpack_lse(lse, S)
            for b, s in enumerate(S):
                if s == 0:
                    continue
                kwb = dict(k_new=kn_seq[b], v_new=vn_seq[b]) if append else {}
                ref = F.flash_attention_kvcache_fp4_paged(st["q_seq"][b], *theirs, sl[b:b + 1], st["table"][b:b + 1],
                                                          is_causal=is_causal, window_size=window, return_lse=True, **kwb)
                assert t4.same((ob[b], lb[b]), ref), (n, is_causal, window, b)
            for name, a, c in zip(("k_cache", "v_cache", "k_scale", "v_scale"), mine, theirs):
                assert torch.equal(a, c), (name, int((a != c).sum()))
            assert torch.equal(sl.cpu(), torch.tensor(fills, dtype=torch.int32))


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_d256_rows_have_the_bits_of_the_sequence_alone(dtype):
    """D = 256 has no rectangular sibling: the rows of sequence b in the mixed step have the bits of the packed call on that
    sequence alone."""
    R = _R()
    H, Hkv, D, page = 8, 2, 256, 32
    st = step(H, Hkv, D, dtype, page, seed=41)
    cu, sl = cuda_cu(S), torch.tensor(LENS, dtype=torch.int32, device="cuda")
    for n in (1, 2, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            o, lse = R.flash_attention_kvcache_fp4_ragged(st["q"], *st["pools"], cu, sl, st["table"], is_causal=is_causal,
                                                          window_size=window, return_lse=True)
            ob, lb = rg.unpack(o, S), rg.unpack_lse(lse, S)
            for b, s in enumerate(S):
                if s == 0:
                    continue
                qb = st["q_seq"][b][0].transpose(0, 1).contiguous()
                o1, l1 = R.flash_attention_kvcache_fp4_ragged(qb, *st["pools"], cuda_cu([s]), sl[b:b + 1], st["table"][b:b + 1],
                                                              is_causal=is_causal, window_size=window, return_lse=True)
                assert t4.same((ob[b], lb[b]), (o1.transpose(0, 1)[None].contiguous(), l1[None].contiguous())), (n, b)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_d256_nibble_order_and_block_scales_element_for_element(dtype):
    """The element test of the MXFP4 suite at D = 256: one key, unit-vector queries, so O = V exactly and LSE = K[d].  Each of
    the eight scale blocks has its own scale byte in K and in V: a wrong half offset (the nibbles' first byte, the 4-byte half of
    the K scale row, the V scale chunk) is off by far more than the bound."""
    R = _R()
    D = 256
    ar = torch.arange(D // 2, device="cuda", dtype=torch.int32)
    kc = (ar * 37 % 256).to(torch.uint8).view(1, 1, 1, D // 2).contiguous()
    vc = (ar * 91 % 256 ^ 0x5A).to(torch.uint8).view(1, 1, 1, D // 2).contiguous()
    ks = torch.tensor([125, 129, 126, 131, 124, 130, 127, 132], dtype=torch.uint8, device="cuda").view(1, 1, 1, -1)
    vs = torch.tensor([130, 124, 128, 127, 131, 125, 129, 126], dtype=torch.uint8, device="cuda").view(1, 1, 1, -1)
    pad = lambda t: torch.cat([t, torch.full((1, 1, 31, t.shape[-1]), FF, dtype=torch.uint8, device="cuda")], dim=2)
    K, V = t4.deq64(kc, ks)[0, 0, 0], t4.deq64(vc, vs)[0, 0, 0]
    assert V.unique().numel() >= 12 and K.unique().numel() >= 12
    assert not torch.equal(V[:128], V[128:]) and not torch.equal(K[:128], K[128:])
    q = torch.eye(D, device="cuda", dtype=dtype).view(1, D, D)                  # head h asks for element h
    sl = torch.ones(1, dtype=torch.int32, device="cuda")
    table = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    o, lse = R.flash_attention_kvcache_fp4_ragged(q, pad(kc), pad(vc), pad(ks), pad(vs), cuda_cu([1]), sl, table,
                                                  softmax_scale=1.0, return_lse=True)
    assert torch.equal(o.double(), V.expand(1, D, D)), "O = V: nibble order or V block scales"
    assert torch.allclose(lse[:, 0].double(), K, rtol=1e-5, atol=1e-5), "nibble order or K block scales"


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_append_writes_exactly_the_quantised_new_rows(D, dtype):
    R, F = _R(), _F()
    H, Hkv, page, MP = 4, 2, 32, 4
    Sa = [1, 3, 0, 5, 2]
    fills = [0, 30, 50, 60, MP * page - 2]                                      # a row that crosses a page; the table's reach
    B = len(Sa)
    after = [f + s for f, s in zip(fills, Sa)]
    qb, kc, vc, ks, vs = t4.make4(B, H, Hkv, max(Sa), MP * page, D, dtype, seed=51 + D)
    NP = sum(-(-L // page) for L in after) + 3
    pools, table = t4.scatter4([kc, vc, ks, vs], after, page, NP, MP, seed=52)
    kn_b, vn_b = t4.append_inputs(B, Hkv, max(Sa), D, dtype, 53)
    kn_seq = [kn_b[b:b + 1, :, :s].contiguous() for b, s in enumerate(Sa)]
    vn_seq = [vn_b[b:b + 1, :, :s].contiguous() for b, s in enumerate(Sa)]
    tq = sum(Sa) + PAD
    kn, vn = rg.pack(kn_seq, tq, fill=7.0), rg.pack(vn_seq, tq, fill=7.0)       # (the padding rows: real values, dropped)
    q = rg.pack([qb[b:b + 1, :, :s].contiguous() for b, s in enumerate(Sa)], tq, fill=0.0)
    want = [t.clone() for t in pools]
    for b, s in enumerate(Sa):
        if s == 0:
            continue
        (kq, kqs), (vq, vqs) = F.quantize_kv_mxfp4(kn_seq[b].cpu()), F.quantize_kv_mxfp4(vn_seq[b].cpu())
        for i in range(s):
            row = fills[b] + i
            pg, r = int(table[b, row // page]), row % page
            for t, new in zip(want, (kq, vq, kqs, vqs)):
                t[pg, :, r] = new[0, :, i].cuda()
    sl = torch.tensor(fills, dtype=torch.int32, device="cuda")
    o, lse = R.flash_attention_kvcache_fp4_ragged(q, *pools, cuda_cu(Sa), sl, t4.wide(table), k_new=kn, v_new=vn, is_causal=True,
                                                  return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(sl.cpu(), torch.tensor(fills, dtype=torch.int32))         # cache_seqlens is not modified
    for name, got, w in zip(("k_cache", "v_cache", "k_scale", "v_scale"), pools, want):
        assert torch.equal(got, w), (name, int((got != w).sum()))
    full = torch.tensor(after, dtype=torch.int32, device="cuda")
    o2, lse2 = R.flash_attention_kvcache_fp4_ragged(q, *want, cuda_cu(Sa), full, table, is_causal=True, return_lse=True)
    assert t4.same((o[:sum(Sa)], lse[:, :sum(Sa)]), (o2[:sum(Sa)], lse2[:, :sum(Sa)]))


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_poison_past_the_fill_level_is_never_read(D, dtype):
    R = _R()
    H, Hkv, page = 4, 2, 96
    st = step(H, Hkv, D, dtype, page, seed=61)
    zeros = [torch.zeros_like(t) for t in st["pad"]]
    for b, L in enumerate(LENS):
        for t in zeros:
            t[b, :, L:] = FF
    own, _ = t4.scatter4(zeros, LENS, page, st["NP"], st["MP"], seed=62)          # 0 where a sequence owns the byte
    clean = [torch.where(m == 0, p, torch.full_like(p, 0x7F if p.shape[-1] == D // 32 else 0x22)) for p, m in zip(st["pools"], own)]
    for p, m in zip(st["pools"], own):
        assert (p[m != 0] == FF).all() and (m != 0).any()
    cu, sl = cuda_cu(S), torch.tensor(LENS, dtype=torch.int32, device="cuda")
    for n in (1, 2, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window, return_lse=True)
            a = R.flash_attention_kvcache_fp4_ragged(st["q"], *clean, cu, sl, st["table"], **kw)
            b = R.flash_attention_kvcache_fp4_ragged(st["q"], *st["pools"], cu, sl, st["table"], **kw)
            rows = sum(S)
            assert torch.isfinite(b[0][:rows]).all() and not torch.isnan(b[1][:, :rows]).any()
            assert t4.same((a[0][:rows], a[1][:, :rows]), (b[0][:rows], b[1][:, :rows])), (n, is_causal, window)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 256])
def test_transposed_pools_and_a_fused_qkv_slice_are_read_in_place(D, dtype):
    R = _R()
    H, Hkv, page = 4, 2, 32
    st = step(H, Hkv, D, dtype, page, seed=71, extra=max(S))
    tr = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)     # [num_pages, page, H_kv, .] storage
    tp = [tr(t) for t in st["pools"]]
    assert not tp[0].is_contiguous() and tp[0].stride(2) == Hkv * D // 2 and tp[2].stride(2) == Hkv * D // 32
    qkv = torch.zeros(TQ, (H + 2 * Hkv) * D, dtype=dtype, device="cuda")
    qkv[:, :H * D] = st["q"].reshape(TQ, H * D)
    qs = qkv[:, :H * D].view(TQ, H, D)
    assert not qs.is_contiguous() and qs.stride(0) == (H + 2 * Hkv) * D
    cu, sl = cuda_cu(S), torch.tensor(LENS, dtype=torch.int32, device="cuda")
    kn_b, vn_b = t4.append_inputs(len(S), Hkv, max(S), D, dtype, 72)
    kn = rg.pack([kn_b[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)], TQ, fill=0.0)
    vn = rg.pack([vn_b[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)], TQ, fill=0.0)
    rows = sum(S)
    for kw in (dict(), dict(k_new=kn, v_new=vn, is_causal=True)):
        pc = [t.clone() for t in st["pools"]]
        a = R.flash_attention_kvcache_fp4_ragged(st["q"], *pc, cu, sl, st["table"], return_lse=True, **kw)
        b = R.flash_attention_kvcache_fp4_ragged(qs, *tp, cu, sl, st["table"], return_lse=True, **kw)
        assert t4.same((a[0][:rows], a[1][:, :rows]), (b[0][:rows], b[1][:, :rows]))
        for x, y in zip(pc, tp):
            assert torch.equal(x, y.contiguous())


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [128, 256])
def test_out_of_range_table_entries_touch_nothing_outside_the_pools(D, dtype):
    """Defined out-of-range behaviour, as in the paged MXFP4 suite: one table entry outside the pool for a page an append
    would write, inside guarded pools.  The row is dropped, no guard byte changes and the other sequences keep their bits.  Not
    a fault test: the kernels clamp such an entry to an empty page and the append drops the row."""
    R = _R()
    page, H, Hkv = 32, 4, 2
    Sa, fills = [1, 2, 1, 2], [70, 100, 33, 63]                                 # the last one: the append crosses into page 2
    B, MP, G = len(Sa), 5, 3
    after = [f + s for f, s in zip(fills, Sa)]
    qb, kc, vc, ks, vs = t4.make4(B, H, Hkv, max(Sa), MP * page, D, dtype, seed=81)
    NP = sum(-(-L // page) for L in after) + 2
    pools, table = t4.scatter4([kc, vc, ks, vs], after, page, NP, MP, seed=82)
    kn_b, vn_b = t4.append_inputs(B, Hkv, max(Sa), D, dtype, 83)
    tq = sum(Sa)
    pk = lambda t: rg.pack([t[b:b + 1, :, :s].contiguous() for b, s in enumerate(Sa)], tq, fill=0.0)
    q, kn, vn = pk(qb), pk(kn_b), pk(vn_b)
    cu, sl = cuda_cu(Sa), torch.tensor(fills, dtype=torch.int32, device="cuda")

    def guarded(pool):
        big = torch.full((NP + 2 * G, *pool.shape[1:]), FF, dtype=torch.uint8, device="cuda")
        big[G:G + NP] = pool
        return big

    def run(tab):
        bigs = [guarded(p) for p in pools]
        out = R.flash_attention_kvcache_fp4_ragged(q, *(b[G:G + NP] for b in bigs), cu, sl, tab, k_new=kn, v_new=vn, return_lse=True)
        torch.cuda.synchronize()
        for b in bigs:
            assert (b[:G] == FF).all() and (b[G + NP:] == FF).all(), "a guard byte was written"
        return out, bigs

    good, good_pools = run(table)
    bad = table.clone()
    bad[3, 2] = 1 << 30                                                         # the page the second appended row of 3 goes to
    (o, lse), bad_pools = run(bad)
    assert torch.isfinite(o).all() and not torch.isnan(lse).any()
    ob, lb, gb, glb = rg.unpack(o, Sa), rg.unpack_lse(lse, Sa), rg.unpack(good[0], Sa), rg.unpack_lse(good[1], Sa)
    for b in (0, 1, 2):
        assert t4.same((ob[b], lb[b]), (gb[b], glb[b])), b
    # row 63 of sequence 3 lands in its page 1; row 64 is dropped: the page the good table names for it keeps its bytes
    dropped = int(table[3, 2])
    for p, gp, bp in zip(pools, good_pools, bad_pools):
        assert torch.equal(bp[G + dropped], p[dropped]) and not torch.equal(gp[G + dropped], p[dropped])
        keep = torch.ones(NP, dtype=torch.bool)
        keep[dropped] = False
        assert torch.equal(gp[G:G + NP][keep], bp[G:G + NP][keep]), "another page changed"


@pytest.mark.parametrize("D", [128, 256])
def test_graph_captured_step_replays_while_the_step_changes_in_place(D):
    R = _R()
    H, Hkv, page, dtype = 8, 2, 32, BF16
    st = step(H, Hkv, D, dtype, page, seed=91, extra=3 * max(S))
    g = torch.Generator(device="cuda").manual_seed(92)
    q = st["q"].clone()
    kn = torch.randn(TQ, Hkv, D, generator=g, device="cuda").to(dtype)
    vn = torch.randn(TQ, Hkv, D, generator=g, device="cuda").to(dtype)
    cu, sl, table = cuda_cu(S), torch.tensor(LENS, dtype=torch.int32, device="cuda"), st["table"].clone()
    pools = st["pools"]
    vck.splits(2)                                                               # the combine kernel is in the graph too
    out = torch.zeros(TQ, H, D, dtype=dtype, device="cuda")

    def eager():
        c = [t.clone() for t in pools]
        o = R.flash_attention_kvcache_fp4_ragged(q, *c, cu.clone(), sl.clone(), table.clone(), k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        return o, c

    eager()                                                                     # warm-up (allocator)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        R.flash_attention_kvcache_fp4_ragged(q, *pools, cu, sl, table, k_new=kn, v_new=vn, is_causal=True, out=out)
    counts = [S, [2, 1, 0, 4, 3, 2], [0, 0, 6, 1, 1, 4]]                        # each sums to cu[B] = 12 at most
    for i, Si in enumerate(counts):
        cu.copy_(cuda_cu(Si))
        if i == 2:                                                              # two sequences swap their pages and fills
            table[[0, 5]] = table[[5, 0]]
            sl[[0, 5]] = sl[[5, 0]]
        rows = sum(Si)
        o_e, c_e = eager()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[:rows].view(torch.int16), o_e[:rows].view(torch.int16)), i
        assert all(torch.equal(a, b) for a, b in zip(pools, c_e)), i
        sl += torch.tensor(Si, dtype=torch.int32, device="cuda")                # advance in place; the next step's q / k / v
        q.copy_((torch.randn(q.shape, generator=g, device="cuda") * 0.03).to(dtype))
        kn.copy_(torch.randn(kn.shape, generator=g, device="cuda").to(dtype))
        vn.copy_(torch.randn(vn.shape, generator=g, device="cuda").to(dtype))
