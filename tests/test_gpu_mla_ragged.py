"""GPU tests of MLA decoding over a paged latent cache with packed variable-length queries
(include_mla_ragged/mi355fa_ragged_mla.h, mla_ragged_kvcache.flash_attention_mla_kvcache_ragged).

Helpers, truth and bounds: tests/mlaraggedcheck.py over tests/mlacheck.py.  1. fp64 parity of one batch that holds empty
sequences first, in the middle and last, a keyless sequence with a query, drafts around a tile edge, a prefill chunk of many row
blocks and a decode row, at H = 16 / 24 / 128 (24: a 32-row block spans two queries and a sequence's last block is partial),
under permuted tables of 32- and 64-key pages with NaN everywhere outside the live keys, strided q and out= with sentinels, the
append bit for bit.  2. the bits of the rectangular call on each sequence alone, at forced split counts.  3. a deep table.
4. another softmax scale.  5. malformed cu_seqlens_q between guard thirds.  6. a captured step replayed while cu_seqlens_q,
cache_seqlens and block_table change in place.  Shapes are the smallest that reach each path."""
import pytest
import torch

import mlacheck as mc
import mlaraggedcheck as mr
import variantcheck as vck
from mlacheck import BF16, D, DV

pytestmark = pytest.mark.gpu

PAD = 3                                       # packed rows allocated past cu[B]
SENT = 777.0                                  # what nothing writes: exact in fp16, bf16 and fp32
SCALE, SCALE_QMUL = 192 ** -0.5, 1.0          # tests/test_host_mla_ragged.py holds the reference-only condition on the CPU
SCALE_SEQS = [(2, 33), (1, 129), (0, 50), (3, 300)]


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def ids(dtype):
    return mc.IDS[mc.DT.index(dtype)]


def wide_q(step):
    """step.qp as a slice of a wider [total_q, H, 640] tensor, NaN around it and in the rows past cu[B]"""
    w = torch.full((step.total_q, step.H, 640), float("nan"), dtype=step.dtype, device="cuda")
    w[..., 32:32 + D] = step.qp
    return w[..., 32:32 + D]


def call(step, pool, table, causal, q=None, out=None, scale=None, cu=None, sl=None):
    return mr.R()(step.qp if q is None else q, pool, step.cu if cu is None else cu, step.sl if sl is None else sl, table,
                  kv_new=step.new if step.append else None, is_causal=causal, softmax_scale=scale, return_lse=True, out=out)


def raw_call(step, pool, table, o, lse, ws, causal, q=None, cu=None, scale=None):
    """the C entry point with o, lse and the workspace owned by the caller (contiguous q / o rows, the pool through its strides)"""
    import _mi355fa as fa
    import ctypes
    P = lambda t: t.data_ptr()
    need = fa.lib.fa_fwd_kvcache_mla_ragged_workspace_bytes(step.total_q, step.B, step.H, table.shape[1], pool.shape[1])
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert 0 < need <= ws.numel() and ws.is_contiguous()
    ks = (ctypes.c_longlong * 2)(pool.stride(0), pool.stride(1))
    q = step.qp if q is None else q
    assert q.is_contiguous() and o.is_contiguous() and lse.is_contiguous() and step.new.is_contiguous()
    rc = fa.lib.fa_fwd_kvcache_mla_ragged(P(q), P(pool), P(step.new) if step.append else None, P(step.cu if cu is None else cu),
                                          P(step.sl), P(table), P(o), P(lse), P(ws), need, step.total_q, step.B, step.H, pool.shape[0],
                                          pool.shape[1], table.shape[1], table.stride(0), int(step.append), int(step.dtype == BF16),
                                          mc.DEFAULT_SCALE if scale is None else scale, int(causal), None, ks, None,
                                          torch.cuda.current_stream().cuda_stream)
    fa.check(rc, "fa_fwd_kvcache_mla_ragged")
    return need


def wide_clone(pool):
    """a copy of a pool whose rows are 640 elements apart, with the same strides and NaN between the rows"""
    w = torch.full((pool.shape[0], pool.shape[1], 640), float("nan"), dtype=pool.dtype, device=pool.device)
    w[..., :D] = pool
    return w, w[..., :D]


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- 1. fp64 parity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("append", [False, True], ids=["noappend", "append"])
@pytest.mark.parametrize("H", [16, 24, 128])
def test_parity_with_fp64_on_a_mixed_batch(H, append, dtype):
    step = mr.Step(mr.BATCH, H, dtype, append, seed=H + append, pad=PAD)
    assert step.rows == 53 and step.total_q == 56 and (append or 0 in [L for s, L in zip(step.S, step.Ls) if s])
    q = wide_q(step)
    for causal in (False, True):
        truths = step.truth(causal, level=True)
        for page in (32, 64):
            before, table, after = step.pools(page, mc.pages_of(384, page), 3, row_stride=640)
            assert before.stride(1) == 640
            wpool, pool = wide_clone(before)
            assert pool.stride(1) == 640
            owide = torch.full((step.total_q, H, DV + 64), SENT, dtype=dtype, device="cuda")
            o, lse = call(step, pool, table, causal, q=q, out=owide[..., :DV])
            tag = "packed parity H%d %s append%d causal%d page%d" % (H, ids(dtype), append, causal, page)
            assert o.data_ptr() == owide.data_ptr()
            mr.held(tag, step, o, lse, truths)
            assert (owide[step.rows:] == SENT).all() and (owide[..., DV:] == SENT).all(), (tag, "rows past cu[B] and the padding of out")
            # the pool: with an append the reference pool bit for bit (NaN padding included), untouched without
            assert torch.equal(bits(pool), bits(after)), (tag, "the pool after the step")
            assert torch.isnan(wpool[..., D:]).all(), (tag, "the padding between the pool's rows")
            assert step.sl.tolist() == step.fills and step.cu.tolist() == step.cu_list
            # LSE past cu[B] (the wrapper allocates LSE: the C entry point on buffers of our own), and the same bits
            o2 = torch.full((step.total_q, H, DV), SENT, dtype=dtype, device="cuda")
            lse2 = torch.full((H, step.total_q), SENT, device="cuda")
            _, pool2 = wide_clone(before)
            raw_call(step, pool2, table, o2, lse2, None, causal, q=q.contiguous())
            assert (lse2[:, step.rows:] == SENT).all() and (o2[step.rows:] == SENT).all(), (tag, "LSE and O past cu[B]")
            assert torch.equal(bits(o2[:step.rows]), bits(o[:step.rows])) and torch.equal(bits(lse2[:, :step.rows]), bits(lse[:, :step.rows]))
            assert torch.equal(bits(pool2), bits(after))


# ---- 2. the bits of the rectangular call on each sequence alone ------------------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("append", [False, True], ids=["noappend", "append"])
@pytest.mark.parametrize("H", [24, 128])
def test_each_sequence_has_the_bits_of_the_rectangular_call_on_it_alone(H, append, dtype):
    step = mr.Step(mr.BATCH, H, dtype, append, seed=20 + H, pad=PAD)
    before, table, after = step.pools(64, 6, 5)
    for causal in (True, False):
        for n in (1, 2, 3, 5):
            vck.splits(n)
            o, lse = call(step, before.clone(), table, causal)
            for b in range(step.B):
                if step.S[b] == 0:
                    continue
                ref = mc.M()(step.q[b], after, torch.tensor([step.Ls[b]], dtype=torch.int32, device="cuda"), table[b:b + 1],
                             is_causal=causal, return_lse=True)
                assert mr.same_rows(o, lse, step.cu_list, b, ref), (n, causal, b, step.S[b], step.Ls[b])


# ---- 3. a deep table: the steady state of the lookup pipeline ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_deep_table_at_three_tiles_per_page(dtype):
    page = 96
    after = [43 * 32 + 5, 45 * 32, 45 * 32 + 17, 46 * 32 + 31, 47 * 32 + 1, 49 * 32]         # 44 .. 49 tiles of keys
    S = [1, 2, 4, 1, 4, 2]
    assert [mc.pages_of(L, 32) for L in after] == [44, 45, 46, 47, 48, 49]
    step = mr.Step([(s, L - s) for s, L in zip(S, after)], 16, dtype, True, seed=31, pad=PAD, S_pad=49 * 32)
    truths = step.truth(True, level=True)
    before, table, want = step.pools(page, mc.pages_of(49 * 32, page), 9)
    for n in (0, 1):
        vck.splits(n)
        pool = before.clone()
        o, lse = call(step, pool, table, True)
        mr.held("packed deep table %s n%d" % (ids(dtype), n), step, o, lse, truths)
        assert torch.equal(bits(pool), bits(want))


# ---- 4. another softmax scale --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_the_deepseek_scale(dtype):
    step = mr.Step(SCALE_SEQS, 16, dtype, True, seed=95)
    step.q = [(x.float() * SCALE_QMUL).to(dtype) for x in step.q]
    step.qp = mr.pack_rows(step.q, step.total_q, float("nan"))
    truths = step.truth(True, SCALE, level=True)
    before, table, _ = step.pools(64, 5, 13)
    for n in (0, 3):
        vck.splits(n)
        o, lse = call(step, before.clone(), table, True, scale=SCALE)
        mr.held("packed scale %.4f %s n%d" % (SCALE, ids(dtype), n), step, o, lse, truths)


# ---- 5. malformed cu_seqlens_q ---------------------------------------------------------------------------------------------------
def thirds(shape, dtype, fill=SENT):
    """(a buffer of three times the size filled with `fill`, its middle third as a contiguous tensor of `shape`)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((3 * n,), fill, dtype=dtype, device="cuda")
    return buf, buf[n:2 * n].view(*shape)


def guards_intact(buf, fill=SENT):
    n = buf.numel() // 3
    return bool((buf[:n] == fill).all() and (buf[2 * n:] == fill).all())


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_malformed_cu_seqlens_q_touches_nothing_outside_the_packed_tensors(dtype):
    seqs = [(3, 40), (4, 100), (1, 31), (4, 65)]                                 # total_q 12
    H = 16
    step = mr.Step(seqs, H, dtype, True, seed=41)
    T = step.total_q
    bad = {"descending": [0, 8, 3, 12, 5], "negative": [0, -5, 4, -T, 12], "too large": [0, 4, 2 * T, 8, 2 * T]}
    before, table, after = step.pools(64, 3, 15)
    truths = step.truth(True, level=True)
    qbuf, q = thirds((T, H, D), dtype)
    q.copy_(step.qp)
    obuf, o = thirds((T, H, DV), dtype)
    lbuf, lse = thirds((H, T), torch.float32)
    for n in (0, 2):
        vck.splits(n)
        import _mi355fa as fa
        need = fa.lib.fa_fwd_kvcache_mla_ragged_workspace_bytes(T, step.B, H, table.shape[1], before.shape[1])
        wbuf, ws = thirds((need,), torch.uint8, fill=0x5a)
        for name, vals in bad.items():
            assert all(-T <= v <= 2 * T for v in vals)
            cu = torch.tensor(vals, dtype=torch.int32, device="cuda")
            pool = before.clone()
            assert raw_call(step, pool, table, o, lse, ws, True, q=q, cu=cu) == need
            torch.cuda.synchronize()
            assert guards_intact(qbuf) and guards_intact(obuf) and guards_intact(lbuf) and guards_intact(wbuf, 0x5a), (name, n)
            assert torch.equal(bits(q), bits(step.qp)) and cu.tolist() == vals, (name, n)
        # a following well-formed call on the same buffers is correct
        pool = before.clone()
        raw_call(step, pool, table, o, lse, ws, True, q=q)
        mr.held("packed after malformed %s n%d" % (ids(dtype), n), step, o, lse, truths)
        assert torch.equal(bits(pool), bits(after))
        assert guards_intact(qbuf) and guards_intact(obuf) and guards_intact(lbuf) and guards_intact(wbuf, 0x5a), n


# ---- 6. graph replay -----------------------------------------------------------------------------------------------------------
def test_captured_step_replays_while_cu_seqlens_and_table_change_in_place():
    page, mp, H, T, B = 64, 3, 16, 8, 3
    dtype = BF16
    g = torch.Generator(device="cuda").manual_seed(97)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(dtype)
    q, new, kv = r(T, H, D), r(T, D), r(B, mp * page, D)
    pool0, table = mc.scatter(kv, [mp * page] * B, page, mp, 17)                # every page of the table in use
    cu = torch.tensor([0, 1, 4, 8], dtype=torch.int32, device="cuda")
    sl = torch.tensor([3, page - 2, 2 * page], dtype=torch.int32, device="cuda")
    pool = pool0.clone()
    out = torch.zeros(T, H, DV, dtype=dtype, device="cuda")
    step = lambda p, o: mr.R()(q, p, cu, sl, table, kv_new=new, is_causal=True, return_lse=True, out=o)
    step(pool0.clone(), torch.zeros_like(out))                                  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step(pool, out)
    gen = torch.Generator().manual_seed(99)
    #           lengths change; the middle sequence empty; rows 5 .. 7 left as padding with the first sequence empty
    for cus, lens in (([0, 3, 5, 8], [4, page, 2 * page + 1]), ([0, 4, 4, 8], [page + 7, 2 * page - 1, 3 * page - 4]),
                      ([0, 0, 2, 5], [0, 1, page])):
        perm = torch.randperm(pool.shape[0], generator=gen).cuda()              # old page -> new page, all in place
        moved = torch.empty_like(pool0)
        moved[perm] = pool0
        pool0 = moved
        pool.copy_(pool0)
        table.copy_(perm[table.long()].to(torch.int32))
        sl.copy_(torch.tensor(lens, dtype=torch.int32))
        cu.copy_(torch.tensor(cus, dtype=torch.int32))
        eager_pool, eager_out = pool0.clone(), torch.zeros_like(out)
        eo, el = step(eager_pool, eager_out)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        n = cus[-1]
        assert torch.equal(bits(got[0]), bits(eo)) and torch.equal(bits(got[1][:, :n]), bits(el[:, :n])), cus
        assert (eo[:n].float().abs().sum(dim=(1, 2)) > 0).all() and (eo[n:] == 0).all(), "rows of sequences written, padding rows not"
        assert torch.equal(bits(pool), bits(eager_pool)) and not torch.equal(bits(eager_pool), bits(pool0))
        pool0 = eager_pool
