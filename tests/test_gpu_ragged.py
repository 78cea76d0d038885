"""GPU tests of paged-cache decoding with packed variable-length queries (include/mi355fa_ragged.h,
ragged_kvcache.flash_attention_kvcache_ragged).

The oracle is the paged kernel: a row block of sequence b is the same work item whichever way the launch finds it, so the
rows of sequence b must have THE BITS of flash_attention_kvcache_paged on that sequence alone (q_b [1, H, S_b, D], rows b of
cache_seqlens and block_table) at the same forced split count -- for the six variants, with an empty sequence, single rows
and several row blocks per sequence in one batch, key lengths that include 0 and one below its sequence's query count, and
five NaN padding rows behind the last sequence whose rows of O and LSE must keep their sentinel.  Then: equal lengths
against the batched paged call, fp64 accuracy on its own, order independence, more sequences than the plan kernel is wide,
strided q / out, the packed append (16-bit and fp8), a captured step replayed while all three device arrays change, and a
malformed cu_seqlens_q.  Pools come from tests/pagedcheck.py: a stray read is a NaN, never a fault, and no table entry is
out of range.  Shapes are the smallest that reach each path; every case runs in a few seconds."""
import ctypes

import pytest
import torch

import blockcheck as bc
import pagedcheck as pc
import raggedcheck as rc
import test_gpu_kvcache as tk
import test_gpu_paged as tpg
import variantcheck as vck

pytestmark = pytest.mark.gpu

F16, BF16, E4M3 = torch.float16, torch.bfloat16, torch.float8_e4m3fn
GROUPS = [(4, 4), (8, 2), (8, 1)]
MASKS = tk.MASKS                         # full, causal, window (40, 8)
VARIANTS = tpg.VARIANTS
MAX_PAGES = tpg.MAX_PAGES
S_BASE = [0, 1, 3, 40, 1, 9]             # an empty sequence, single rows, 36 rows at g = 4, 10 row blocks at g = 8
PAD = 5                                  # q rows past cu[B]
SENT = -77.0                             # the pre-fill of O and LSE


def base_lens(page):
    """key lengths from lengths(page) of the paged tests: 0 under a query, 31 < 40 queries, both ends of the table"""
    lens = [33, 0, 2 * page + 5, 31, page, MAX_PAGES * page]
    assert set(lens) <= set(tpg.lengths(page))
    return lens


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def _ragged():
    import ragged_kvcache as R
    return R.flash_attention_kvcache_ragged


def _paged():
    import paged_kvcache as P
    return P.flash_attention_kvcache_paged


class Step:
    """One step: sequences of S[b] queries over lens[b] keys, as the packed call takes it (q with `pad` NaN rows behind the
    last sequence) and as the per-sequence paged calls it must reproduce take it."""

    def __init__(self, variant, dtype, D, H, Hkv, S, page, lens, seed, pad=PAD, alloc=None, max_pages=MAX_PAGES):
        assert len(S) == len(lens)
        self.variant, self.S, self.lens, self.page, self.dtype = variant, list(S), list(lens), page, dtype
        self.H, self.Hkv, self.D = H, Hkv, D
        B = len(S)
        g = torch.Generator(device="cuda").manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g, device="cuda")
        self.qs = [r(1, H, s, D).to(dtype) for s in S]
        self.total = sum(S) + pad
        self.q = rc.pack(self.qs, self.total)
        self.cu = rc.cu_of(S, "cuda")
        self.fp8 = variant.startswith("fp8")
        kc, vc = ((r(B, Hkv, max_pages * page, D) * (2.0 if self.fp8 else 1.0)).to(E4M3 if self.fp8 else dtype) for _ in range(2))
        pages = sum(pc.pages_of(L, page) for L in (alloc or lens))
        (self.kp, self.vp), self.table = pc.scatter([kc, vc], lens, page, pages + 5, max_pages, seed, alloc=alloc)
        self.sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        self.mods = {}
        if variant == "softcap":
            self.mods = dict(softcap=15.0)
        elif variant == "alibi":
            self.mods = dict(alibi_slopes=torch.rand(B, H, generator=g, device="cuda") * 0.5 + 0.01)
        elif variant in ("sink", "fp8_sink"):
            self.mods = dict(sinks=r(H))
        if self.fp8:
            self.mods.update(k_descale=torch.rand(B, Hkv, generator=g, device="cuda") + 0.5,
                             v_descale=torch.rand(Hkv, generator=g, device="cuda") + 0.5)

    def mods_of(self, b):
        """the transform of sequence b alone: the (B, .) vectors' row b"""
        return {k: (v[b:b + 1] if isinstance(v, torch.Tensor) and v.dim() == 2 else v) for k, v in self.mods.items()}

    def ragged(self, kp=None, vp=None, q=None, out=None, **kw):
        """(O, LSE) of the packed call; O pre-filled with the sentinel unless `out` is given"""
        q = self.q if q is None else q
        if out is None:
            out = torch.full((self.total, self.H, self.D), SENT, dtype=self.dtype, device="cuda")
        o, lse = _ragged()(q, self.kp if kp is None else kp, self.vp if vp is None else vp, self.cu, self.sl, self.table,
                           return_lse=True, out=out, **self.mods, **kw)
        assert o.data_ptr() == out.data_ptr()
        return o, lse

    def per_sequence(self, kp=None, vp=None, k_new=None, v_new=None, **kw):
        """[(O [1, H, S_b, D], LSE [1, H, S_b]) or None for an empty sequence]: the paged call on each sequence alone"""
        res = []
        for b, s in enumerate(self.S):
            if s == 0:
                res.append(None)
                continue
            new = {} if k_new is None else dict(k_new=k_new[b], v_new=v_new[b])
            res.append(_paged()(self.qs[b], self.kp if kp is None else kp, self.vp if vp is None else vp, self.sl[b:b + 1],
                                self.table[b:b + 1].contiguous(), return_lse=True, **self.mods_of(b), **new, **kw))
        return res


def assert_rows(step, got, refs, what, sentinel=True):
    """the rows of every sequence have the bits of its reference; the padding rows of O keep the sentinel"""
    o, lse = got
    os, ls = rc.unpack(o, step.S), rc.unpack_lse(lse, step.S)
    for b, ref in enumerate(refs):
        if ref is None:
            continue
        assert bc.same_bits(os[b], ref[0]), ("O", b, what)
        assert bc.same_bits(ls[b], ref[1]), ("LSE", b, what)
    if sentinel:
        assert (o[sum(step.S):] == SENT).all(), ("O padding", what)


def raw_ragged(step, n, is_causal=False, window=(-1, -1), cu=None, guard=64):
    """fa_fwd_kvcache_ragged through ctypes at `n` forced splits with O, LSE and the workspace each inside a larger buffer
    of sentinel bytes.  Returns (O, LSE, the three whole buffers as bytes before the call, the same after it, the three
    (start, stop) byte ranges the call may write)."""
    import _mi355fa as fa
    vck.splits(n)
    T, H, D, Hkv, B = step.total, step.H, step.D, step.Hkv, len(step.S)
    NP, MP, page = step.kp.shape[0], step.table.shape[1], step.page
    cdt = fa.PAGED_CACHE_FP8_E4M3 if step.fp8 else fa.PAGED_CACHE_16BIT
    need = fa.lib.fa_fwd_kvcache_ragged_workspace_bytes(T, B, H, Hkv, MP, page, D, cdt)
    assert need == rc.workspace_bytes(n, T, B, H, Hkv, D), need
    G = guard * H * D * 2                                                  # guard bytes on each side (a multiple of 16)
    sizes = (T * H * D * 2, H * T * 4, need)
    bufs = [torch.full((G + (sz + 15) // 16 * 16 + G,), 0xA5, dtype=torch.uint8, device="cuda") for sz in sizes]
    bufs[0].view(step.dtype)[:] = SENT
    bufs[1].view(torch.float32)[:] = SENT
    before = [x.clone() for x in bufs]
    o = bufs[0][G:G + sizes[0]].view(step.dtype).view(T, H, D)
    lse = bufs[1][G:G + sizes[1]].view(torch.float32).view(H, T)
    ws = bufs[2][G:G + sizes[2]]
    m = step.mods
    P = lambda t: None if t is None else t.data_ptr()
    kd, vd = m.get("k_descale"), m.get("v_descale")
    if kd is not None and vd.dim() == 1:
        vd = vd.expand(B, Hkv).contiguous()
    sl = m.get("alibi_slopes")
    mods = fa.PagedMods(softcap=m.get("softcap", 0.0), alibi_slopes=P(sl), slopes_batch_stride=H if sl is not None else 0,
                        sinks=P(m.get("sinks")), k_descale=P(kd), v_descale=P(vd), descale_bstride=Hkv if kd is not None else 0)
    wl, wr = tk.window_of(is_causal, window)
    cu = step.cu if cu is None else cu
    fa.check(fa.lib.fa_fwd_kvcache_ragged(P(step.q), P(step.kp), P(step.vp), None, None, P(cu), P(step.sl), P(step.table),
                                          P(o), P(lse), P(ws), need, T, B, H, Hkv, NP, page, MP, MP, D,
                                          int(step.dtype == BF16), cdt, D ** -0.5, wl, wr, ctypes.byref(mods), None,
                                          torch.cuda.current_stream().cuda_stream), "fa_fwd_kvcache_ragged")
    torch.cuda.synchronize()
    return o, lse, before, bufs, [(G, G + sz) for sz in sizes]


def assert_guards(before, after, ranges, what):
    for i, (x, y, (a, b)) in enumerate(zip(before, after, ranges)):
        assert torch.equal(x[:a], y[:a]) and torch.equal(x[b:], y[b:]), ("bytes outside buffer %d were written" % i, what)


# ---- 1. the bits of the per-sequence call ----------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [32, 64])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("variant", VARIANTS)
def test_rows_of_a_sequence_have_the_bits_of_the_paged_call_on_it(variant, D, dtype, page):
    for H, Hkv in GROUPS:
        st = Step(variant, dtype, D, H, Hkv, S_BASE, page, base_lens(page), seed=D + H + page)
        tail = sum(st.S)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            for n in (1, 3, 7):
                vck.splits(n)
                what = (H, Hkv, is_causal, window, n)
                refs = st.per_sequence(**kw)
                got = st.ragged(**kw)
                assert torch.isfinite(got[0][:tail]).all() and not torch.isnan(got[1][:, :tail]).any(), what
                assert_rows(st, got, refs, what)
                again = st.ragged(**kw)                                        # and its own bits again
                assert bc.same_bits(again[0], got[0]) and bc.same_bits(again[1][:, :tail], got[1][:, :tail]), what
                # through the C ABI with O, LSE and the workspace pre-filled: the same bits, and the padding rows of both
                # keep every byte
                o, lse, before, after, ranges = raw_ragged(st, n, is_causal, window)
                assert bc.same_bits(o, got[0]) and bc.same_bits(lse[:, :tail], got[1][:, :tail]), what
                assert (lse[:, tail:] == SENT).all() and (o[tail:] == SENT).all(), what
                assert_guards(before, after, ranges, what)


# ---- 2. equal lengths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", [(64, F16), (128, BF16)], ids=["d64-fp16", "d128-bf16"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_equal_lengths_have_the_bits_of_the_batched_paged_call(variant, D, dtype):
    page = 64
    for H, Hkv in GROUPS:
        for Sq in (1, 3):
            c = tpg.Case(variant, dtype, D, H, Hkv, Sq, page, tpg.lengths(page), seed=3 + D + Sq + H)
            B = len(c.lens)
            packed = c.q.transpose(1, 2).reshape(B * Sq, H, D).contiguous()
            q4 = packed.view(B, Sq, H, D).transpose(1, 2)                       # the same memory as the paged call sees it
            cu = rc.cu_of([Sq] * B, "cuda")
            for is_causal, window in MASKS:
                kw = dict(is_causal=is_causal, window_size=window, return_lse=True, **c.mods)
                for n in (1, 3, 7):
                    vck.splits(n)
                    ro, rl = _paged()(q4, c.kp, c.vp, c.sl, c.table, **kw)
                    o, lse = _ragged()(packed, c.kp, c.vp, cu, c.sl, c.table, **kw)
                    what = (H, Hkv, Sq, is_causal, window, n)
                    assert o.shape == (B * Sq, H, D) and lse.shape == (H, B * Sq) and o.is_contiguous()
                    assert bc.same_bits(o.view(B, Sq, H, D).transpose(1, 2).contiguous(), ro.contiguous()), what
                    assert bc.same_bits(lse.view(H, B, Sq).transpose(0, 1).contiguous(), rl.contiguous()), what


# ---- 3. accuracy on its own -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [32, 64])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_plain_variant_matches_fp64_per_sequence(D, dtype, page):
    for H, Hkv in GROUPS:
        st = Step("plain", dtype, D, H, Hkv, S_BASE, page, base_lens(page), seed=7 + D + H)
        kc, vc = pc.gather(st.kp, st.table), pc.gather(st.vp, st.table)
        for is_causal, window in MASKS:
            wl, wr = tk.window_of(is_causal, window)
            ref = []
            for b, s in enumerate(st.S):
                if s == 0:
                    ref.append(None)
                    continue
                one = (st.qs[b], kc[b:b + 1], vc[b:b + 1], [st.lens[b]], wl, wr)
                O_ref, LSE_ref = tk.ref_fp64(*one)
                ref.append((O_ref, LSE_ref, tk.tol(dtype, *one, O_ref)))
            for n in (0, 3):
                vck.splits(n)
                o, lse = st.ragged(is_causal=is_causal, window_size=window)
                os, ls = rc.unpack(o, st.S), rc.unpack_lse(lse, st.S)
                for b, r in enumerate(ref):
                    if r is None:
                        continue
                    err = tk.rel(os[b], r[0])
                    assert err < r[2], (H, Hkv, b, is_causal, window, n, err, r[2])
                    tk.check_lse(ls[b], r[1])
                    assert (os[b][torch.isinf(r[1])] == 0).all()
        # the base batch has rows without a visible key: the sequence over no keys, and the negative positions of S_b > L_b
        assert torch.isinf(ref[1][1]).all() and torch.isinf(ref[3][1]).any() and not torch.isinf(ref[3][1]).all()


# ---- 4. order independence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "alibi", "fp8_sink"])
def test_permuting_the_sequences_leaves_each_sequences_bits(variant):
    page, D, H, Hkv = 64, 128, 8, 2
    st = Step(variant, BF16, D, H, Hkv, S_BASE, page, base_lens(page), seed=41)
    for perm in ([5, 3, 0, 4, 1, 2], [3, 5, 4, 2, 1, 0]):
        pm = Step.__new__(Step)
        pm.__dict__.update(st.__dict__)
        pm.S, pm.lens, pm.qs = [st.S[i] for i in perm], [st.lens[i] for i in perm], [st.qs[i] for i in perm]
        pm.q, pm.cu = rc.pack(pm.qs, st.total), rc.cu_of(pm.S, "cuda")
        idx = torch.tensor(perm, device="cuda")
        pm.sl, pm.table = st.sl[idx].contiguous(), st.table[idx].contiguous()
        pm.mods = {k: (v[idx].contiguous() if isinstance(v, torch.Tensor) and v.dim() == 2 else v) for k, v in st.mods.items()}
        for n in (1, 3):
            vck.splits(n)
            for is_causal, window in MASKS:
                kw = dict(is_causal=is_causal, window_size=window)
                a, b = st.ragged(**kw), pm.ragged(**kw)
                ao, al = rc.unpack(a[0], st.S), rc.unpack_lse(a[1], st.S)
                bo, bl = rc.unpack(b[0], pm.S), rc.unpack_lse(b[1], pm.S)
                for j, i in enumerate(perm):
                    assert bc.same_bits(bo[j], ao[i]) and bc.same_bits(bl[j], al[i]), (perm, n, is_causal, window, i)


# ---- 5. more sequences than the plan kernel is wide ---------------------------------------------------------------------------
def test_three_hundred_sequences_against_the_paged_calls_grouped_by_length():
    """B = 300 > the 256 sequences the plan kernel scans at a time; S_b in {0, 1, 2}.  The oracle is the batched paged call
    over the sequences of each non-zero S_b (an S_q = 0 call does not exist: the sequences of S_b = 0 own no row, and the
    rows of the others tile [0, cu[B]) exactly, so nothing is left unchecked)."""
    B, page, D, H, Hkv = 300, 32, 64, 8, 2
    gen = torch.Generator().manual_seed(51)
    S = torch.randint(0, 3, (B,), generator=gen).tolist()
    lens = torch.randint(0, 41, (B,), generator=gen).tolist()
    assert {0, 1, 2} == set(S) and min(lens) == 0 and max(lens) == 40
    st = Step("plain", F16, D, H, Hkv, S, page, lens, seed=52)
    for n in (1, 3):
        vck.splits(n)
        for is_causal, window in MASKS[:2]:
            kw = dict(is_causal=is_causal, window_size=window)
            o, lse = st.ragged(**kw)
            os, ls = rc.unpack(o, S), rc.unpack_lse(lse, S)
            for s in (1, 2):
                ids = [b for b in range(B) if S[b] == s]
                idx = torch.tensor(ids, device="cuda")
                ro, rl = _paged()(torch.cat([st.qs[b] for b in ids]), st.kp, st.vp, st.sl[idx].contiguous(),
                                  st.table[idx].contiguous(), return_lse=True, **kw)
                assert bc.same_bits(torch.cat([os[b] for b in ids]), ro), (n, is_causal, s)
                assert bc.same_bits(torch.cat([ls[b] for b in ids]), rl), (n, is_causal, s)
            assert (o[sum(S):] == SENT).all()


# ---- 6. strided q and out ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "fp8"])
def test_q_and_out_as_slices_of_wider_buffers(variant):
    page, D, H, Hkv = 64, 128, 8, 2
    st = Step(variant, BF16, D, H, Hkv, S_BASE, page, base_lens(page), seed=61)
    T = st.total
    qkv = torch.full((T, 3 * H * D), 3.0, dtype=BF16, device="cuda")             # a fused projection: q is its first third
    qkv[:, :H * D] = st.q.view(T, H * D)
    q = qkv[:, :H * D].view(T, H, D)
    wide = torch.full((T, 2 * H * D + 16), SENT, dtype=BF16, device="cuda")       # out: columns [16, 16 + H * D)
    out = wide[:, 16:16 + H * D].view(T, H, D)
    assert not q.is_contiguous() and not out.is_contiguous() and q.data_ptr() == qkv.data_ptr()
    for n in (1, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            wide.fill_(SENT)
            ref = st.ragged(**kw)
            got = st.ragged(q=q, out=out, **kw)
            assert bc.same_bits(out.contiguous(), ref[0]) and bc.same_bits(got[1][:, :sum(st.S)], ref[1][:, :sum(st.S)]), (n, is_causal)
            assert (wide[:, :16] == SENT).all() and (wide[:, 16 + H * D:] == SENT).all()
            assert (qkv[:, H * D:] == 3.0).all() and bc.same_bits(qkv[:, :H * D].contiguous().view(T, H, D), st.q)


# ---- 7. the append ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [32, 64])
@pytest.mark.parametrize("variant,dtype", [("plain", F16), ("plain", BF16), ("fp8", BF16), ("fp8_sink", F16)])
def test_packed_append_is_the_per_sequence_paged_append(variant, dtype, page):
    D, H, Hkv = 64, 8, 2
    S = [3, 0, 40, 1, 9]
    lens = [page - 1, 5, page - 20, 2 * page, 0]                # the new rows cross page boundaries; one sequence starts empty
    full = [L + s for L, s in zip(lens, S)]
    st = Step(variant, dtype, D, H, Hkv, S, page, lens, seed=71 + page, alloc=full)
    g = torch.Generator(device="cuda").manual_seed(72)
    new = [[torch.randn(1, Hkv, s, D, generator=g, device="cuda").to(dtype) for s in S] for _ in range(2)]
    kn, vn = (rc.pack(x, st.total).contiguous() for x in new)   # [total_q, H_kv, D]; NaN rows behind the last sequence
    for n in (1, 3):
        vck.splits(n)
        kr, vr, kp, vp = st.kp.clone(), st.vp.clone(), st.kp.clone(), st.vp.clone()
        refs = st.per_sequence(kr, vr, k_new=new[0], v_new=new[1], is_causal=True)
        got = st.ragged(kp, vp, k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        assert torch.equal(st.sl.cpu(), torch.tensor(lens, dtype=torch.int32))           # cache_seqlens is not modified
        assert not pc.same_bytes(kr, st.kp)                                               # the appends wrote something
        assert pc.same_bytes(kp, kr) and pc.same_bytes(vp, vr), n                         # the whole pool, byte for byte
        assert_rows(st, got, refs, n)
        assert torch.isfinite(got[0][:sum(S)]).all()


# ---- 8. graph replay --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "fp8_sink"])
def test_captured_step_replays_while_all_three_device_arrays_change(variant):
    page, D, H, Hkv = 64, 128, 8, 2
    S0 = [1, 4, 0, 7]                                                          # total_q = 12 rows, all in use at capture
    st = Step(variant, BF16, D, H, Hkv, S0, page, [3 * page] * 4, seed=81, pad=0)   # every page of the table in use
    T = st.total
    g = torch.Generator(device="cuda").manual_seed(82)
    st.q = torch.randn(T, H, D, generator=g, device="cuda").to(BF16)           # no NaN rows: any row may become a query
    kn, vn = (torch.randn(T, Hkv, D, generator=g, device="cuda").to(BF16) for _ in range(2))
    st.sl.copy_(torch.tensor([3, page - 1, 7, 2 * page - 3], dtype=torch.int32))
    k0, v0 = st.kp.clone(), st.vp.clone()
    out = torch.full((T, H, D), SENT, dtype=BF16, device="cuda")
    step = lambda kp, vp, o: st.ragged(kp, vp, out=o, k_new=kn, v_new=vn, is_causal=True)
    step(k0.clone(), v0.clone(), torch.empty_like(out))                        # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step(st.kp, st.vp, out)
    # another split of the same rows; fewer rows than total_q (the tail becomes padding); then lengths that fill pages
    steps = (([5, 0, 6, 1], [4, page, 2 * page + 1, 0]), ([2, 1, 1, 3], [page + 7, 2 * page - 1, 0, 3 * page - 3]),
             ([0, 12, 0, 0], [1, page - 5, 9, 9]))
    perm_gen = torch.Generator().manual_seed(83)
    for S, lens in steps:
        perm = torch.randperm(st.kp.shape[0], generator=perm_gen).cuda()       # every page moved, the table renumbered
        k0, v0 = pc.move_pages(k0, perm), pc.move_pages(v0, perm)
        st.kp.copy_(k0)
        st.vp.copy_(v0)
        st.table.copy_(perm[st.table.long()].to(torch.int32))
        st.sl.copy_(torch.tensor(lens, dtype=torch.int32))
        st.cu.copy_(rc.cu_of(S))
        used = sum(S)
        ke, ve, oe = k0.clone(), v0.clone(), torch.full_like(out, SENT)
        eager = step(ke, ve, oe)
        out.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        assert bc.same_bits(res[0], eager[0]) and bc.same_bits(res[1][:, :used], eager[1][:, :used]), (S, lens)
        assert (out[used:] == SENT).all() and torch.isfinite(out[:used]).all(), (S, lens)
        assert pc.same_bytes(st.kp, ke) and pc.same_bytes(st.vp, ve), (S, lens)           # the replayed append, too
        assert not pc.same_bytes(ke, k0)
        k0, v0 = ke, ve


# ---- 9. a malformed cu_seqlens_q ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "fp8_sink"])
def test_malformed_cu_seqlens_touch_nothing_outside_the_buffers(variant):
    """Safe by construction: every kernel takes S_b through one clamp (both ends of a sequence into [0, total_q], the
    second to the first), the plan stops at the bound the grid was sized by, and the append drops rows no sequence owns.
    So a malformed entry costs the sequences next to it their result and nothing else: the call returns, the bytes around
    O, LSE and the workspace are untouched, and the sequences whose own two entries are intact, and whose rows no other
    sequence claims, keep their bits."""
    page, D, H, Hkv = 64, 64, 8, 2
    st = Step(variant, F16, D, H, Hkv, S_BASE, page, base_lens(page), seed=91)
    T, good = st.total, rc.cu_of(S_BASE).tolist()                            # [0, 0, 1, 4, 44, 45, 54], T = 59
    cases = {   # name: (cu_seqlens_q, the sequences that keep their bits)
        "non-monotone": ([0, 0, 1, 4, 2, 45, 54], [1, 5]),                    # 3 ends before it starts; 4 claims [2, 45) over 2's rows
        "negative": ([0, 0, 1, -7, 44, 45, 54], [4, 5]),                      # 2 is empty; 3 claims [0, 44) over 1's row
        "beyond total_q": ([0, 0, 1, 4, 44, 45, 1 << 30], [1, 2, 3, 4]),      # 5 runs on to total_q, into the NaN rows
        "sum past total_q": ([0, T, 0, T, 0, T, T], []),                      # 3 * total_q rows claimed: the plan stops at NB_max
        "all past the end": ([T + 9] * 7, []),
        "int extremes": ([-(1 << 31), -5, 1, 4, 44, 45, (1 << 31) - 1], [1, 2, 3, 4]),   # 1 clamps to its own rows [0, 1)
    }
    for n in (1, 3):
        ref = raw_ragged(st, n, True)
        ro, rl = rc.unpack(ref[0], S_BASE), rc.unpack_lse(ref[1], S_BASE)
        for name, (cu, intact) in cases.items():
            o, lse, before, after, ranges = raw_ragged(st, n, True, cu=torch.tensor(cu, dtype=torch.int32, device="cuda"))
            assert_guards(before, after, ranges, (name, n))
            for b in intact:
                rows = slice(good[b], good[b + 1])
                assert bc.same_bits(o[rows].transpose(0, 1)[None].contiguous(), ro[b]), (name, n, b)
                assert bc.same_bits(lse[:, rows][None].contiguous(), rl[b]), (name, n, b)
    # the same through the Python call with an append: it returns, and nothing outside the pools' pages is there to write
    kn = torch.zeros(T, Hkv, D, dtype=F16, device="cuda")
    for name, (cu, _) in cases.items():
        st.cu = torch.tensor(cu, dtype=torch.int32, device="cuda")
        o, lse = st.ragged(st.kp.clone(), st.vp.clone(), k_new=kn, v_new=kn, is_causal=True)
        torch.cuda.synchronize()
        assert o.shape == (T, H, D) and lse.shape == (H, T)
