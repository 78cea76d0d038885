"""GPU tests of decoding attention over a paged KV cache (include/mi355fa_paged.h, paged_kvcache.flash_attention_kvcache_paged).

The oracle is the padded kernel: a paged call visits the same 32-key tiles in the same order with the same split shares,
so it must return THE BITS of the padded call on the gathered cache [B, H_kv, max_pages * page, D] -- for each of the six
variants (plain, soft cap, ALiBi, sinks over 16-bit caches; plain and sinks over e4m3 caches), at forced split counts, for
lengths around every tile and page boundary.  The plain variant is also held to fp64 on its own, with the bounds of
tests/test_gpu_kvcache.py.  Pools come from tests/pagedcheck.py: every unused page, every row past L_b in a last page and
every page an unused table entry names is NaN, and no entry is ever out of range, so a stray read shows as a NaN and never
as a fault.  Then: the append through the table (16-bit and fp8) against the padded append, a strided
[num_pages, page, H_kv, D] pool, a pool beyond 2^32 bytes, and a captured step replayed while cache_seqlens and
block_table change in place.  Shapes are the smallest that reach each path; every case runs in a few seconds."""
import pytest
import torch

import blockcheck as bc
import pagedcheck as pc
import test_gpu_kvcache as tk
import variantcheck as vck

pytestmark = pytest.mark.gpu

F16, BF16, E4M3 = torch.float16, torch.bfloat16, torch.float8_e4m3fn
GROUPS = [(4, 4), (8, 2), (8, 1)]
MASKS = tk.MASKS                         # full, causal, window (40, 8)
SPLITS = (0, 1, 3, 7)
VARIANTS = ("plain", "softcap", "alibi", "sink", "fp8", "fp8_sink")
MAX_PAGES = 3


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def _paged():
    import paged_kvcache as P
    return P.flash_attention_kvcache_paged


def lengths(page):
    """around every tile and page boundary, from the empty sequence to the full table"""
    return sorted({0, 1, 31, 32, 33, page - 1, page, page + 1, 2 * page + 5, MAX_PAGES * page})


class Case:
    """One batch of sequences of `lens` keys as a padded cache (NaN past each length, as gathered) and as a pool + table,
    with the arguments of one variant for the paged call and for the padded call it must reproduce."""

    def __init__(self, variant, dtype, D, H, Hkv, Sq, page, lens, seed, alloc=None, amp=1.0, max_pages=MAX_PAGES):
        self.variant, self.lens, self.page = variant, list(lens), page
        B = len(lens)
        S = max_pages * page
        g = torch.Generator(device="cuda").manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g, device="cuda")
        self.q = (r(B, H, Sq, D) * amp).to(dtype)
        fp8 = variant.startswith("fp8")
        kc, vc = ((r(B, Hkv, S, D) * (2.0 if fp8 else 1.0)).to(E4M3 if fp8 else dtype) for _ in range(2))
        pages = sum(pc.pages_of(L, page) for L in (alloc or lens))
        (self.kp, self.vp), self.table = pc.scatter([kc, vc], lens, page, pages + 5, max_pages, seed, alloc=alloc)
        self.kc, self.vc = pc.gather(self.kp, self.table), pc.gather(self.vp, self.table)
        self.sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        self.mods = {}
        if variant == "softcap":
            self.mods = dict(softcap=15.0)
        elif variant == "alibi":
            self.mods = dict(alibi_slopes=torch.rand(H, generator=g, device="cuda") * 0.5 + 0.01)
        elif variant in ("sink", "fp8_sink"):
            self.mods = dict(sinks=r(H))
        if fp8:
            self.mods.update(k_descale=torch.rand(B, Hkv, generator=g, device="cuda") + 0.5,
                             v_descale=torch.rand(Hkv, generator=g, device="cuda") + 0.5)

    def paged(self, kp=None, vp=None, **kw):
        return _paged()(self.q, self.kp if kp is None else kp, self.vp if vp is None else vp, self.sl, self.table,
                        return_lse=True, **self.mods, **kw)

    def padded(self, kc=None, vc=None, **kw):
        M = vck.M()
        kc, vc = self.kc if kc is None else kc, self.vc if vc is None else vc
        m = self.mods
        f, extra = {"plain": (M.flash_attention_kvcache, ()),
                    "softcap": (M.flash_attention_kvcache_softcap, (m.get("softcap"),)),
                    "alibi": (M.flash_attention_kvcache_alibi, (m.get("alibi_slopes"),)),
                    "sink": (M.flash_attention_kvcache_sink, (m.get("sinks"),)),
                    "fp8": (M.flash_attention_kvcache_fp8, ()),
                    "fp8_sink": (M.flash_attention_kvcache_fp8_sink, (m.get("sinks"),))}[self.variant]
        if self.variant.startswith("fp8"):
            kw = dict(kw, k_descale=m["k_descale"], v_descale=m["v_descale"])
        return f(self.q, kc, vc, self.sl, *extra, return_lse=True, **kw)


def assert_same(a, b, what):
    assert bc.same_bits(a[0], b[0]), ("O", what)
    assert bc.same_bits(a[1], b[1]), ("LSE", what)


# ---- 1. the bits of the padded kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [32, 64, 256])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("variant", VARIANTS)
def test_paged_call_has_the_bits_of_the_padded_call(variant, D, dtype, page):
    for H, Hkv in GROUPS:
        for Sq in (1, 3, 40):
            c = Case(variant, dtype, D, H, Hkv, Sq, page, lengths(page), seed=D + Sq + H + page)
            for is_causal, window in MASKS:
                for n in SPLITS:
                    vck.splits(n)
                    what = (H, Hkv, Sq, is_causal, window, n)
                    kw = dict(is_causal=is_causal, window_size=window)
                    ref = c.padded(**kw)
                    got = c.paged(**kw)
                    assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), what
                    assert_same(got, ref, what)
                    assert_same(c.paged(**kw), got, what)                 # and its own bits again


# ---- 2. accuracy on its own --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [32, 64, 256])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_plain_variant_matches_fp64(D, dtype, page):
    for H, Hkv in GROUPS:
        for Sq in (1, 3, 40):
            c = Case("plain", dtype, D, H, Hkv, Sq, page, lengths(page), seed=7 + D + Sq + H)
            for is_causal, window in MASKS:
                wl, wr = tk.window_of(is_causal, window)
                O_ref, LSE_ref = tk.ref_fp64(c.q, c.kc, c.vc, c.lens, wl, wr)
                bound = tk.tol(dtype, c.q, c.kc, c.vc, c.lens, wl, wr, O_ref)
                for n in (0, 3):
                    vck.splits(n)
                    o, lse = c.paged(is_causal=is_causal, window_size=window)
                    err = tk.rel(o, O_ref)
                    assert err < bound, (H, Hkv, Sq, is_causal, window, n, err, bound)
                    tk.check_lse(lse, LSE_ref)
                    assert (o[torch.isinf(LSE_ref)] == 0).all()


# ---- 3. nothing unused is read -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "fp8"])
def test_nan_pages_rows_and_table_entries_are_never_read(variant):
    page, D = 64, 128
    c = Case(variant, BF16, D, 8, 2, 3, page, lengths(page), seed=11)
    assert torch.isnan(c.kp.float()).any() and torch.isnan(c.kc.float()).any()       # the fill is there to be found
    for n in SPLITS:
        vck.splits(n)
        for is_causal, window in MASKS:
            o, lse = c.paged(is_causal=is_causal, window_size=window)
            assert torch.isfinite(o).all() and not torch.isnan(lse).any(), (n, is_causal, window)


def test_sequences_that_share_prefix_pages_keep_their_own_results():
    page, D, H, Hkv = 64, 64, 8, 2
    lens = [page + 40, 2 * page + 5]                      # one shared page, then each its own
    c = Case("plain", F16, D, H, Hkv, 3, page, lens, seed=13)
    kc, vc = pc.gather(c.kp, c.table, lens), pc.gather(c.vp, c.table, lens)
    kc[1, :, :page], vc[1, :, :page] = kc[0, :, :page], vc[0, :, :page]               # the common prefix
    table = torch.tensor([[2, 4, 0], [2, 5, 6]], dtype=torch.int32)                   # page 0 stays NaN
    (c.kp, c.vp), c.table = pc.scatter([kc, vc], lens, page, 8, MAX_PAGES, 0, table=table)
    c.kc, c.vc = pc.gather(c.kp, c.table), pc.gather(c.vp, c.table)
    for n in SPLITS:
        vck.splits(n)
        got = c.paged(is_causal=True)
        assert_same(got, c.padded(is_causal=True), n)
        for b in range(2):                                # each sequence alone, through a one-row table
            one = Case.__new__(Case)
            one.__dict__.update(c.__dict__, q=c.q[b:b + 1], sl=c.sl[b:b + 1], table=c.table[b:b + 1].contiguous())
            o, lse = one.paged(is_causal=True)
            assert bc.same_bits(o[0], got[0][b]) and bc.same_bits(lse[0], got[1][b]), (n, b)


# ---- 4. the append -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [32, 64])
@pytest.mark.parametrize("variant,dtype", [("plain", F16), ("plain", BF16), ("fp8", BF16), ("fp8_sink", F16)])
def test_append_through_the_table_is_the_padded_append(variant, dtype, page):
    D, H, Hkv, Sq, Snew = 64, 8, 2, 3, 3
    lens = [0, page - 1, page, 2 * page - 2]              # the new rows cross page boundaries
    full = [L + Snew for L in lens]
    c = Case(variant, dtype, D, H, Hkv, Sq, page, lens, seed=17 + page, alloc=full)
    g = torch.Generator(device="cuda").manual_seed(18)
    kn, vn = (torch.randn(len(lens), Hkv, Snew, D, generator=g, device="cuda").to(dtype) for _ in range(2))
    for n in (0, 3):
        vck.splits(n)
        kc, vc, kp, vp = c.kc.clone(), c.vc.clone(), c.kp.clone(), c.vp.clone()
        ref = c.padded(kc, vc, k_new=kn, v_new=vn, is_causal=True)
        got = c.paged(kp, vp, k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        assert torch.equal(c.sl.cpu(), torch.tensor(lens, dtype=torch.int32))        # cache_seqlens is not modified
        assert not pc.same_bytes(kc, c.kc)                                            # the padded append wrote something
        # the whole pool: the new rows where the table sends them, every other page and row untouched
        (kx, vx), _ = pc.scatter([kc, vc], full, page, kp.shape[0], MAX_PAGES, 0, table=c.table.cpu())
        assert pc.same_bytes(kp, kx) and pc.same_bytes(vp, vx), n
        assert_same(got, ref, n)
        assert torch.isfinite(got[0]).all()
        if not variant.startswith("fp8"):                                             # attention sees the new keys
            O_ref, LSE_ref = tk.ref_fp64(c.q, kc, vc, full, -1, 0)
            assert tk.rel(got[0], O_ref) < tk.tol(dtype, c.q, kc, vc, full, -1, 0, O_ref)
            tk.check_lse(got[1], LSE_ref)
            old, _ = c.paged(is_causal=True)                                          # the step before: other keys
            assert tk.rel(old, O_ref) > 10 * tk.rel(got[0], O_ref)


# ---- 5. a strided pool ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "fp8"])
def test_page_major_pool_is_read_and_appended_in_place(variant):
    page, D, H, Hkv, Snew = 64, 128, 8, 2, 2
    lens = [5, page - 1, 2 * page + 5]
    full = [L + Snew for L in lens]
    c = Case(variant, BF16, D, H, Hkv, 3, page, lens, seed=19, alloc=full)
    kt, vt = (x.transpose(1, 2).contiguous().transpose(1, 2) for x in (c.kp, c.vp))   # [num_pages, page, H_kv, D] storage
    assert not kt.is_contiguous() and kt.stride(2) == Hkv * D
    for is_causal, window in MASKS:
        kw = dict(is_causal=is_causal, window_size=window)
        assert_same(c.paged(kt, vt, **kw), c.paged(**kw), (is_causal, window))
    g = torch.Generator(device="cuda").manual_seed(20)
    kn, vn = (torch.randn(len(lens), Hkv, Snew, D, generator=g, device="cuda").to(BF16) for _ in range(2))
    kp, vp = c.kp.clone(), c.vp.clone()
    a = c.paged(kp, vp, k_new=kn, v_new=vn)
    b = c.paged(kt, vt, k_new=kn, v_new=vn)
    assert_same(a, b, "append")
    assert pc.same_bytes(kt.contiguous(), kp) and pc.same_bytes(vt.contiguous(), vp)
    assert not pc.same_bytes(kp, c.kp)


# ---- 6. a pool beyond 2^32 bytes -----------------------------------------------------------------------------------------------
def test_pages_at_the_top_of_a_pool_beyond_4_gib():
    page, D, H, Hkv, Sq = 32, 64, 4, 1, 3
    lens = [2 * page + 5]
    c = Case("plain", BF16, D, H, Hkv, Sq, page, lens, seed=23)
    num_pages = (1 << 32) // (page * D * 2) + 64                                      # 2^32 bytes and 64 pages more
    try:
        big_k, big_v = (torch.empty(num_pages, Hkv, page, D, dtype=BF16, device="cuda") for _ in range(2))
    except RuntimeError as e:                                                         # (torch.OutOfMemoryError is one)
        pytest.skip("no room for two pools of %d bytes: %s" % (num_pages * page * D * 2, str(e)[:80]))
    assert big_k.numel() * 2 > 1 << 32
    top = torch.tensor([[num_pages - 1, num_pages - 3, num_pages - 2]], dtype=torch.int32, device="cuda")
    for i in range(MAX_PAGES):                                                        # only these pages are ever initialised
        big_k[int(top[0, i])], big_v[int(top[0, i])] = c.kp[int(c.table[0, i])], c.vp[int(c.table[0, i])]
    small = c.paged(is_causal=True)
    c.table = top
    for n in (0, 3):
        vck.splits(n)
        assert_same(c.paged(big_k, big_v, is_causal=True), small if n == 0 else c.padded(is_causal=True), n)
    kn, vn = (torch.ones(1, Hkv, 2, D, dtype=BF16, device="cuda") * s for s in (0.5, -0.25))
    c.paged(big_k, big_v, k_new=kn, v_new=vn)                                         # the append reaches the top pages too
    row = lens[0] - 2 * page
    assert (big_k[num_pages - 2, :, row:row + 2] == 0.5).all() and (big_v[num_pages - 2, :, row:row + 2] == -0.25).all()


# ---- 7. graph replay -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "fp8_sink"])
def test_captured_step_replays_while_seqlens_and_table_change_in_place(variant):
    page, D, H, Hkv, Snew = 64, 128, 8, 2, 1
    lens = [3, page - 1, 2 * page]
    steps = ([4, page, 2 * page + 1], [page + 7, 2 * page - 1, 3 * page - 1], [0, 1, page])
    c = Case(variant, BF16, D, H, Hkv, 1, page, [3 * page] * 3, seed=29)              # every page of the table in use
    c.sl.copy_(torch.tensor(lens, dtype=torch.int32))
    g = torch.Generator(device="cuda").manual_seed(30)
    kn, vn = (torch.randn(3, Hkv, Snew, D, generator=g, device="cuda").to(BF16) for _ in range(2))
    k0, v0 = c.kp.clone(), c.vp.clone()
    step = lambda kp, vp: c.paged(kp, vp, k_new=kn, v_new=vn, is_causal=True)
    step(k0.clone(), v0.clone())                                                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(c.kp, c.vp)
    perm_gen = torch.Generator().manual_seed(31)
    for new_lens in steps:
        # other lengths, and every page moved: the pool permuted and the table renumbered to match, all in place
        perm = torch.randperm(c.kp.shape[0], generator=perm_gen).cuda()               # old page -> new page
        k0, v0 = pc.move_pages(k0, perm), pc.move_pages(v0, perm)
        c.kp.copy_(k0)
        c.vp.copy_(v0)
        c.table.copy_(perm[c.table.long()].to(torch.int32))
        c.sl.copy_(torch.tensor(new_lens, dtype=torch.int32))
        ke, ve = k0.clone(), v0.clone()
        eager = step(ke, ve)
        graph.replay()
        torch.cuda.synchronize()
        assert_same(out, eager, new_lens)
        assert pc.same_bytes(c.kp, ke) and pc.same_bytes(c.vp, ve), new_lens           # the replayed append, too
        assert not pc.same_bytes(ke, k0)
        k0, v0 = ke, ve
