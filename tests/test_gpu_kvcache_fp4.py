"""GPU tests of decoding attention over an MXFP4 KV cache (include/mi355fa_kvcache_fp4.h; fp4_kvcache.py), padded and paged.

The truth is tests/attn_ref.py in fp64 on the dequantised cache (dequantize_kv_mxfp4 in fp64: e2m1(nibble) * 2^(scale - 127)),
so quantisation error is not in the comparison: the kernel's conversions are exact for these scales and it makes the 16-bit
kernel's rounding errors only.  Every (sequence, head) is held on its own to the project's per-head decode bounds, relative
Frobenius 1e-3 (fp16) / 8e-3 (bf16), and LSE to rtol 1e-3 / atol 2e-3 (tests/test_gpu_kvcache.py check_lse).

Inputs: uniformly random nibbles (all 16 codes, so V rows are distinct), scale bytes that differ per (row, block), spread
over 127 +- 6 and drawn separately for K and V: a wrong block-to-scale or nibble-order mapping moves a result by far more
than the bound.  q is scaled so that the scores stay of order one and many keys carry weight.  Shapes are the smallest that
reach each path: a 32-key tile, four key groups per workgroup, 32 MFMA rows per row block."""
import pytest
import torch

import attn_ref as ar
import fa_oracle as fo
import variantcheck as vck
from test_gpu_kvcache import check_lse

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DT = [F16, BF16]
IDS = ["fp16", "bf16"]
BOUND = {F16: 1e-3, BF16: 8e-3}
LENS = [1, 31, 32, 33, 129, 200]            # around one tile, past four tiles (one step of the workgroup), and 7 tiles
SC = 224
GEOMS = [(4, 2, 1), (4, 2, 3), (5, 1, 1), (5, 1, 3), (8, 1, 5)]    # (H, H_kv, S_q): odd group; 40 rows = two row blocks
MASKS = [(False, (-1, -1)), (True, (-1, -1)), (False, (40, 0))]     # full, causal, window (40, 0)
FF = 0xFF                                    # the poison byte: the NaN scale, and nibbles -6, -6


def _F():
    import fp4_kvcache as F
    return F


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def make4(B, H, Hkv, Sq, Sc, D, dtype, seed=0):
    """q, k_cache, v_cache (random nibbles), k_scale, v_scale (127 +- 6 per (row, block), K and V drawn separately)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
    kc, vc = ri(0, 256, B, Hkv, Sc, D // 2), ri(0, 256, B, Hkv, Sc, D // 2)
    ks, vs = ri(121, 134, B, Hkv, Sc, D // 32), ri(121, 134, B, Hkv, Sc, D // 32)
    assert not torch.equal(ks, vs) and ks.unique().numel() == 13 and (ks[..., 0] != ks[..., 1]).any()
    # |K| is about 2.7 * 2^3 on average: scores of order one at the default 1 / sqrt(D) scale
    q = (torch.randn(B, H, Sq, D, generator=g, device="cuda") * 0.03).to(dtype)
    return q, kc, vc, ks, vs


def deq64(packed, scales):
    return _F().dequantize_kv_mxfp4(packed, scales, torch.float32).double()      # exact in fp32, then widened


def truth(q, K, V, lens, wl, wr, sinks=None, scale=None):
    """O [B, H, S_q, D] and LSE [B, H, S_q] in fp64, per sequence on K / V sliced to L_b"""
    B, H, Sq, D = q.shape
    scale = D ** -0.5 if scale is None else scale
    O = torch.zeros(B, H, Sq, D, dtype=torch.float64, device=q.device)
    LSE = torch.empty(B, H, Sq, dtype=torch.float64, device=q.device)
    for b, L in enumerate(lens):
        r = ar.attention_fp64(q[b:b + 1], K[b:b + 1, :, :L], V[b:b + 1, :, :L], None, scale,
                              ar.visible(Sq, L, wl, wr, q.device, L=L), sinks=sinks)
        O[b], LSE[b] = r["O"][0], r["LSE"][0]
    return O, LSE


def check(tag, q, o, lse, O_ref, LSE_ref):
    B, H, Sq, D = q.shape
    assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == (B, H, Sq) and lse.dtype == torch.float32
    assert torch.isfinite(o).all()
    err = fo.block_errors(O_ref, o, block=Sq)[..., 0]                            # [B, H]: every (sequence, head) on its own
    at = tuple(int(x) for x in torch.unravel_index(err.argmax(), err.shape))
    print(tag, "worst (b, h)", at, "relFro %.3e (bound %.0e)" % (err[at].item(), BOUND[q.dtype]))
    assert (err < BOUND[q.dtype]).all(), (tag, at, err[at].item())
    check_lse(lse, LSE_ref)


def window_of(is_causal, window):
    return (window[0], 0) if is_causal else window


def same(a, b):
    return all(torch.equal(x.view(torch.int16) if x.element_size() == 2 else x, y.view(torch.int16) if y.element_size() == 2 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv,Sq", GEOMS)
def test_matches_fp64_per_head(H, Hkv, Sq, D, dtype):
    F = _F()
    B = len(LENS)
    q, kc, vc, ks, vs = make4(B, H, Hkv, Sq, SC, D, dtype, seed=H + Sq + D)
    K, V = deq64(kc, ks), deq64(vc, vs)
    sl = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    sinks = torch.linspace(-1.0, 3.0, H, device="cuda", dtype=torch.float32)
    for is_causal, window in MASKS:
        wl, wr = window_of(is_causal, window)
        for sk in (None, sinks):
            O_ref, LSE_ref = truth(q, K, V, LENS, wl, wr, sk)
            for n in (1, 2, 3):
                vck.splits(n)
                o, lse = F.flash_attention_kvcache_fp4(q, kc, vc, ks, vs, sl, is_causal=is_causal, window_size=window,
                                                       return_lse=True, sinks=sk)
                torch.cuda.synchronize()
                check("causal=%s window=%s sinks=%s n=%d" % (is_causal, window, sk is not None, n), q, o, lse, O_ref, LSE_ref)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_nibble_order_and_block_scales_element_for_element(dtype):
    """One key, one query that is a unit vector: the score picks K[d] out, and with a single key O is V itself.  Element d of
    the row must come from nibble d % 2 of byte d // 2 with the scale of block d // 32 -- held exactly on V (O = V, every
    product representable) and through LSE on K."""
    F = _F()
    for D in (64, 128):
        kc = (torch.arange(D // 2, device="cuda", dtype=torch.int32) * 37 % 256).to(torch.uint8).view(1, 1, 1, D // 2).contiguous()
        vc = (torch.arange(D // 2, device="cuda", dtype=torch.int32) * 91 % 256 ^ 0x5A).to(torch.uint8).view(1, 1, 1, D // 2).contiguous()
        ks = torch.tensor([125, 129, 126, 131][:D // 32], dtype=torch.uint8, device="cuda").view(1, 1, 1, -1)
        vs = torch.tensor([130, 124, 128, 127][:D // 32], dtype=torch.uint8, device="cuda").view(1, 1, 1, -1)
        pad = lambda t: torch.cat([t, torch.full((1, 1, 31, t.shape[-1]), FF, dtype=torch.uint8, device="cuda")], dim=2)
        K, V = deq64(kc, ks)[0, 0, 0], deq64(vc, vs)[0, 0, 0]
        assert V.unique().numel() >= 12 and K.unique().numel() >= 12
        q = torch.eye(D, device="cuda", dtype=dtype).view(1, D, 1, D)           # head h asks for element h
        sl = torch.ones(1, dtype=torch.int32, device="cuda")
        o, lse = F.flash_attention_kvcache_fp4(q, pad(kc), pad(vc), pad(ks), pad(vs), sl, softmax_scale=1.0, return_lse=True)
        assert torch.equal(o.double(), V.expand(1, D, 1, D)), "O = V: nibble order or V block scales"
        # LSE = the one score = K[d], through the kernel's log2 units: a wrong nibble or scale is off by 1e-3 of the largest |K| at least
        assert torch.allclose(lse[0, :, 0].double(), K, rtol=1e-5, atol=1e-5), "nibble order or K block scales"


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_poison_past_the_fill_level_is_never_read(D, dtype):
    F = _F()
    B, H, Hkv, Sq = len(LENS), 4, 2, 3
    q, kc, vc, ks, vs = make4(B, H, Hkv, Sq, SC, D, dtype, seed=5)
    sl = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    poisoned = [t.clone() for t in (kc, vc, ks, vs)]
    for b, L in enumerate(LENS):
        for t in poisoned:
            t[b, :, L:] = FF
    K, V = deq64(kc, ks), deq64(vc, vs)
    for n in (1, 2, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            a = F.flash_attention_kvcache_fp4(q, kc, vc, ks, vs, sl, is_causal=is_causal, window_size=window, return_lse=True)
            b = F.flash_attention_kvcache_fp4(q, *poisoned, sl, is_causal=is_causal, window_size=window, return_lse=True)
            assert torch.isfinite(b[0]).all() and not torch.isnan(b[1]).any()
            assert same(a, b), (n, is_causal, window)
            check("poison n=%d" % n, q, b[0], b[1], *truth(q, K, V, LENS, *window_of(is_causal, window)))


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_transposed_storage_is_read_in_place_bit_for_bit(D, dtype):
    F = _F()
    B, H, Hkv, Sq = len(LENS), 4, 2, 3
    q, kc, vc, ks, vs = make4(B, H, Hkv, Sq, SC, D, dtype, seed=9)
    tr = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)      # [B, S, H_kv, .] storage seen as [B, H_kv, S, .]
    kt, vt, kst, vst = (tr(t) for t in (kc, vc, ks, vs))
    assert not kt.is_contiguous() and kt.stride(2) == Hkv * D // 2 and kst.stride(2) == Hkv * D // 32
    sl = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    for is_causal, window in MASKS:
        a = F.flash_attention_kvcache_fp4(q, kc, vc, ks, vs, sl, is_causal=is_causal, window_size=window, return_lse=True)
        b = F.flash_attention_kvcache_fp4(q, kt, vt, kst, vst, sl, is_causal=is_causal, window_size=window, return_lse=True)
        assert same(a, b)
    # the append writes the transposed storage in place
    g = torch.Generator(device="cuda").manual_seed(10)
    kn = torch.randn(B, Hkv, 2, D, generator=g, device="cuda").to(dtype)
    vn = torch.randn(B, Hkv, 2, D, generator=g, device="cuda").to(dtype)
    a = F.flash_attention_kvcache_fp4(q, kc, vc, ks, vs, sl, k_new=kn, v_new=vn, return_lse=True)
    b = F.flash_attention_kvcache_fp4(q, kt, vt, kst, vst, sl, k_new=kn, v_new=vn, return_lse=True)
    for x, y in ((kc, kt), (vc, vt), (ks, kst), (vs, vst)):
        assert torch.equal(x, y.contiguous())
    assert same(a, b)


def append_inputs(B, Hkv, Snew, D, dtype, seed):
    """k_new / v_new with magnitudes over many binades inside a row, signed zeros, a zero block and exact ties"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mag = torch.exp2(torch.randint(-8, 9, (B, Hkv, Snew, D // 32, 1), generator=g, device="cuda").float())
    mk = lambda: (torch.randn(B, Hkv, Snew, D // 32, 32, generator=g, device="cuda") * mag).reshape(B, Hkv, Snew, D).to(dtype)
    kn, vn = mk(), mk()
    kn[:, :, 0, 0], kn[:, :, 0, 1], vn[:, :, 0, 2], vn[:, :, 0, 3] = 0.0, -0.0, -0.0, 0.0
    kn[:, :, -1, 32:64] = 0.0                                                   # an all-zero block
    ties = torch.tensor([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, 7.0],
                        device="cuda")
    vn[:, :, -1, 0:16] = (ties * 8).to(dtype)                                   # the block's amax is 7 * 8: X = 3
    return kn, vn


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_append_writes_exactly_the_quantised_new_rows(D, dtype):
    F = _F()
    B, H, Hkv, Sq, Snew = 4, 4, 2, 3, 3
    lens = [0, 30, 100, SC - Snew]                                              # the last one fills the cache to its end
    q, kc, vc, ks, vs = make4(B, H, Hkv, Sq, SC, D, dtype, seed=7)
    kn, vn = append_inputs(B, Hkv, Snew, D, dtype, 8)
    before = [t.clone() for t in (kc, vc, ks, vs)]
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    o, lse = F.flash_attention_kvcache_fp4(q, kc, vc, ks, vs, sl, k_new=kn, v_new=vn, is_causal=True, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(sl.cpu(), torch.tensor(lens, dtype=torch.int32))         # cache_seqlens is not modified
    (kq, kqs), (vq, vqs) = F.quantize_kv_mxfp4(kn.cpu()), F.quantize_kv_mxfp4(vn.cpu())      # the expected bytes, on the CPU
    assert (kq == 0x80).any() or ((kq & 0x0F) == 8).any() or ((kq >> 4) == 8).any()            # a -0.0 nibble is there
    want = [t.clone() for t in before]
    for b, L in enumerate(lens):
        for t, new in zip(want, (kq, vq, kqs, vqs)):
            t[b, :, L:L + Snew] = new[b].cuda()
    for name, got, w in zip(("k_cache", "v_cache", "k_scale", "v_scale"), (kc, vc, ks, vs), want):
        assert torch.equal(got, w), (name, int((got != w).sum()))
    # and the helper builds the same bytes on the device
    assert torch.equal(F.quantize_kv_mxfp4(kn)[0].cpu(), kq) and torch.equal(F.quantize_kv_mxfp4(vn)[1].cpu(), vqs)
    full = torch.tensor([L + Snew for L in lens], dtype=torch.int32, device="cuda")
    o2, lse2 = F.flash_attention_kvcache_fp4(q, *want, full, is_causal=True, return_lse=True)
    assert same((o, lse), (o2, lse2))
    check("append", q, o, lse, *truth(q, deq64(want[0], want[2]), deq64(want[1], want[3]), full.tolist(), -1, 0))


# ---------------------------------------------------------------- paged
def scatter4(tensors, lens, page, num_pages, max_pages, seed):
    """The padded byte tensors [B, H_kv, S, w] as pools [num_pages, H_kv, page, w] under one permuted table; every byte no
    sequence owns is 0xFF.  The table's entries past a sequence's pages name pages no sequence uses."""
    B = tensors[0].shape[0]
    used = [-(-L // page) for L in lens]
    assert sum(used) < num_pages and max(used) <= max_pages
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    spare = perm[sum(used):]
    table = torch.empty(B, max_pages, dtype=torch.int32)
    at = 0
    for b in range(B):
        for i in range(max_pages):
            table[b, i] = perm[at + i] if i < used[b] else spare[(b + i) % len(spare)]
        at += used[b]
    pools = []
    for t in tensors:
        pool = torch.full((num_pages, t.shape[1], page, t.shape[3]), FF, dtype=torch.uint8, device=t.device)
        for b, L in enumerate(lens):
            for i in range(used[b]):
                n = min(page, L - i * page)
                pool[int(table[b, i]), :, :n] = t[b, :, i * page:i * page + n]
        pools.append(pool)
    return pools, table.cuda()


def wide(table):
    """the table as a strided view: columns [3, 3 + max_pages) of a wider tensor whose other columns are out of range"""
    B, mp = table.shape
    w = torch.full((B, mp + 7), 1 << 20, dtype=torch.int32, device=table.device)
    w[:, 3:3 + mp] = table
    return w[:, 3:3 + mp]


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("page", [32, 96])
def test_paged_has_the_bits_of_the_padded_call_on_the_gathered_cache(page, D, dtype):
    F = _F()
    H, Hkv, Sq, Snew = 4, 2, 3, 3
    MP = -(-SC // page)
    reach = MP * page
    # fill levels: mid-page, a page boundary inside an append (page - 1 -> page + 2), the table's end with the append
    lens = [1, page - 1, 129, reach - Snew, 40, 0]
    B = len(lens)
    q, kc, vc, ks, vs = make4(B, H, Hkv, Sq, reach, D, dtype, seed=11 + page)
    kn, vn = append_inputs(B, Hkv, Snew, D, dtype, 12)
    after = [L + Snew for L in lens]
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    NP = sum(-(-L // page) for L in after) + 4
    for n in (1, 2, 3):
        vck.splits(n)
        pad = [t.clone() for t in (kc, vc, ks, vs)]
        for b, L in enumerate(lens):
            for t in pad:
                t[b, :, L:] = FF
        # pools that hold the rows below the fill level, with pages allotted for the appended rows too
        pools, table = scatter4(pad, after, page, NP, MP, seed=page + n)
        for b, L in enumerate(lens):                                            # (scatter4 copied the poison rows [L, L + Snew) too)
            assert (pools[2][int(table[b, L // page]), :, L % page] == FF).all()
        for is_causal, window in MASKS:
            a_t = [t.clone() for t in pad]
            p_t = [t.clone() for t in pools]
            kw = dict(k_new=kn, v_new=vn, is_causal=is_causal, window_size=window, return_lse=True)
            a = F.flash_attention_kvcache_fp4(q, *a_t, sl, **kw)
            b = F.flash_attention_kvcache_fp4_paged(q, *p_t, sl, wide(table), **kw)
            assert same(a, b), (n, is_causal, window)
            # the pools after the append are the padded caches after theirs, page by page; every other byte is untouched
            want, _ = scatter4(a_t, after, page, NP, MP, seed=page + n)
            for name, got, w in zip(("k_cache", "v_cache", "k_scale", "v_scale"), p_t, want):
                assert torch.equal(got, w), (name, int((got != w).sum()))
        K, V = deq64(a_t[0], a_t[2]), deq64(a_t[1], a_t[3])
        check("paged page=%d n=%d" % (page, n), q, b[0], b[1], *truth(q, K, V, after, *window_of(*MASKS[-1])))


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_out_of_range_table_entries_touch_nothing_outside_the_pools(dtype):
    """Out-of-range entries below ceil(L / page_size), inside guarded pools: that sequence's result is unspecified but finite,
    the other sequences' results are unchanged and no guard byte is written.  Not a fault test: the kernels clamp such an
    entry to an empty page and the append drops the row."""
    F = _F()
    D, page, H, Hkv, Sq, Snew = 128, 32, 4, 2, 1, 2
    lens = [70, 100, 33, 63]                                                    # the last one: the append crosses into page 2
    B, MP, G = len(lens), 5, 3
    q, kc, vc, ks, vs = make4(B, H, Hkv, Sq, MP * page, D, dtype, seed=13)
    after = [L + Snew for L in lens]
    NP = sum(-(-L // page) for L in after) + 2
    pools, table = scatter4([kc, vc, ks, vs], after, page, NP, MP, seed=14)
    kn, vn = append_inputs(B, Hkv, Snew, D, dtype, 15)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")

    def guarded(pool):
        big = torch.full((NP + 2 * G, *pool.shape[1:]), FF, dtype=torch.uint8, device="cuda")
        big[G:G + NP] = pool
        return big

    def run(tab):
        bigs = [guarded(p) for p in pools]
        out = F.flash_attention_kvcache_fp4_paged(q, *(b[G:G + NP] for b in bigs), sl, tab, k_new=kn, v_new=vn, return_lse=True)
        torch.cuda.synchronize()
        for b in bigs:
            assert (b[:G] == FF).all() and (b[G + NP:] == FF).all(), "a guard byte was written"
        return out, bigs

    good, good_pools = run(table)
    bad = table.clone()
    bad[1, 0], bad[1, 2], bad[3, 2] = NP + 1, -1, 1 << 30                        # read entries, and the page the append of 3 goes to
    (o, lse), bad_pools = run(bad)
    assert torch.isfinite(o).all() and not torch.isnan(lse).any()
    for b in (0, 2):
        assert same((o[b], lse[b]), (good[0][b], good[1][b])), b
    # sequence 3's appended rows: row 63 lands in its page 1, row 64 would land in the entry that is out of range and is
    # dropped; every page that is not one of sequences 1 and 3 holds what the run with the good table left there
    theirs = torch.zeros(NP, dtype=torch.bool)
    for b in (1, 3):
        for i in range(-(-after[b] // page)):
            theirs[int(table[b, i])] = True
    for gp, bp in zip(good_pools, bad_pools):
        assert torch.equal(gp[G:G + NP][~theirs], bp[G:G + NP][~theirs]), "a page of another sequence changed"


def test_graph_captured_step_replays_after_seqlens_advance():
    F = _F()
    B, H, Hkv, Sq, D, Snew, dtype = 4, 8, 2, 1, 128, 1, BF16
    lens = [5, 100, 31, 200]
    q, kc, vc, ks, vs = make4(B, H, Hkv, Sq, SC, D, dtype, seed=19)
    g = torch.Generator(device="cuda").manual_seed(20)
    kn = torch.randn(B, Hkv, Snew, D, generator=g, device="cuda").to(dtype)
    vn = torch.randn(B, Hkv, Snew, D, generator=g, device="cuda").to(dtype)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    vck.splits(2)                                                               # the combine kernel is in the graph too
    caches = (kc, vc, ks, vs)

    def eager():
        c = [t.clone() for t in caches]
        o = F.flash_attention_kvcache_fp4(q, *c, sl.clone(), k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        return o, c

    eager()                                                                     # warm-up (allocator)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = F.flash_attention_kvcache_fp4(q, *caches, sl, k_new=kn, v_new=vn, is_causal=True)
    for step in range(3):
        o_e, c_e = eager()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), o_e.view(torch.int16)), step
        assert all(torch.equal(a, b) for a, b in zip(caches, c_e)), step
        sl += Snew                                                              # advance in place; the new token's q / k / v
        q.copy_((torch.randn(q.shape, generator=g, device="cuda") * 0.03).to(dtype))
        kn.copy_(torch.randn(kn.shape, generator=g, device="cuda").to(dtype))
        vn.copy_(torch.randn(vn.shape, generator=g, device="cuda").to(dtype))
