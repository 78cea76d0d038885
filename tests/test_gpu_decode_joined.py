"""GPU test of the decode launch path the three cache formats share (csrc/fa_decode.hip launch_decode_t / launch_append /
launch_decode_mod): every branch of the launchers at the smallest shape that takes it.

One shape: B = 2, H = 4, H_kv = 2, S_q = 1, D = 64, fill levels (0, 70), S_new = 2, a cache of 128 rows or four pages of 32
(the new rows of the second sequence go to its third page, those of the first to its first).  Crossed: the format (16-bit,
e4m3, MXFP4), padded and paged, forced splits 1 and 3 (3: the combine kernel, and for the two-key sequence splits without
work), sinks none and given, fp16 and bf16.  Every cell:
  * the caches after the call are the caches before with the host quantiser's bytes in rows [L_b, L_b + 2), bit for bit
    (16-bit: the rows themselves; e4m3: (x / d).clamp(-448, 448).to(float8_e4m3fn); MXFP4: quantize_kv_mxfp4);
  * O / LSE against tests/attn_ref.py in fp64 on those caches dequantised, under the bound the format's own accuracy test
    uses: test_gpu_kvcache.tol, test_gpu_kvcache_fp8.tol, test_gpu_kvcache_fp4.BOUND per (sequence, head); with sinks
    test_gpu_sink.REL (MXFP4: BOUND again); LSE by test_gpu_kvcache.check_lse;
  * the paged call has the padded call's bits, and its pools afterwards are the padded caches' pages;
  * the sequence of length 0 sees exactly its two new keys: its rows equal, bit for bit, a call without an append on a
    cache that holds nothing but those two rows -- everything else in every cache is poison (0xFF bytes: NaN in the three
    formats' value or scale bytes), so a stray read shows.
One more cell at D = 256, 16-bit and e4m3, where an MXFP4 cache is still refused."""
import pytest
import torch

import test_gpu_kvcache as tk
import test_gpu_kvcache_fp4 as t4
import test_gpu_kvcache_fp8 as t8
import test_gpu_sink as tsk
import variantcheck as vck

pytestmark = pytest.mark.gpu

F16, BF16, F8 = torch.float16, torch.bfloat16, torch.float8_e4m3fn
B, H, HKV, SQ, SNEW, SC, PAGE = 2, 4, 2, 1, 2, 128, 32
LENS = [0, 70]
AFTER = [L + SNEW for L in LENS]
MP = SC // PAGE


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def u8(t):
    return t.view(torch.uint8)


class Fmt16:
    name = "16bit"

    def make(self, D, dtype, seed):
        q, kc, vc = tk.make(B, H, HKV, SQ, SC, D, dtype, seed)
        return q, [kc, vc]

    def quantised(self, kn, vn):
        return [kn, vn]

    def dequantised(self, c):
        return c[0].double(), c[1].double()

    def run(self, q, c, sl, table, sinks, **kw):
        M = tk._M()
        if table is not None:
            import paged_kvcache as P
            return P.flash_attention_kvcache_paged(q, *c, sl, table, sinks=sinks, return_lse=True, **kw)
        if sinks is not None:
            return M.flash_attention_kvcache_sink(q, *c, sl, sinks, return_lse=True, **kw)
        return M.flash_attention_kvcache(q, *c, sl, return_lse=True, **kw)

    def bound(self, q, K, V, O_ref, sinks):
        return tsk.REL[q.dtype] if sinks is not None else tk.tol(q.dtype, q, K.to(q.dtype), V.to(q.dtype), AFTER, -1, -1, O_ref)


class Fmt8(Fmt16):
    name = "e4m3"

    def make(self, D, dtype, seed):
        q, k8, v8, self.kd, self.vd = t8.make8(B, H, HKV, SQ, SC, D, dtype, [SC, SC], seed)
        return q, [k8, v8]

    def quantised(self, kn, vn):
        cast = lambda x, d: (x.float() / d[:, :, None, None]).clamp(-448, 448).to(F8)
        return [cast(kn.cpu(), self.kd.cpu()).cuda(), cast(vn.cpu(), self.vd.cpu()).cuda()]

    def dequantised(self, c):
        return t8.deq(c[0], self.kd), t8.deq(c[1], self.vd)

    def run(self, q, c, sl, table, sinks, **kw):
        M = tk._M()
        if table is not None:
            import paged_kvcache as P
            return P.flash_attention_kvcache_paged(q, *c, sl, table, sinks=sinks, k_descale=self.kd, v_descale=self.vd,
                                                   return_lse=True, **kw)
        if sinks is not None:
            return M.flash_attention_kvcache_fp8_sink(q, *c, sl, sinks, self.kd, self.vd, return_lse=True, **kw)
        return M.flash_attention_kvcache_fp8(q, *c, sl, self.kd, self.vd, return_lse=True, **kw)

    def bound(self, q, K, V, O_ref, sinks):
        return tsk.REL[q.dtype] if sinks is not None else t8.tol(q.dtype, q, K, V, AFTER, -1, -1, O_ref)


class Fmt4(Fmt16):
    name = "mxfp4"

    def make(self, D, dtype, seed):
        q, kc, vc, ks, vs = t4.make4(B, H, HKV, SQ, SC, D, dtype, seed)
        return q, [kc, vc, ks, vs]

    def quantised(self, kn, vn):
        F = t4._F()
        (kq, kqs), (vq, vqs) = F.quantize_kv_mxfp4(kn.cpu()), F.quantize_kv_mxfp4(vn.cpu())
        return [kq.cuda(), vq.cuda(), kqs.cuda(), vqs.cuda()]

    def dequantised(self, c):
        return t4.deq64(c[0], c[2]), t4.deq64(c[1], c[3])

    def run(self, q, c, sl, table, sinks, **kw):
        F = t4._F()
        if table is not None:
            return F.flash_attention_kvcache_fp4_paged(q, *c, sl, table, sinks=sinks, return_lse=True, **kw)
        return F.flash_attention_kvcache_fp4(q, *c, sl, sinks=sinks, return_lse=True, **kw)

    bound = None        # per (sequence, head): t4.check


def poison_past(caches, lens):
    out = [t.clone() for t in caches]
    for b, L in enumerate(lens):
        for t in out:
            u8(t)[b, :, L:] = t4.FF
    return out


def scatter(caches, seed):
    """the padded caches as pools of MP pages per sequence plus spares under one permuted table (t4.scatter4 on their bytes)"""
    pools, table = t4.scatter4([u8(t) for t in caches], AFTER, PAGE, sum(-(-L // PAGE) for L in AFTER) + 3, MP, seed)
    return [p.view(t.dtype) for p, t in zip(pools, caches)], table


def new_rows(D, dtype, scale, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda: (torch.randn(B, HKV, SNEW, D, generator=g, device="cuda") * scale).to(dtype)
    return r(), r()


def cell(fmt, D, dtype, nsplit, with_sinks, seed):
    q, caches = fmt.make(D, dtype, seed)
    # new rows at the magnitude of the format's cached values, so that old and new keys both carry weight
    kn, vn = new_rows(D, dtype, 20.0 if isinstance(fmt, Fmt4) else 1.0, seed + 1)
    sinks = torch.linspace(-1.0, 2.0, H, device="cuda", dtype=torch.float32) if with_sinks else None
    sl = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    before = poison_past(caches, LENS)
    want = [t.clone() for t in before]
    for t, new in zip(want, fmt.quantised(kn, vn)):
        for b, L in enumerate(LENS):
            u8(t)[b, :, L:L + SNEW] = u8(new)[b]
    vck.splits(nsplit)
    # padded
    pad = [t.clone() for t in before]
    o, lse = fmt.run(q, pad, sl, None, sinks, k_new=kn, v_new=vn)
    torch.cuda.synchronize()
    for i, (got, w) in enumerate(zip(pad, want)):
        assert torch.equal(u8(got), u8(w)), ("padded cache %d" % i, int((u8(got) != u8(w)).sum()))
    assert o.shape == q.shape and o.dtype == dtype and lse.shape == (B, H, SQ) and torch.isfinite(o).all()
    # fp64 on the dequantised caches (rows past the new fill level zeroed: they are poison and not part of the problem)
    clean = [t.clone() for t in want]
    for b, L in enumerate(AFTER):
        for t in clean:
            u8(t)[b, :, L:] = 0
    K, V = fmt.dequantised(clean)
    O_ref, LSE_ref = t4.truth(q, K, V, AFTER, -1, -1, sinks)
    tag = "%s D%d %s n=%d sinks=%s" % (fmt.name, D, dtype, nsplit, with_sinks)
    if fmt.bound is None:
        t4.check(tag, q, o, lse, O_ref, LSE_ref)
    else:
        err, bound = tk.rel(o, O_ref), fmt.bound(q, K, V, O_ref, sinks)
        print(tag, "relFro %.3e bound %.3e" % (err, bound))
        assert err < bound, (tag, err, bound)
        tk.check_lse(lse, LSE_ref)
    # paged: the padded call's bits, and its pools afterwards the padded caches' pages
    pools, table = scatter(before, seed + 2)
    po, plse = fmt.run(q, pools, sl, t4.wide(table), sinks, k_new=kn, v_new=vn)
    torch.cuda.synchronize()
    assert t4.same((o, lse), (po, plse)), tag
    for i, (got, w) in enumerate(zip(pools, scatter(want, seed + 2)[0])):
        assert torch.equal(u8(got), u8(w)), ("pool %d" % i, int((u8(got) != u8(w)).sum()))
    # the empty sequence sees exactly its two new keys
    only = [torch.full_like(u8(t), t4.FF).view(t.dtype) for t in want]
    for t, w in zip(only, want):
        u8(t)[0, :, :SNEW] = u8(w)[0, :, :SNEW]
    two = torch.tensor([SNEW, 0], dtype=torch.int32, device="cuda")
    o2, lse2 = fmt.run(q, only, two, None, sinks)
    assert t4.same((o[0], lse[0]), (o2[0], lse2[0])), tag


@pytest.mark.parametrize("with_sinks", [False, True], ids=["plain", "sinks"])
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("fmt", [Fmt16, Fmt8, Fmt4], ids=lambda f: f.name)
def test_every_branch_of_the_joined_launch_path(fmt, nsplit, with_sinks):
    for i, dtype in enumerate((F16, BF16)):
        cell(fmt(), 64, dtype, nsplit, with_sinks, seed=10 * nsplit + i)


@pytest.mark.parametrize("fmt", [Fmt16, Fmt8], ids=lambda f: f.name)
def test_head_dim_256_takes_the_same_path_and_mxfp4_is_refused_there(fmt):
    cell(fmt(), 256, BF16, 3, True, seed=5)
    cell(fmt(), 256, F16, 1, False, seed=6)
    F = t4._F()
    q = torch.zeros(B, H, SQ, 256, dtype=BF16, device="cuda")
    c8 = lambda w: torch.zeros(B, HKV, SC, w, dtype=torch.uint8, device="cuda")
    sl = torch.zeros(B, dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError, match="D = 64 or 128"):
        F.flash_attention_kvcache_fp4(q, c8(128), c8(128), c8(8), c8(8), sl)
    import _mi355fa as fa
    p = q.data_ptr()
    rc = fa.lib.fa_fwd_kvcache_fp4(p, p, p, p, p, None, None, sl.data_ptr(), None, None, None, p, None, None, 0, B, H, HKV, SQ, SC,
                                   0, 256, fa.BF16, fa.KV_MXFP4, 0.0625, -1, -1, None, None)
    assert rc == -2 and fa.lib.fa_last_error().decode() == "fa_fwd_kvcache_fp4: an MXFP4 cache takes head dim 64 or 128"
    torch.cuda.synchronize()
