"""The poisoned repeat-launch check (tests/racecheck.py) on the MXFP4 decode step with append, padded and paged
(the MXFP4 overloads of fa_decode_mod_kernel / fa_decode_paged_kernel and of fa_kvcache_append_kernel / _paged_kernel, the
shared combine kernel): every launch behind NaN poison in LDS and registers, or behind a decoy launch on other inputs, must give the bits
of the first one and of an undisturbed launch, the caches and scales must hold the reference bytes after the append, and the
undisturbed result is held to the fp64 truth of tests/test_gpu_kvcache_fp4.py.  Fill levels of 1, 4, 5 and 9 tiles (a
workgroup takes four tiles per step), at the formula's split count and with a forced split of 3; the control of both is the
same call at one forced split."""
import functools

import pytest
import torch

import racecheck as rc
import variantcheck as vck
import test_gpu_kvcache_fp4 as t4

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
RUNS = 40
TILES = (1, 4, 5, 9)
NEW = 2
H, HKV, SQ = 8, 2, 3
PAGE = 64


class Problem:
    """One step on one set of inputs: the raw C entry point with o, lse, the caches, the scales and the workspace owned by
    the caller.  Sequence i fills TILES[i] tiles to their last row but one before the append, so the append ends on the
    tile's edge."""

    def __init__(self, layout, D, dtype, seed):
        import _mi355fa as fa
        import fp4_kvcache as F
        self.fa, self.layout, self.D, self.dtype = fa, layout, D, dtype
        self.Ls = [32 * t for t in TILES]
        fills = [L - NEW for L in self.Ls]
        self.B = B = len(fills)
        self.Sc = Sc = 320
        self.q, kc, vc, ks, vs = t4.make4(B, H, HKV, SQ, Sc, D, dtype, seed=100 + seed)
        g = torch.Generator(device="cuda").manual_seed(200 + seed)
        self.kn = torch.randn(B, HKV, NEW, D, generator=g, device="cuda").to(dtype)
        self.vn = torch.randn(B, HKV, NEW, D, generator=g, device="cuda").to(dtype)
        ref = [t.clone() for t in (kc, vc, ks, vs)]                             # the caches with the new rows in place
        new = F.quantize_kv_mxfp4(self.kn) + F.quantize_kv_mxfp4(self.vn)       # (k nibbles, k scales, v nibbles, v scales)
        for b, f in enumerate(fills):
            for t, n in zip(ref, (new[0], new[2], new[1], new[3])):
                t[b, :, f:f + NEW] = n[b]
        self.ref = ref

        def poisoned(ts, lens):
            ts = [t.clone() for t in ts]
            for b, L in enumerate(lens):
                for t in ts:
                    t[b, :, L:] = t4.FF
            return ts
        self.sl = torch.tensor(fills, dtype=torch.int32, device="cuda")
        if layout == "padded":
            init, expect = poisoned((kc, vc, ks, vs), fills), poisoned(ref, self.Ls)
            self.table = None
        else:
            self.MP = Sc // PAGE
            NP = sum(-(-L // PAGE) for L in self.Ls) + 3
            init, self.table = t4.scatter4(poisoned((kc, vc, ks, vs), fills), self.Ls, PAGE, NP, self.MP, seed=7)
            expect, _ = t4.scatter4(poisoned(ref, self.Ls), self.Ls, PAGE, NP, self.MP, seed=7)
        o, lse = torch.empty_like(self.q), torch.empty(B, H, SQ, device="cuda")
        names = ("K cache", "V cache", "K scale", "V scale")
        self.outs = [rc.Out("O", o), rc.Out("LSE", lse)] + [rc.Out(n, i, init=i, expect=e) for n, i, e in zip(names, init, expect)]
        self.scratch_outs = [torch.empty_like(x.like) if x.init is None else x.init.clone() for x in self.outs]   # the decoy's
        self.ws = torch.empty(max(self.need(n) for n in (1, 3)) + 16, dtype=torch.uint8, device="cuda")

    def need(self, n=None):
        L = self.fa.lib
        if n is not None:
            vck.splits(n)
        if self.layout == "padded":
            return L.fa_fwd_kvcache_fp4_workspace_bytes(self.B, H, HKV, SQ, self.Sc, NEW, self.D)
        return L.fa_fwd_kvcache_fp4_paged_workspace_bytes(self.B, H, HKV, SQ, self.MP, PAGE, NEW, self.D)

    def launch(self, xs):
        fa = self.fa
        o, lse, kc, vc, ks, vs = xs
        P = lambda t: None if t is None else t.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        need = self.need()
        assert 0 <= need <= self.ws.numel()
        dt, scale = int(self.dtype == BF16), self.D ** -0.5
        if self.layout == "padded":
            rcode = fa.lib.fa_fwd_kvcache_fp4(P(self.q), P(kc), P(vc), P(ks), P(vs), P(self.kn), P(self.vn), P(self.sl), None, None,
                                              None, P(o), P(lse), P(self.ws), need, self.B, H, HKV, SQ, self.Sc, NEW, self.D, dt,
                                              fa.KV_MXFP4, scale, -1, 0, None, st)
        else:
            rcode = fa.lib.fa_fwd_kvcache_fp4_paged(P(self.q), P(kc), P(vc), P(ks), P(vs), P(self.kn), P(self.vn), P(self.sl),
                                                    P(self.table), None, None, None, P(o), P(lse), P(self.ws), need, self.B, H, HKV,
                                                    SQ, kc.shape[0], PAGE, self.MP, self.MP, NEW, self.D, dt, fa.KV_MXFP4, scale,
                                                    -1, 0, None, st)
        fa.check(rcode, "fa_fwd_kvcache_fp4" + ("_paged" if self.layout == "paged" else ""))


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


@pytest.mark.parametrize("n", [0, 3], ids=["formula", "split3"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("layout", ["padded", "paged"])
def test_poisoned_and_decoyed_launches_repeat_bit_for_bit(layout, D, dtype, n):
    p, d = Problem(layout, D, dtype, 1), Problem(layout, D, dtype, 2)
    stems = {"padded": ["fa_decode_mod_kernel", "fa_kvcache_append_kernel"],
             "paged": ["fa_decode_paged_kernel", "fa_kvcache_append_paged_kernel"]}[layout]
    case = dict(id="%s-fp4-d%d-%s/n%d" % (layout, D, rc.DT[dtype], n), stems=stems + ["fa_decode_combine_kernel"])
    vck.splits(n)
    assert n == 0 or p.need() == n * p.B * H * SQ * (D + 2) * 4
    decoy = lambda: d.launch(d.scratch_outs)

    def control(mode):                                                          # the same call at one forced split
        vck.splits(1)
        try:
            return rc.series(p.launch, p.outs, mode, decoy, [p.ws], RUNS)[1]
        finally:
            vck.splits(n)
    for mode in rc.MODES:
        res = rc.check(case, p.launch, p.outs, mode, decoy=decoy, scratch=[p.ws],
                       control=functools.partial(control, mode), runs=RUNS)
    o, lse = res["plain"][0], res["plain"][1]
    K, V = t4.deq64(p.ref[0], p.ref[2]), t4.deq64(p.ref[1], p.ref[3])
    t4.check(case["id"], p.q, o, lse, *t4.truth(p.q, K, V, p.Ls, -1, 0))
