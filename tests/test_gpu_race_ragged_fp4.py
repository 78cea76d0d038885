"""The poisoned repeat-launch check (tests/racecheck.py) on the packed MXFP4 decode step with append
(include/mi355fa_ragged_fp4.h: the plan kernel, the MXFP4 overloads of fa_kvcache_append_ragged_kernel and
fa_decode_ragged_kernel, the shared packed combine kernel), in the shape of tests/test_gpu_race_decode_fp4.py: every launch
behind NaN poison in LDS and registers, or behind a decoy launch on other inputs, must give the bits of the first one and of an
undisturbed launch, the pools and scale pools must hold the reference bytes after the append, the padding rows of O and LSE
must keep their fill, and the undisturbed result is held to the fp64 truth of tests/test_gpu_kvcache_fp4.py.  Fill levels of
1, 4, 5 and 9 tiles (a workgroup takes four tiles per step, two at D = 256, where the odd shares leave a wave pair that only
joins the barrier) with 1, 3, 0 and 5 queries, at the formula's split count and with a forced split of 3; the control of both
is the same call at one forced split."""
import functools

import pytest
import torch

import racecheck as rc
import raggedcheck as rg
import variantcheck as vck
import test_gpu_kvcache_fp4 as t4

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
RUNS = 40
TILES = (1, 4, 5, 9)
S = (1, 3, 0, 5)
PADROWS = 2
H, HKV = 8, 2
PAGE = 64


class Problem:
    """One step on one set of inputs: the raw C entry point with o, lse, the pools, the scale pools and the workspace (the
    plan at its head) owned by the caller.  Sequence i ends at TILES[i] whole tiles after its S[i] appended rows."""

    def __init__(self, D, dtype, seed):
        import _mi355fa as fa
        import fp4_kvcache as F
        self.fa, self.D, self.dtype = fa, D, dtype
        self.Ls = [32 * t for t in TILES]
        fills = [L - s for L, s in zip(self.Ls, S)]
        self.B = B = len(fills)
        self.T = sum(S) + PADROWS
        Sc = 320
        qb, kc, vc, ks, vs = t4.make4(B, H, HKV, max(S), Sc, D, dtype, seed=100 + seed)
        self.q_seq = [qb[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)]
        self.q = rg.pack(self.q_seq, self.T, fill=0.0)
        g = torch.Generator(device="cuda").manual_seed(200 + seed)
        knb = torch.randn(B, HKV, max(S), D, generator=g, device="cuda").to(dtype)
        vnb = torch.randn(B, HKV, max(S), D, generator=g, device="cuda").to(dtype)
        pk = lambda t: rg.pack([t[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)], self.T, fill=0.0)
        self.kn, self.vn = pk(knb), pk(vnb)
        ref = [t.clone() for t in (kc, vc, ks, vs)]                             # the caches with the new rows in place
        new = F.quantize_kv_mxfp4(knb) + F.quantize_kv_mxfp4(vnb)               # (k nibbles, k scales, v nibbles, v scales)
        for b, (f, s) in enumerate(zip(fills, S)):
            for t, n in zip(ref, (new[0], new[2], new[1], new[3])):
                t[b, :, f:f + s] = n[b, :, :s]
        self.ref = ref

        def poisoned(ts, lens):
            ts = [t.clone() for t in ts]
            for b, L in enumerate(lens):
                for t in ts:
                    t[b, :, L:] = t4.FF
            return ts
        self.sl = torch.tensor(fills, dtype=torch.int32, device="cuda")
        self.cu = rg.cu_of(S, device="cuda")
        self.MP = Sc // PAGE
        NP = sum(-(-L // PAGE) for L in self.Ls) + 3
        init, self.table = t4.scatter4(poisoned((kc, vc, ks, vs), fills), self.Ls, PAGE, NP, self.MP, seed=7)
        expect, _ = t4.scatter4(poisoned(ref, self.Ls), self.Ls, PAGE, NP, self.MP, seed=7)
        o, lse = torch.empty_like(self.q), torch.empty(H, self.T, device="cuda")
        rows = torch.arange(self.T) < sum(S)                                    # the rows a sequence owns
        names = ("K pool", "V pool", "K scale", "V scale")
        self.outs = [rc.Out("O", o, owned=rows), rc.Out("LSE", lse, owned=rows[None].expand(H, self.T).contiguous())] + [
            rc.Out(n, i, init=i, expect=e) for n, i, e in zip(names, init, expect)]
        self.scratch_outs = [torch.empty_like(x.like) if x.init is None else x.init.clone() for x in self.outs]   # the decoy's
        self.ws = torch.empty(max(self.need(n) for n in (0, 1, 3)) + 16, dtype=torch.uint8, device="cuda")   # (0: the formula's)

    def need(self, n=None):
        if n is not None:
            vck.splits(n)
        return self.fa.lib.fa_fwd_kvcache_fp4_ragged_workspace_bytes(self.T, self.B, H, HKV, self.MP, PAGE, self.D)

    def launch(self, xs):
        fa = self.fa
        o, lse, kc, vc, ks, vs = xs
        P = lambda t: None if t is None else t.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        need = self.need()
        assert 0 < need <= self.ws.numel()
        rcode = fa.lib.fa_fwd_kvcache_fp4_ragged(P(self.q), P(kc), P(vc), P(ks), P(vs), P(self.kn), P(self.vn), P(self.cu),
                                                 P(self.sl), P(self.table), None, None, None, P(o), P(lse), P(self.ws), need,
                                                 self.T, self.B, H, HKV, kc.shape[0], PAGE, self.MP, self.MP, self.D,
                                                 int(self.dtype == BF16), fa.KV_MXFP4, self.D ** -0.5, -1, 0, None, st)
        fa.check(rcode, "fa_fwd_kvcache_fp4_ragged")


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


@pytest.mark.parametrize("n", [0, 3], ids=["formula", "split3"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_poisoned_and_decoyed_launches_repeat_bit_for_bit(D, dtype, n):
    p, d = Problem(D, dtype, 1), Problem(D, dtype, 2)
    case = dict(id="ragged-fp4-d%d-%s/n%d" % (D, rc.DT[dtype], n),
                stems=["fa_decode_ragged_plan_kernel", "fa_kvcache_append_ragged_kernel", "fa_decode_ragged_kernel",
                       "fa_decode_combine_ragged_kernel"])
    vck.splits(n)
    assert n == 0 or p.need() == rg.workspace_bytes(n, p.T, p.B, H, HKV, D)
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
    for b, (ob, lb) in enumerate(zip(rg.unpack(o, S), rg.unpack_lse(lse, S))):
        if S[b]:
            t4.check("%s b=%d" % (case["id"], b), p.q_seq[b], ob, lb, *t4.truth(p.q_seq[b], K[b:b + 1], V[b:b + 1], [p.Ls[b]], -1, 0))
