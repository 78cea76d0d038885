"""The poisoned repeat-launch check (tests/racecheck.py) on the per-token-scaled e4m3 decode step with append -- padded, paged and
packed (the <T, D, SINK, TOKEN> overloads of fa_decode_mod_kernel / _paged_kernel / _ragged_kernel, the <T, TOKEN> overloads of the
three appends, the plan kernel and the shared combine kernels): every launch behind NaN poison in LDS and registers, or behind a
decoy launch on other inputs, must give the bits of the first one and of an undisturbed launch, the caches and the scale tensors
must hold the reference contents after the append, and the undisturbed result is held to the fp64 truth of
tests/fp8tokencheck.py.  Fill levels of 1, 4, 5 and 9 tiles (D = 256, two tiles per step: 1, 2, 3 and 5), at the formula's split
count and with a forced split of 3; the control of both is the same call at one forced split.  The kernels keep a wave's row
scales in LDS between two of its own instructions, which is what the poison is for here."""
import functools

import pytest
import torch

import fp8tokencheck as tk
import racecheck as rc
import variantcheck as vck
from fp8tokencheck import BF16, F16

pytestmark = pytest.mark.gpu

RUNS = 40
NEW = 2
H, HKV, SQ = 8, 2, NEW
PAGE = 64
SC = 320
CASES = [("padded", 64), ("padded", 128), ("paged", 64), ("paged", 128), ("packed", 64), ("packed", 128), ("packed", 256)]


class Problem:
    """One step on one set of inputs: the raw C entry point with o, lse, the caches, the scales and the workspace owned by the
    caller.  Sequence i fills its tiles to their last row but NEW before the append, so the append ends on the tile's edge; the
    packed step brings NEW rows per sequence."""

    def __init__(self, layout, D, dtype, seed):
        import _mi355fa as fa
        self.fa, self.layout, self.D, self.dtype = fa, layout, D, dtype
        tiles = (1, 2, 3, 5) if D == 256 else (1, 4, 5, 9)
        self.Ls = [32 * t for t in tiles]
        fills = [L - NEW for L in self.Ls]
        self.B = B = len(fills)
        self.q, k8, v8, ks, vs = tk.make(B, H, HKV, SQ, SC, D, dtype, seed=100 + seed)
        g = torch.Generator(device="cuda").manual_seed(200 + seed)
        self.kn = tk.rows((B, HKV, NEW, D), -6.0, 6.0, g).to(dtype)
        self.vn = tk.rows((B, HKV, NEW, D), -6.0, 6.0, g).to(dtype)
        ref = [t.clone() for t in (k8, v8, ks, vs)]                             # the caches with the new rows in place
        (kq, kqs), (vq, vqs) = (tuple(t.cuda() for t in tk.T().quantize_kv_fp8_per_token(x.cpu())) for x in (self.kn, self.vn))
        for b, f in enumerate(fills):
            for t, n in zip(ref, (kq, vq, kqs, vqs)):
                t[b, :, f:f + NEW] = n[b]
        self.ref = ref

        def poisoned(ts, lens):
            ts = [t.clone() for t in ts]
            for b, L in enumerate(lens):
                for t in ts:
                    t[b, :, L:].view(torch.uint8).fill_(0xFF) if t.dtype == tk.F8 else t[b, :, L:].fill_(float("nan"))
            return ts
        self.sl = torch.tensor(fills, dtype=torch.int32, device="cuda")
        if layout == "padded":
            init, expect = poisoned((k8, v8, ks, vs), fills), poisoned(ref, self.Ls)
            self.table = None
        else:
            self.MP = SC // PAGE
            NP = sum(-(-L // PAGE) for L in self.Ls) + 3
            *init, self.table = tk.scatter(*poisoned((k8, v8, ks, vs), fills), self.Ls, PAGE, NP, self.MP, seed=7)
            *expect, _ = tk.scatter(*poisoned(ref, self.Ls), self.Ls, PAGE, NP, self.MP, seed=7)
        if layout == "packed":                                                  # NEW rows per sequence, sequence after sequence
            self.T = B * SQ
            self.cu = torch.arange(0, self.T + 1, SQ, dtype=torch.int32, device="cuda")
            self.qp = self.q.transpose(1, 2).reshape(self.T, H, D).contiguous()
            self.knp = self.kn.transpose(1, 2).reshape(self.T, HKV, D).contiguous()
            self.vnp = self.vn.transpose(1, 2).reshape(self.T, HKV, D).contiguous()
            o, lse = torch.empty_like(self.qp), torch.empty(H, self.T, device="cuda")
        else:
            o, lse = torch.empty_like(self.q), torch.empty(B, H, SQ, device="cuda")
        names = ("K cache", "V cache", "K scale", "V scale")
        self.outs = [rc.Out("O", o), rc.Out("LSE", lse)] + [rc.Out(n, i, init=i, expect=e) for n, i, e in zip(names, init, expect)]
        self.scratch_outs = [torch.empty_like(x.like) if x.init is None else x.init.clone() for x in self.outs]   # the decoy's
        self.ws = torch.empty(max(self.need(n) for n in (1, 3, 0)) + 16, dtype=torch.uint8, device="cuda")

    def need(self, n=None):
        L = self.fa.lib
        if n is not None:
            vck.splits(n)
        if self.layout == "padded":
            return L.fa_fwd_kvcache_fp8_token_workspace_bytes(self.B, H, HKV, SQ, SC, NEW, self.D)
        if self.layout == "paged":
            return L.fa_fwd_kvcache_fp8_token_paged_workspace_bytes(self.B, H, HKV, SQ, self.MP, PAGE, NEW, self.D)
        return L.fa_fwd_kvcache_fp8_token_ragged_workspace_bytes(self.T, self.B, H, HKV, self.MP, PAGE, self.D)

    def launch(self, xs):
        fa = self.fa
        o, lse, kc, vc, ks, vs = xs
        P = lambda t: None if t is None else t.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        need = self.need()
        assert 0 <= need <= self.ws.numel()
        dt, scale = int(self.dtype == BF16), self.D ** -0.5
        if self.layout == "padded":
            rcode = fa.lib.fa_fwd_kvcache_fp8_token(P(self.q), P(kc), P(vc), P(ks), P(vs), P(self.kn), P(self.vn), P(self.sl), None,
                                                    None, None, P(o), P(lse), P(self.ws), need, self.B, H, HKV, SQ, SC, NEW, self.D,
                                                    dt, scale, -1, 0, None, st)
        elif self.layout == "paged":
            rcode = fa.lib.fa_fwd_kvcache_fp8_token_paged(P(self.q), P(kc), P(vc), P(ks), P(vs), P(self.kn), P(self.vn), P(self.sl),
                                                          P(self.table), None, None, None, P(o), P(lse), P(self.ws), need, self.B, H,
                                                          HKV, SQ, kc.shape[0], PAGE, self.MP, self.MP, NEW, self.D, dt, scale, -1, 0,
                                                          None, st)
        else:
            rcode = fa.lib.fa_fwd_kvcache_fp8_token_ragged(P(self.qp), P(kc), P(vc), P(ks), P(vs), P(self.knp), P(self.vnp),
                                                           P(self.cu), P(self.sl), P(self.table), None, None, None, P(o), P(lse),
                                                           P(self.ws), need, self.T, self.B, H, HKV, kc.shape[0], PAGE, self.MP,
                                                           self.MP, self.D, dt, scale, -1, 0, None, st)
        fa.check(rcode, "fa_fwd_kvcache_fp8_token (%s)" % self.layout)


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


@pytest.mark.parametrize("n", [0, 3], ids=["formula", "split3"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("layout,D", CASES, ids=["%s-d%d" % c for c in CASES])
def test_poisoned_and_decoyed_launches_repeat_bit_for_bit(layout, D, dtype, n):
    p, d = Problem(layout, D, dtype, 1), Problem(layout, D, dtype, 2)
    stems = {"padded": ["fa_decode_mod_kernel", "fa_kvcache_append_kernel", "fa_decode_combine_kernel"],
             "paged": ["fa_decode_paged_kernel", "fa_kvcache_append_paged_kernel", "fa_decode_combine_kernel"],
             "packed": ["fa_decode_ragged_kernel", "fa_kvcache_append_ragged_kernel", "fa_decode_ragged_plan_kernel",
                        "fa_decode_combine_ragged_kernel"]}[layout]
    case = dict(id="%s-fp8token-d%d-%s/n%d" % (layout, D, rc.DT[dtype], n), stems=stems)
    vck.splits(n)
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
    if layout == "packed":
        o = o.view(p.B, SQ, H, D).transpose(1, 2).contiguous()
        lse = lse.view(H, p.B, SQ).transpose(0, 1).contiguous()
    tk.check(case["id"], p.q, o, lse, *p.ref, p.Ls, True)
