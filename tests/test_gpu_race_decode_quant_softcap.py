"""The poisoned repeat-launch check (tests/racecheck.py) on the soft-capped decode step with append over the quantised caches --
one case per (format, geometry) and the packed kernel at D = 256 per format (the <T, D, F, SOFTCAP> overloads of
fa_decode_mod_kernel / _paged_kernel / _ragged_kernel, the formats' appends, the plan kernel and the shared combine kernels): every
launch behind NaN poison in LDS and registers, or behind a decoy launch on other inputs, must give the bits of the first one and
of an undisturbed launch, the caches and the scale tensors must hold what the format's plain call appends, and the undisturbed
result is held to the fp64 truth of tests/quantcapcheck.py.  Fill levels of 1, 4, 5 and 9 tiles (D = 256, two tiles per step: 1, 2,
3 and 5), at the formula's split count and with a forced split of 3; the control of both is the same call at one forced split."""
import ctypes
import functools

import pytest
import torch

import quantcapcheck as qc
import racecheck as rc
import variantcheck as vck
from quantcapcheck import BF16, F16

pytestmark = pytest.mark.gpu

RUNS = 40
NEW = 2
H, HKV, SQ = 8, 2, NEW
PAGE = 64
SC = 320
CAP = 30.0
FMT_ID = {"e4m3": 0, "token": 1, "fp4": 2}
CASES = [(f, g, D, dt) for f in qc.FORMATS
         for g, D, dt in (("padded", 128, BF16), ("paged", 64, F16), ("packed", 128, F16), ("packed", 256, BF16))]


class Problem:
    """One step on one set of inputs: the raw C entry point with o, lse, the caches, the scales and the workspace owned by the
    caller.  Sequence i fills its tiles to their last row but NEW before the append, so the append ends on the tile's edge; the
    packed step brings NEW rows per sequence."""

    def __init__(self, fmt, layout, D, dtype, seed):
        import _mi355fa as fa
        self.fa, self.fmt, self.layout, self.D, self.dtype = fa, fmt, layout, D, dtype
        tiles = (1, 2, 3, 5) if D == 256 else (1, 4, 5, 9)
        self.Ls = [32 * t for t in tiles]
        fills = [L - NEW for L in self.Ls]
        self.B = B = len(fills)
        self.q, c = qc.make(fmt, B, H, HKV, SQ, SC, D, dtype, CAP, seed=100 + seed)
        self.kn, self.vn = qc.new_rows(B, HKV, NEW, D, dtype, 200 + seed)
        self.sl = qc.sl_of(fills)
        self.MP = SC // PAGE
        self.kd, self.vd = c.kd, c.vd
        if layout == "packed":                                                  # NEW rows per sequence, sequence after sequence
            self.T = B * SQ
            self.cu = torch.arange(0, self.T + 1, SQ, dtype=torch.int32, device="cuda")
            self.qp = self.q.transpose(1, 2).reshape(self.T, H, D).contiguous()
            self.knp = self.kn.transpose(1, 2).reshape(self.T, HKV, D).contiguous()
            self.vnp = self.vn.transpose(1, 2).reshape(self.T, HKV, D).contiguous()
            o, lse = torch.empty_like(self.qp), torch.empty(H, self.T, device="cuda")
        else:
            o, lse = torch.empty_like(self.q), torch.empty(B, H, SQ, device="cuda")
        vck.splits(1)                                                           # the reference append: the format's plain call
        if layout == "padded":
            init = c.clone()
            for b, f in enumerate(fills):                                       # poison at and past the fill level
                for t in init.tensors():
                    t[b, :, f:].view(torch.uint8).fill_(0xFF) if t.element_size() == 1 else t[b, :, f:].fill_(float("nan"))
            self.table = None
            expect = init.clone()
            qc.plain_padded(self.q, expect, self.sl, k_new=self.kn, v_new=self.vn)
            self.ref = expect
        else:
            init, self.table = qc.scatter(c, fills, PAGE, self.MP, seed=7, alloc=self.Ls)
            expect = init.clone()
            if layout == "paged":
                qc.plain_paged(self.q, expect, self.sl, self.table, k_new=self.kn, v_new=self.vn)
            else:
                qc.plain_packed(self.qp, expect, self.cu, self.sl, self.table, k_new=self.knp, v_new=self.vnp)
            self.ref = qc.gather(expect, self.table)
        torch.cuda.synchronize()
        vck.splits(0)
        names = ("K cache", "V cache", "K scale", "V scale")
        self.outs = [rc.Out("O", o), rc.Out("LSE", lse)] + [rc.Out(n, i, init=i, expect=e)
                                                            for n, i, e in zip(names, init.tensors(), expect.tensors())]
        self.scratch_outs = [torch.empty_like(x.like) if x.init is None else x.init.clone() for x in self.outs]   # the decoy's
        self.ws = torch.empty(max(self.need(n) for n in (1, 3, 0)) + 16, dtype=torch.uint8, device="cuda")

    def need(self, n=None):
        L, f = self.fa.lib, FMT_ID[self.fmt]
        if n is not None:
            vck.splits(n)
        if self.layout == "padded":
            return L.fa_fwd_kvcache_quant_softcap_workspace_bytes(f, self.B, H, HKV, SQ, SC, NEW, self.D)
        if self.layout == "paged":
            return L.fa_fwd_kvcache_quant_softcap_paged_workspace_bytes(f, self.B, H, HKV, SQ, self.MP, PAGE, NEW, self.D)
        return L.fa_fwd_kvcache_quant_softcap_ragged_workspace_bytes(f, self.T, self.B, H, HKV, self.MP, PAGE, self.D)

    def launch(self, xs):
        fa = self.fa
        o, lse, kc, vc = xs[:4]
        P = lambda t: None if t is None else t.data_ptr()
        cache = fa.QuantCache(format=FMT_ID[self.fmt])
        if self.fmt == "e4m3":
            cache.k_descale, cache.v_descale, cache.descale_bstride = P(self.kd), P(self.vd), HKV
        else:
            cache.k_scale, cache.v_scale = P(xs[4]), P(xs[5])
        cp = ctypes.byref(cache)
        st = torch.cuda.current_stream().cuda_stream
        need = self.need()
        assert 0 <= need <= self.ws.numel()
        dt, scale = int(self.dtype == BF16), self.D ** -0.5
        if self.layout == "padded":
            rcode = fa.lib.fa_fwd_kvcache_quant_softcap(P(self.q), P(kc), P(vc), P(self.kn), P(self.vn), P(self.sl), P(o), P(lse),
                                                        P(self.ws), need, self.B, H, HKV, SQ, SC, NEW, self.D, dt, scale, CAP, -1, 0,
                                                        cp, None, st)
        elif self.layout == "paged":
            rcode = fa.lib.fa_fwd_kvcache_quant_softcap_paged(P(self.q), P(kc), P(vc), P(self.kn), P(self.vn), P(self.sl),
                                                              P(self.table), P(o), P(lse), P(self.ws), need, self.B, H, HKV, SQ,
                                                              kc.shape[0], PAGE, self.MP, self.MP, NEW, self.D, dt, scale, CAP, -1, 0,
                                                              cp, None, st)
        else:
            rcode = fa.lib.fa_fwd_kvcache_quant_softcap_ragged(P(self.qp), P(kc), P(vc), P(self.knp), P(self.vnp), P(self.cu),
                                                               P(self.sl), P(self.table), P(o), P(lse), P(self.ws), need, self.T,
                                                               self.B, H, HKV, kc.shape[0], PAGE, self.MP, self.MP, self.D, dt, scale,
                                                               CAP, -1, 0, cp, None, st)
        fa.check(rcode, "fa_fwd_kvcache_quant_softcap (%s)" % self.layout)


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


@pytest.mark.parametrize("n", [0, 3], ids=["formula", "split3"])
@pytest.mark.parametrize("fmt,layout,D,dtype", CASES, ids=["%s-%s-d%d-%s" % (f, g, D, rc.DT[dt]) for f, g, D, dt in CASES])
def test_poisoned_and_decoyed_launches_repeat_bit_for_bit(fmt, layout, D, dtype, n):
    p, d = Problem(fmt, layout, D, dtype, 1), Problem(fmt, layout, D, dtype, 2)
    stems = {"padded": ["fa_decode_mod_kernel", "fa_kvcache_append_kernel", "fa_decode_combine_kernel"],
             "paged": ["fa_decode_paged_kernel", "fa_kvcache_append_paged_kernel", "fa_decode_combine_kernel"],
             "packed": ["fa_decode_ragged_kernel", "fa_kvcache_append_ragged_kernel", "fa_decode_ragged_plan_kernel",
                        "fa_decode_combine_ragged_kernel"]}[layout]
    if fmt == "e4m3":                                                           # the per-tensor format's quantising appends
        stems[1] = stems[1].replace("_kernel", "_fp8_kernel")
    case = dict(id="%s-%s-softcap-d%d-%s/n%d" % (layout, fmt, D, rc.DT[dtype], n), stems=stems)
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
    qc.check(case["id"], p.q, o, lse, qc.truth(p.q, p.ref, p.Ls, CAP, True), p.Ls, matters=False)
