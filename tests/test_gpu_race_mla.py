"""The poisoned repeat-launch check (tests/racecheck.py) on the MLA decode step with append (the <MLA, T> overloads of
fa_decode_paged_kernel and fa_kvcache_append_paged_kernel and the shared combine kernel at D = 512): every launch behind NaN
poison in LDS and registers, or behind a decoy launch on other inputs, must give the bits of the first one and of an
undisturbed launch, the pool must hold the reference contents after the append, and the undisturbed result is held to the
fp64 truth of tests/mlacheck.py.  Fill levels of 1, 2, 3, 5 and 9 tiles, at the formula's split count and with a forced
split of 3; the control of both is the same call at one forced split.  The four waves of a workgroup hand each other their
quarters of the scores through LDS slots that are reused two steps later, behind one barrier per step: that exchange is what
the poison and the decoy are for here."""
import functools

import pytest
import torch

import mlacheck as mc
import racecheck as rc
import variantcheck as vck
from mlacheck import BF16, F16

pytestmark = pytest.mark.gpu

RUNS = 40
NEW = 2
H, SQ = 24, NEW            # 48 rows: a full row block and a partial one
PAGE = 64
MP = 5                     # 320 keys of table reach


class Problem:
    """One step on one set of inputs: the raw C entry point with o, lse, the pool and the workspace owned by the caller.
    Sequence i fills its tiles to their last row but NEW before the append, so the append ends on the tile's edge."""

    def __init__(self, dtype, seed):
        import _mi355fa as fa
        self.fa, self.dtype = fa, dtype
        self.Ls = [32 * t for t in (1, 2, 3, 5, 9)]
        fills = [L - NEW for L in self.Ls]
        self.B = B = len(fills)
        self.q, kv = mc.make(B, H, SQ, MP * PAGE, dtype, seed=100 + seed)
        self.new = torch.randn(B, NEW, mc.D, generator=torch.Generator(device="cuda").manual_seed(200 + seed), device="cuda").to(dtype)
        self.full = kv.clone()                                                  # the cache with the new rows in place
        for b, f in enumerate(fills):
            self.full[b, f:f + NEW] = self.new[b]
        init, self.table = mc.scatter(kv, fills, PAGE, MP, 7, alloc=self.Ls)
        expect, _ = mc.scatter(self.full, self.Ls, PAGE, MP, 7)
        self.sl = torch.tensor(fills, dtype=torch.int32, device="cuda")
        o, lse = torch.empty(B, H, SQ, mc.DV, dtype=dtype, device="cuda"), torch.empty(B, H, SQ, device="cuda")
        self.outs = [rc.Out("O", o), rc.Out("LSE", lse), rc.Out("latent pool", init, init=init, expect=expect)]
        self.scratch_outs = [torch.empty_like(x.like) if x.init is None else x.init.clone() for x in self.outs]   # the decoy's
        self.ws = torch.empty(max(self.need(n) for n in (1, 3, 0)) + 16, dtype=torch.uint8, device="cuda")

    def need(self, n=None):
        if n is not None:
            vck.splits(n)
        return self.fa.lib.fa_fwd_kvcache_mla_workspace_bytes(self.B, H, SQ, MP, PAGE, NEW)

    def launch(self, xs):
        fa = self.fa
        o, lse, pool = xs
        P = lambda t: t.data_ptr()
        need = self.need()
        assert 0 <= need <= self.ws.numel()
        rcode = fa.lib.fa_fwd_kvcache_mla(P(self.q), P(pool), P(self.new), P(self.sl), P(self.table), P(o), P(lse), P(self.ws), need,
                                          self.B, H, SQ, pool.shape[0], PAGE, MP, MP, NEW, int(self.dtype == BF16), mc.DEFAULT_SCALE,
                                          1, None, None, None, torch.cuda.current_stream().cuda_stream)
        fa.check(rcode, "fa_fwd_kvcache_mla")


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


@pytest.mark.parametrize("n", [0, 3], ids=["formula", "split3"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_poisoned_and_decoyed_launches_repeat_bit_for_bit(dtype, n):
    p, d = Problem(dtype, 1), Problem(dtype, 2)
    case = dict(id="paged-mla-%s/n%d" % (rc.DT[dtype], n),
                stems=["fa_decode_paged_kernel", "fa_kvcache_append_paged_kernel", "fa_decode_combine_kernel"])
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
    O, LSE = mc.truth(p.q, p.full, p.Ls, True)
    level = mc.sdpa_level(p.q, p.full, p.Ls, True, None, O) if dtype == BF16 else None
    mc.held(case["id"], p.q, o, lse, O, LSE, p.Ls, level)
