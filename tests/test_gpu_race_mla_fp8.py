"""The poisoned repeat-launch check (tests/racecheck.py) on the FP8 MLA decode step with append, in the manner of
tests/test_gpu_race_mla.py: the <Fp8Row, T> overloads of fa_decode_paged_kernel, fa_kvcache_append_paged_kernel and
fa_decode_combine_kernel.  Every launch behind NaN poison in LDS and registers, or behind a decoy launch on other inputs, must
give the bits of the first one and of an undisturbed launch, the pool must hold the quantised reference rows after the append,
and the undisturbed result is held to the fp64 truth on the dequantised cache.  Fill levels of 1, 2, 3, 5 and 9 tiles, at one
forced split and at three; the control of both is the same call at one forced split.  Beside the exchange slots of the 16-bit
kernel, the wave-private scale slots in LDS are rewritten every step: the poison and the decoy are for both."""
import functools

import pytest
import torch

import mlacheck as mc
import mlafp8check as f8
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
        full = kv.clone()                                                       # the cache with the new rows in place
        for b, x in enumerate(fills):
            full[b, x:x + NEW] = self.new[b]
        quant = lambda x: f8.F().quantize_mla_latent_fp8(x.cpu()).cuda()        # on the CPU: the correctly rounded amax / 448
        self.rows_full = quant(full)
        init, self.table = f8.scatter(quant(kv), dtype, fills, PAGE, MP, 7, alloc=self.Ls)
        expect, _ = f8.scatter(self.rows_full, dtype, self.Ls, PAGE, MP, 7)
        self.sl = torch.tensor(fills, dtype=torch.int32, device="cuda")
        o, lse = torch.empty(B, H, SQ, mc.DV, dtype=dtype, device="cuda"), torch.empty(B, H, SQ, device="cuda")
        self.outs = [rc.Out("O", o), rc.Out("LSE", lse), rc.Out("FP8 latent pool", init, init=init, expect=expect)]
        self.scratch_outs = [torch.empty_like(x.like) if x.init is None else x.init.clone() for x in self.outs]   # the decoy's
        self.ws = torch.empty(max(self.need(n) for n in (1, 3)) + 16, dtype=torch.uint8, device="cuda")

    def need(self, n=None):
        if n is not None:
            vck.splits(n)
        return self.fa.lib.fa_fwd_kvcache_mla_fp8_workspace_bytes(self.B, H, SQ, MP, PAGE, NEW)

    def launch(self, xs):
        fa = self.fa
        o, lse, pool = xs
        P = lambda t: t.data_ptr()
        need = self.need()
        assert 0 <= need <= self.ws.numel()
        rcode = fa.lib.fa_fwd_kvcache_mla_fp8(P(self.q), P(pool), P(self.new), P(self.sl), P(self.table), P(o), P(lse), P(self.ws),
                                              need, self.B, H, SQ, pool.shape[0], PAGE, MP, MP, NEW, int(self.dtype == BF16),
                                              mc.DEFAULT_SCALE, 1, None, None, None, torch.cuda.current_stream().cuda_stream)
        fa.check(rcode, "fa_fwd_kvcache_mla_fp8")


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


@pytest.mark.parametrize("n", [1, 3], ids=["split1", "split3"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_poisoned_and_decoyed_launches_repeat_bit_for_bit(dtype, n):
    p, d = Problem(dtype, 1), Problem(dtype, 2)
    case = dict(id="paged-mla-fp8-%s/n%d" % (rc.DT[dtype], n),
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
                       control=None if n == 1 else functools.partial(control, mode), runs=RUNS)
    o, lse = res["plain"][0], res["plain"][1]
    _, O, LSE, level = f8.reference(p.q, p.rows_full, p.Ls, True)
    mc.held(case["id"], p.q, o, lse, O, LSE, p.Ls, level)
