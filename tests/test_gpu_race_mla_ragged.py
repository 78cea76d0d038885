"""The poisoned repeat-launch check (tests/racecheck.py) on the packed MLA decode step with append (the plan kernel and the
<Latent, T> overloads of fa_kvcache_append_ragged_kernel, fa_decode_ragged_kernel and fa_decode_combine_ragged_kernel), modelled on
tests/test_gpu_race_mla.py: every launch behind NaN poison in LDS and registers, or behind a decoy launch on other inputs, must
give the bits of the first one and of an undisturbed launch, the pool must hold the reference contents after the append, the rows
no sequence owns must keep their fill, and the undisturbed result is held to the fp64 truth of tests/mlaraggedcheck.py.
Sequences of 1, 2, 2, 0 and 3 queries at 1, 2, 3, 5 and 9 tiles after the append, H = 24 (a row block spans two queries, every
sequence's last block is partial), total_q allocated 4 rows past cu[B] so that end-marker workgroups and padding rows are in every
launch; at the formula's split count and with a forced split of 3, the control of both being the same call at one forced split.
The workspace -- the plan included -- is refilled before every launch: a workgroup that read the plan of an earlier launch
would find end markers only."""
import functools

import pytest
import torch

import mlacheck as mc
import mlaraggedcheck as mr
import racecheck as rc
import variantcheck as vck
from mlacheck import BF16, F16

pytestmark = pytest.mark.gpu

RUNS = 40
H = 24
PAGE = 64
MP = 5                     # 320 keys of table reach
QS = [1, 2, 2, 0, 3]
TILES = [1, 2, 3, 5, 9]
PAD = 4


class Problem:
    """One step on one set of inputs: the raw C entry point with o, lse, the pool and the workspace owned by the caller.
    Every sequence's append ends on the edge of a tile."""

    def __init__(self, dtype, seed):
        import _mi355fa as fa
        self.fa, self.dtype = fa, dtype
        seqs = [(s, 32 * t - s) for s, t in zip(QS, TILES)]
        self.step = st = mr.Step(seqs, H, dtype, True, seed=100 + seed, pad=PAD, S_pad=MP * PAGE)
        assert st.Ls == [32 * t for t in TILES] and st.total_q == sum(QS) + PAD
        init, self.table, expect = st.pools(PAGE, MP, 7)
        rows = torch.arange(st.total_q) < st.rows
        o = torch.empty(st.total_q, H, mc.DV, dtype=dtype, device="cuda")
        lse = torch.empty(H, st.total_q, device="cuda")
        self.outs = [rc.Out("O", o, owned=rows), rc.Out("LSE", lse, owned=rows[None].expand(H, -1).contiguous()),
                     rc.Out("latent pool", init, init=init, expect=expect)]
        self.scratch_outs = [torch.empty_like(x.like) if x.init is None else x.init.clone() for x in self.outs]   # the decoy's
        self.ws = torch.empty(max(self.need(n) for n in (1, 3, 0)) + 16, dtype=torch.uint8, device="cuda")

    def need(self, n=None):
        if n is not None:
            vck.splits(n)
        return self.fa.lib.fa_fwd_kvcache_mla_ragged_workspace_bytes(self.step.total_q, self.step.B, H, MP, PAGE)

    def launch(self, xs):
        fa, st = self.fa, self.step
        o, lse, pool = xs
        P = lambda t: t.data_ptr()
        need = self.need()
        assert 0 < need <= self.ws.numel()
        rcode = fa.lib.fa_fwd_kvcache_mla_ragged(P(st.qp), P(pool), P(st.new), P(st.cu), P(st.sl), P(self.table), P(o), P(lse), P(self.ws),
                                                 need, st.total_q, st.B, H, pool.shape[0], PAGE, MP, MP, 1, int(self.dtype == BF16),
                                                 mc.DEFAULT_SCALE, 1, None, None, None, torch.cuda.current_stream().cuda_stream)
        fa.check(rcode, "fa_fwd_kvcache_mla_ragged")


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


@pytest.mark.parametrize("n", [0, 3], ids=["formula", "split3"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_poisoned_and_decoyed_launches_repeat_bit_for_bit(dtype, n):
    p, d = Problem(dtype, 1), Problem(dtype, 2)
    case = dict(id="packed-mla-%s/n%d" % (rc.DT[dtype], n),
                stems=["fa_decode_ragged_plan_kernel", "fa_decode_ragged_kernel", "fa_kvcache_append_ragged_kernel",
                       "fa_decode_combine_ragged_kernel"])
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
    mr.held(case["id"], p.step, o, lse, p.step.truth(True, level=True))
