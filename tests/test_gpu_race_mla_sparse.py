"""The poisoned and decoyed repeat-launch check (tests/racecheck.py, as tests/test_gpu_race_mla.py applies it) on the sparse MLA
decode step with append, through the raw C entry point: the <Topk, T> overload of fa_decode_paged_kernel between the <MLA, T>
append and the shared combine kernel.  Lists of 1, 2, 3, 5 and 9 live tiles (-1 beyond them: those tiles are passed over), at
one forced split and at three (its control: the same call at one split); the undisturbed result is held to the fp64 truth."""
import functools

import pytest
import torch

import mlacheck as mc
import mlasparsecheck as ms
import racecheck as rc
import variantcheck as vck
from mlacheck import BF16, F16

pytestmark = pytest.mark.gpu

RUNS = 40
NEW = 2
H, SQ = 40, NEW            # a full head block and a partial one, per query token
PAGE = 64
MP = 5                     # 320 keys of table reach
L = 300
TILES = (1, 2, 3, 5, 9)
TOPK = 32 * TILES[-1]


class Problem:
    """One step on one set of inputs, with o, lse, the pool and the workspace owned by the caller.  Every sequence holds L keys
    after the append; sequence b's lists name the appended rows first and hold 32 * TILES[b] entries."""

    def __init__(self, dtype, seed):
        import _mi355fa as fa
        self.fa, self.dtype, self.B, self.Ls = fa, dtype, len(TILES), [L] * len(TILES)
        B = self.B
        self.q, kv = mc.make(B, H, SQ, MP * PAGE, dtype, seed=100 + seed)
        self.new = torch.randn(B, NEW, mc.D, generator=torch.Generator(device="cuda").manual_seed(200 + seed), device="cuda").to(dtype)
        self.full = kv.clone()                                                  # the cache with the new rows in place
        self.full[:, L - NEW:L] = self.new
        init, self.table = mc.scatter(kv, [L - NEW] * B, PAGE, MP, 7, alloc=self.Ls)
        expect, _ = mc.scatter(self.full, self.Ls, PAGE, MP, 7)
        self.sl = torch.tensor([L - NEW] * B, dtype=torch.int32, device="cuda")
        self.idx = ms.draw(self.Ls, SQ, TOPK, seed=300 + seed, lead=(L - 1, L - 2)).cuda()
        for b, t in enumerate(TILES):
            self.idx[b, :, 32 * t:] = -1
        o, lse = torch.empty(B, H, SQ, mc.DV, dtype=dtype, device="cuda"), torch.empty(B, H, SQ, device="cuda")
        self.outs = [rc.Out("O", o), rc.Out("LSE", lse), rc.Out("latent pool", init, init=init, expect=expect)]
        self.scratch_outs = [torch.empty_like(x.like) if x.init is None else x.init.clone() for x in self.outs]   # the decoy's
        self.ws = torch.empty(max(self.need(n) for n in (1, 3)) + 16, dtype=torch.uint8, device="cuda")

    def need(self, n=None):
        vck.splits(n) if n is not None else None
        return self.fa.lib.fa_fwd_kvcache_mla_sparse_workspace_bytes(self.B, H, SQ, TOPK, MP, PAGE, NEW)

    def launch(self, xs):
        fa, (o, lse, pool), P, need = self.fa, xs, lambda t: t.data_ptr(), self.need()
        assert 0 <= need <= self.ws.numel()
        rcode = fa.lib.fa_fwd_kvcache_mla_sparse(P(self.q), P(pool), P(self.new), P(self.idx), P(self.sl), P(self.table), P(o), P(lse),
                                                 P(self.ws), need, self.B, H, SQ, TOPK, pool.shape[0], PAGE, MP, MP, NEW,
                                                 int(self.dtype == BF16), mc.DEFAULT_SCALE, 1, None, None, None, None,
                                                 torch.cuda.current_stream().cuda_stream)
        fa.check(rcode, "fa_fwd_kvcache_mla_sparse")


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


@pytest.mark.parametrize("n", [1, 3], ids=["split1", "split3"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_poisoned_and_decoyed_launches_repeat_bit_for_bit(dtype, n):
    p, d = Problem(dtype, 1), Problem(dtype, 2)
    case = dict(id="sparse-mla-%s/n%d" % (rc.DT[dtype], n),
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
                       control=functools.partial(control, mode) if n > 1 else None, runs=RUNS)
    ms.held(case["id"], ms.reference(p.q, p.full, p.idx, p.Ls, True), (res["plain"][0], res["plain"][1]))
