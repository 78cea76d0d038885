"""The poisoned and decoyed repeat-launch check (tests/racecheck.py, as tests/test_gpu_race_mla_indexer.py applies it) on the two
selection kernels: the resident one at W 32768 and the streaming one at W 40000, S_q 2, topk 2048, three-valued rows, so that
the threshold falls inside a tie run and the histogram, the candidate buffer and both scans all decide the result.  The launch is
its own control; the undisturbed result is held to the reference."""
import pytest
import torch

import racecheck as rc
from test_gpu_mla_select import reference, rows

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W", [32768, 40000], ids=["resident", "streaming"])
def test_poisoned_and_decoyed_launches_repeat_bit_for_bit(W):
    import mla_indexer as M
    x, d = (rows("three", 1, 2, W, seed=s) for s in (31, 32))
    launch = lambda lg: lambda xs: M.mla_indexer_select(lg, 2048, out=xs[0])
    outs = [rc.Out("indices", torch.empty(1, 2, 2048, dtype=torch.int32, device="cuda"))]
    case = dict(id="mla-select-%d" % W, stems=["fa_decode_paged_kernel"])
    px, dx = x.cuda(), d.cuda()
    for mode in rc.MODES:
        res = rc.check(case, launch(px), outs, mode, decoy=lambda: launch(dx)([torch.empty_like(outs[0].like)]), runs=40)
    assert torch.equal(res["plain"][0].cpu(), reference(x, 2048))
