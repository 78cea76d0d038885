"""The poisoned and decoyed repeat-launch check (tests/racecheck.py, as tests/test_gpu_race_mla.py applies it) on the indexer
logits kernel: 18 tiles of 32 keys, so a wave walks more tiles than its register ring of two is deep, and S_q 3 (a group with
a repeated last row).  The launch is its own control; the undisturbed result is held to the fp64 truth."""
import pytest
import torch

import mlaindexercheck as ic
import racecheck as rc

pytestmark = pytest.mark.gpu


def test_poisoned_and_decoyed_launches_repeat_bit_for_bit():
    import mla_indexer as M
    p, d = (ic.Problem([570, 300], 64, 3, 64, 9, seed=s) for s in (21, 22))
    launch = lambda prob: lambda xs: M.mla_indexer_logits_fp8(*prob.args(), is_causal=True, out=xs[0])
    outs = [rc.Out("logits", torch.empty(2, 3, 9 * 64, device="cuda"))]
    case = dict(id="mla-indexer", stems=["fa_decode_paged_kernel"])
    for mode in rc.MODES:
        res = rc.check(case, launch(p), outs, mode, decoy=lambda: launch(d)([torch.empty_like(outs[0].like)]), runs=40)
    ic.held(case["id"], res["plain"][0], *ic.truth(p.q8, p.w, p.keys, p.scales, p.fills, True, 9 * 64))
