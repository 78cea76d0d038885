"""The poisoned and decoyed repeat-launch check (tests/racecheck.py, as tests/test_gpu_race_mla_indexer.py applies it) on the prefill
logits kernel: 40 rows (three row blocks, the last partial) x 570 keys, 18 tiles through an LDS ring of two.  Its own control."""
import pytest
import torch

import mlaindexercheck as ic
import racecheck as rc
from test_gpu_mla_indexer_prefill import device_args, problem, ranges, truth

pytestmark = pytest.mark.gpu


def test_poisoned_and_decoyed_launches_repeat_bit_for_bit():
    import mla_indexer as M
    ks, ke = ranges("context", 40, 570)
    p, d = problem(40, 570, 64), problem(40, 570, 32)                # (the decoy: other data through another instance)
    launch = lambda args: lambda xs: M.mla_indexer_logits_fp8_prefill(*args, out=xs[0])
    pa, da = device_args(*p, ks, ke), device_args(*d, ks, ke)
    outs = [rc.Out("logits", torch.empty(40, 570, device="cuda"))]
    case = dict(id="mla-indexer-prefill", stems=["fa_decode_paged_kernel"])
    for mode in rc.MODES:
        res = rc.check(case, launch(pa), outs, mode, decoy=lambda: launch(da)([torch.empty_like(outs[0].like)]), runs=40)
    ic.held(case["id"], res["plain"][0], *truth(*p, ks, ke, 570))
