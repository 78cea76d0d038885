"""Race tests (run with -m gpu on an MI355X): every one-wave-per-SIMD kernel (schedule family 4) is launched many times
on FIXED inputs at the headline shape, each launch preceded by fa_debug_poison (NaN patterns in every CU's LDS and in every
vector / accumulator register) or, in decoy mode, by the same launch on other inputs, and every result must equal the first
one bit for bit -- and one launch made without either.

Why this exists: these kernels order their LDS-DMA pieces, row-constant loads and stores with COUNTED vmcnt waits.  A count
that is off by one request is invisible to the parity tests -- the load it fails to cover has almost always landed -- and
invisible to a test that repeats one launch without poison, because LDS and registers still hold the previous launch's
(identical) data.  Round 4's dK/dV family 4 published a row constant ahead of its load once in ~30 launches under load;
parity, fuzz and family-vs-family tests were green.  The check itself is tests/racecheck.py, shared with
tests/test_gpu_race_families.py (every family at edge shapes), test_gpu_race_variants.py and test_gpu_race_decode.py;
tools/race_stress.py is the same check with more runs and shapes.  On one MI355X this file takes about 4 s.
"""
import pytest
import torch

import racecases as rc

pytestmark = pytest.mark.gpu

B, H, S = 4, 32, 4096   # BASELINE configs[2] / [3]: 1024-2048 work items, 4-8 passes per persistent workgroup
RUNS = rc.RUNS
assert RUNS == 120
CASES = {c["id"]: c for c in rc.HEADLINE_CASES}


@pytest.mark.parametrize("causal", [1, 0], ids=["causal", "full"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kern,D", [("fwd", 64), ("dq", 64), ("dkv", 64), ("fwd", 128)], ids=["fwd", "dq", "dkv", "fwd-d128"])
def test_family4_results_do_not_change_from_launch_to_launch(kern, D, dtype, causal):
    name = kern if D == 64 else "fwd-d128"
    c = CASES["%s-%s-%s" % (name, rc.DT[dtype], "causal" if causal else "full")]
    assert (c["kern"], c["D"], c["dtype"], c["causal"], c["B"], c["H"], c["Sq"], c["Sk"]) == (kern, D, dtype, bool(causal), B, H, S, S)
    # (the fp64 truth of this shape is tests/test_gpu_persistent.py's; a launch family 4 does not take skips, as before)
    rc.run_family_case(c, runs=RUNS, truth=False, admitted=False)
