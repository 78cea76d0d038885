"""The decode wrappers' checks behind is_cuda (dtype mismatch, head dim, cache_seqlens, the k_new shapes, the in-place
condition on the caches, the fp8 descales), on device tensors: B=1, H=2, H_kv=1, S_q=1, S_cache=16, D=64 and D=96.  Every
case of tests/host_surface.py's GPU table is refused before anything is allocated or launched, with the exception type and
message of tests/golden/host_errors.json ("gpu"): the table was written from the source text of the tree before the
host wrappers were folded (no device was at hand to record it); on a device `python tests/host_surface.py` records it."""
import json
import os

import pytest

import host_surface as hs

pytestmark = pytest.mark.gpu


def test_checks_behind_is_cuda_raise_what_they_raised():
    with open(os.path.join(hs.GOLDEN, "host_errors.json")) as fh:
        want = json.load(fh)["gpu"]
    cases = dict(hs.gpu_cases())
    assert sorted(cases) == sorted(want) and len(want) >= 12 * 20
    assert all(v[0] == "AssertionError" for v in want.values())     # the binding's own refusals, none from the C ABI
    wrong = {}
    for cid, thunk in cases.items():
        got = hs.outcome(thunk)
        if got != want[cid]:
            wrong[cid] = (got, want[cid])
    assert not wrong, wrong
