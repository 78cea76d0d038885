"""The paged and packed decode calls' checks behind is_cuda (dtypes, head dim, cu_seqlens_q, cache_seqlens, the table, every
fp32 vector argument, the in-place condition on the pools, the k_new shapes, `out`), on device tensors: every case of
tests/paged_surface.py's GPU table is refused before anything is allocated or launched, with the exception type and
message of tests/golden/paged_errors.json ("gpu"), recorded on an MI355X before the two bindings became one module."""
import json
import os

import pytest

import paged_surface as ps

pytestmark = pytest.mark.gpu


def test_checks_behind_is_cuda_raise_what_they_raised():
    with open(os.path.join(ps.GOLDEN, "paged_errors.json")) as fh:
        want = json.load(fh)["gpu"]
    cases = dict(ps.gpu_cases())
    assert sorted(cases) == sorted(want) and len(want) >= 4 * 80
    assert all(v[0] == "AssertionError" for v in want.values())     # the wrappers' and the binding's own refusals
    wrong = {}
    for cid, thunk in cases.items():
        got = ps.outcome(thunk)
        if got != want[cid]:
            wrong[cid] = (got, want[cid])
    assert not wrong, wrong
