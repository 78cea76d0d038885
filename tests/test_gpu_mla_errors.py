"""The packed, FP8, sparse and sparse-FP8 MLA decode calls' checks behind their first device check, on device tensors: every case
of tests/mla_surface.py's GPU table is refused before anything is allocated or launched, with the exception type and message
of tests/golden/mla_errors.json ("gpu"), recorded on an MI355X before the MLA host layers were folded."""

import pytest

import mla_surface as ms

pytestmark = pytest.mark.gpu


def test_checks_behind_the_device_check_raise_what_they_raised():
    want = ms.load()["gpu"]
    cases = dict(ms.gpu_cases())
    assert sorted(cases) == sorted(want) and len(want) >= 300
    assert all(v[0] == "AssertionError" for v in want.values())     # the wrappers' and the bindings' own refusals
    wrong = {}
    for cid, thunk in cases.items():
        got = ms.outcome(thunk)
        if got != want[cid]:
            wrong[cid] = (got, want[cid])
    assert not wrong, wrong
