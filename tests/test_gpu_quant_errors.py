"""The quantised-cache and MLA decode calls' checks behind the first device check (dtypes, cu_seqlens_q, cache_seqlens, the
table, the overflow guards, sinks and descales, the in-place conditions on caches and scales, k_new, `out`), on device tensors:
every case of tests/quant_surface.py's GPU table is refused before anything is allocated or launched, with the exception type
and message of tests/golden/quant_errors.json ("gpu"), recorded on an MI355X before the quantised bindings were folded."""

import pytest

import quant_surface as qs

pytestmark = pytest.mark.gpu


def test_checks_behind_the_device_check_raise_what_they_raised():
    want = qs.load()["gpu"]
    cases = dict(qs.gpu_cases())
    assert sorted(cases) == sorted(want) and len(want) >= 1000
    assert all(v[0] == "AssertionError" for v in want.values())     # the wrappers' and the bindings' own refusals
    wrong = {}
    for cid, thunk in cases.items():
        got = qs.outcome(thunk)
        if got != want[cid]:
            wrong[cid] = (got, want[cid])
    assert not wrong, wrong
