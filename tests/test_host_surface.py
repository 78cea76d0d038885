"""The host layer's surface replayed against its fixtures (CPU): every public signature of the Python module and of the
C++ binding (tests/golden/host_surface.json), and for each malformed call of tests/host_surface.py's CPU table the first
check that fails, with its exception type and exact message (tests/golden/host_errors.json).  The fixtures were recorded
from the tree before the host wrappers were folded; `python tests/host_surface.py` rewrites them."""
import functools
import json
import os

import pytest

import host_surface as hs


def _golden(name):
    with open(os.path.join(hs.GOLDEN, name)) as fh:
        return json.load(fh)


SURFACE = _golden("host_surface.json")
ERRORS = _golden("host_errors.json")["cpu"]
FUNCTIONS = sorted({cid.split("/")[0] for cid in ERRORS})


@functools.lru_cache(maxsize=None)
def _cases():
    return dict(hs.cpu_cases())


@pytest.mark.parametrize("section", ["python", "autograd", "binding", "constants"])
def test_signatures(section):
    got = hs.surface()[section]
    assert sorted(got) == sorted(SURFACE[section])     # no name lost, none added unrecorded
    for name, sig in SURFACE[section].items():
        assert got[name] == sig, name


def test_the_table_and_the_fixture_list_the_same_cases():
    assert sorted(_cases()) == sorted(ERRORS)
    assert len(FUNCTIONS) == 6 + 6 + 3 * 7     # decode wrappers, their pybind functions, 7 training callables per feature
    for fn in FUNCTIONS:                       # per function: >= 3 cases that violate two checks at once
        assert sum(1 for cid in ERRORS if cid.startswith(fn + "/") and "+" in cid) >= 3, fn
    assert all(v[0] != "returned" for v in ERRORS.values())


@pytest.mark.parametrize("function", FUNCTIONS)
def test_malformed_calls_raise_what_they_raised(function):
    cases = _cases()
    wrong = {}
    for cid, want in ERRORS.items():
        if cid.startswith(function + "/"):
            got = hs.outcome(cases[cid])
            if got != want:
                wrong[cid] = (got, want)
    assert not wrong, wrong
