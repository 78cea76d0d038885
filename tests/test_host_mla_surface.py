"""The MLA decode family's host surface, replayed on any machine against tests/golden/mla_errors.json (tests/mla_surface.py
says what it holds and how it was recorded): the refusals of the ten C entry points with return code and fa_last_error() text,
the four pybind signature lines, and every malformed call of the CPU table of the packed, FP8, sparse and sparse-FP8 bindings and
wrappers with exception type and exact message.  tests/test_gpu_mla_errors.py replays the device half.

The coverage tests read the sources, wherever a fold puts the text: every "%s: ..." literal of the MLA entry points and every
FA_ASSERT message of the five MLA bindings and their shared header is the recorded first failure of at least one case, but for
the few written out below with their reasons."""
import functools
import os
import re

import pytest

import mla_surface as ms
from test_host_quant_surface import CSRC, _LITERAL, _assert_messages

MLA_ERRORS = ms.load()
TABLES = sorted({cid.split("/")[0] for half in ("c", "cpu") for cid in MLA_ERRORS[half]})
C_SOURCES = ("fa_api_mla.hip", "fa_api_mla_ragged.hip", "fa_api_mla_fp8.hip", "fa_api_mla_sparse.hip", "fa_api_mla_sparse_fp8.hip")
BINDING_SOURCES = ("torch_binding_mla.cpp", "torch_binding_mla_ragged.cpp", "torch_binding_mla_fp8.cpp", "torch_binding_mla_sparse.cpp",
                   "torch_binding_mla_sparse_fp8.cpp", "torch_binding_mla.h")
C_EXEMPT = {"%s: the launch failed (HIP error %lld)": "a launch has to fail: no argument makes it"}
BINDING_EXEMPT = {
    "all tensors must be on q's device": "needs tensors on two GPUs: the suite runs on one",
    "all tensors must be on packed q's device": "likewise, the packed call's wording",
}


@functools.lru_cache(maxsize=None)
def _cases():
    return dict(ms.c_cases()[0] + ms.cpu_cases())


def test_the_fixture_names_its_commit_and_the_four_signatures():
    assert re.fullmatch(r"[0-9a-f]{40}", MLA_ERRORS["commit"])
    assert ms.signatures() == MLA_ERRORS["signatures"]
    assert sorted(MLA_ERRORS["signatures"]) == ["kvcache_mla_fp8_forward", "kvcache_mla_ragged_forward", "kvcache_mla_sparse_forward",
                                                "kvcache_mla_sparse_fp8_forward"]


def test_the_tables_and_the_fixture_list_the_same_cases():
    assert sorted(_cases()) == sorted(list(MLA_ERRORS["c"]) + list(MLA_ERRORS["cpu"]))
    assert sorted(dict(ms.gpu_cases("cpu"))) == sorted(MLA_ERRORS["gpu"])      # the device half: the ids only, here
    # ten C functions; four bindings, and four wrappers in front of and (OnDevice) behind their device checks
    assert len(TABLES) == 10 + 4 + 4 + 4
    for half in ("cpu", "gpu"):
        assert all(v[0] == "AssertionError" for v in MLA_ERRORS[half].values())       # refused, every one: nothing returned
    # the entry points refuse every case -- none reaches a launch --; a workspace function returns its bytes for a sound shape
    for cid, (rc, text) in MLA_ERRORS["c"].items():
        assert (int(rc) < 0 and text.startswith(cid.split("/")[0] + ": ")) or ("_workspace_bytes/" in cid and int(rc) >= 0 and not text), cid
    for half in ("c", "cpu", "gpu"):
        assert sum("+" in cid for cid in MLA_ERRORS[half]) >= 0.3 * len(MLA_ERRORS[half])     # the pairs that fix the order
    unbuilt = ms.unbuilt_pairs()
    assert all(why for _, why in unbuilt) and not {cid for cid, _ in unbuilt} & {c for h in ("c", "cpu", "gpu") for c in MLA_ERRORS[h]}


@pytest.mark.parametrize("table", TABLES)
def test_malformed_calls_are_refused_as_they_were(table):
    cases = _cases()
    wrong = {}
    for half in ("c", "cpu"):
        for cid, want in MLA_ERRORS[half].items():
            if cid.startswith(table + "/"):
                got = cases[cid]() if half == "c" else ms.outcome(cases[cid])
                if got != want:
                    wrong[cid] = (got, want)
    assert not wrong, wrong


# ---- coverage: what the sources can raise against what the fixture records --------------------------------------------------------
def _sources(names):
    for name in names:
        path = os.path.join(CSRC, name)
        if os.path.exists(path):            # a fold may have merged a file away, or not yet added the header
            with open(path) as fh:
                yield name, fh.read()


def _matches(fmt, recorded):
    """does a printf format ("%s: ... %lld ...") produce one of the recorded texts?"""
    rx = re.compile("".join(r"-?\d+" if p == "%lld" else r"\w+" if p == "%s" else re.escape(p) for p in re.split(r"(%lld|%s)", fmt)))
    return any(rx.fullmatch(text) for text in recorded)


def test_every_text_of_the_entry_points_is_a_recorded_first_failure():
    recorded = {v[1] for v in MLA_ERRORS["c"].values()}
    seen, missing = [], {}
    for name, text in _sources(C_SOURCES):
        for lit in _LITERAL.findall(re.sub(r'"\s+"', "", text)):
            if lit.startswith("%s: "):
                seen.append(lit)
                if lit not in C_EXEMPT and not _matches(lit, recorded):
                    missing.setdefault(lit, name)
    assert len(set(seen)) >= 66, len(set(seen))      # the distinct texts of the tree the fixture was recorded from
    assert not missing, missing
    assert len(C_EXEMPT) <= 4 and set(C_EXEMPT) <= set(seen)


def test_every_message_of_the_bindings_is_a_recorded_first_failure():
    import quant_surface as qs
    recorded = {v[1] for half in ("cpu", "gpu") for v in MLA_ERRORS[half].values()}
    recorded |= {v[1] for half in ("cpu", "gpu") for v in qs.load()[half].values()}       # the dense pair's
    seen, missing = set(), {}
    for name, text in _sources(BINDING_SOURCES):
        for lit in _assert_messages(text):
            seen.add(lit)
            if len(lit) > 1 and lit not in BINDING_EXEMPT and not any(lit in msg for msg in recorded):
                missing.setdefault(lit, name)
    assert len(seen) >= 52, len(seen)                # likewise
    assert not missing, missing
    assert len(BINDING_EXEMPT) <= 4 and set(BINDING_EXEMPT) <= seen, set(BINDING_EXEMPT) - seen
