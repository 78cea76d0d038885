"""The quantised-cache (MXFP4, per-token FP8, soft-capped) and MLA decode calls' surface, replayed on any machine: the seven
pybind signature lines, and every malformed call of tests/quant_surface.py's CPU table refused at the check, with the exception
type and the exact message, that tests/golden/quant_errors.json records -- taken from the tree before the quantised bindings
were folded onto the shared call path.  tests/test_gpu_quant_errors.py replays the device half.

The coverage test reads the bindings' sources: every message an FA_ASSERT there can raise is the recorded first failure of at
least one case (of either half), but for the few written out below with their reasons."""
import functools
import os
import re

import pytest

from conftest import ROOT
import quant_surface as qs

QUANT_ERRORS = qs.load()
TABLES = sorted({cid.split("/")[0] for cid in QUANT_ERRORS["cpu"]})
CSRC = os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd", "csrc")
# the four quantised / MLA bindings and the headers that hold the checks they share
SOURCES = ("torch_binding_fp4.cpp", "torch_binding_fp8_token.cpp", "torch_binding_quant_softcap.cpp", "torch_binding_mla.cpp",
           "torch_binding_common.h", "torch_binding_decode.h")
# messages no case of the tables can be refused with, by their text
EXEMPT = {
    "all tensors must be on q's device": "needs tensors on two GPUs: the suite runs on one",
    "packed queries go over paged pools: block_table is required":
        "the packed binding functions take block_table as a tensor, never None: only a new caller of the *_impl could trip it",
}


@functools.lru_cache(maxsize=None)
def _cpu_cases():
    return dict(qs.cpu_cases())


def test_binding_signatures_are_the_recorded_ones():
    assert qs.signatures() == QUANT_ERRORS["signatures"]
    assert sorted(QUANT_ERRORS["signatures"]) == [
        "kvcache_fp4_forward", "kvcache_fp4_ragged_forward", "kvcache_fp8_token_forward", "kvcache_fp8_token_ragged_forward",
        "kvcache_mla_forward", "kvcache_quant_softcap_forward", "kvcache_quant_softcap_ragged_forward"]


def test_the_error_tables_and_the_fixture_list_the_same_cases():
    want = QUANT_ERRORS["cpu"]
    assert sorted(_cpu_cases()) == sorted(want)
    assert sorted(dict(qs.gpu_cases("cpu"))) == sorted(QUANT_ERRORS["gpu"])      # the device half: the ids only, here
    # ten Python functions and seven binding functions, the soft-capped ones once per format, the padded-or-paged ones per geometry
    assert len(TABLES) == 3 + 3 + 9 + 1 + 3 + 3 + 9 + 1
    for half in ("cpu", "gpu"):
        assert all(v[0] == "AssertionError" for v in QUANT_ERRORS[half].values())     # refused, every one: nothing returned
        assert sum("+" in cid for cid in QUANT_ERRORS[half]) >= 10 * len(TABLES)      # the pairs that fix the order
    # a pair that is not in the tables is named with its reason
    unbuilt = qs.unbuilt_pairs()
    assert all(why for _, why in unbuilt) and not {cid for cid, _ in unbuilt} & (set(want) | set(QUANT_ERRORS["gpu"]))


@pytest.mark.parametrize("table", TABLES)
def test_malformed_calls_raise_what_they_raised(table):
    cases = _cpu_cases()
    wrong = {}
    for cid, want in QUANT_ERRORS["cpu"].items():
        if cid.startswith(table + "/"):
            got = qs.outcome(cases[cid])
            if got != want:
                wrong[cid] = (got, want)
    assert not wrong, wrong


# ---- coverage: what the sources can raise against what the fixture records --------------------------------------------------------
_LITERAL = re.compile(r'"((?:[^"\\]|\\.)*)"')


def _assert_messages(text):
    """the string literals of the message argument of every FA_ASSERT(cond, msg) in `text`, adjacent literals joined"""
    out = []
    for m in re.finditer(r"\bFA_ASSERT\(", text):
        depth, i, comma = 1, m.end(), None
        in_str = False
        while depth:
            c = text[i]
            if in_str:
                i += 1 if c == "\\" else 0
                in_str = c != '"'
            elif c == '"':
                in_str = True
            elif c == "(":
                depth += 1
            elif c == ")":
                depth -= 1
            elif c == "," and depth == 1 and comma is None:
                comma = i
            i += 1
        msg = text[comma + 1:i - 1]
        msg = re.sub(r'"\s+"', "", msg)                       # "a" "b" is one literal
        out += [s for s in _LITERAL.findall(msg) if s.strip()]
    return out


def test_the_parser_reads_an_assert_as_the_compiler_does():
    text = 'FA_ASSERT(f(a, b) && c == d, packed ? "one, (two" " three" : std::string(n) + " four");\nFA_ASSERT(x, w + " five" + num(y) + ")");'
    assert _assert_messages(text) == ["one, (two three", " four", " five", ")"]


def test_every_message_of_the_bindings_is_a_recorded_first_failure():
    recorded = {v[1] for half in ("cpu", "gpu") for v in QUANT_ERRORS[half].values()}
    seen, missing = set(), {}
    for name in SOURCES:
        path = os.path.join(CSRC, name)
        if not os.path.exists(path):
            continue
        with open(path) as fh:
            for lit in _assert_messages(fh.read()):
                seen.add(lit)
                if len(lit) > 1 and lit not in EXEMPT and not any(lit in msg for msg in recorded):
                    missing.setdefault(lit, name)
    assert len(seen) >= 60, len(seen)            # the scan sees the messages, wherever the fold has put them
    assert not missing, missing
    assert len(EXEMPT) <= 4 and set(EXEMPT) <= seen, set(EXEMPT) - seen
