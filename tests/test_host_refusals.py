"""The refusals of the decode entry points, recorded before the decode host path was folded (tests/golden/decode_refusals.json,
written by tools/record_refusals.py from the library of the commit the file names) and replayed here against the in-tree
library: the ten decode calls and their six workspace functions, every distinct refusal of the shared checks, and cases with
two faults at once, which pin the order of the checks.  Return code and fa_last_error() text are compared exactly.  Every
case is refused before a launch: no GPU."""
import importlib.util
import json
import os
import re

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "decode_refusals.json")


def _tool():
    spec = importlib.util.spec_from_file_location("record_refusals", os.path.join(ROOT, "tools", "record_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_recorded_refusals_are_replayed_exactly():
    tool = _tool()
    doc = json.load(open(GOLDEN))
    want = doc["cases"]
    assert re.fullmatch(r"[0-9a-f]{40}", doc["commit"]), "the file names the commit its library was built from"
    assert sorted(want) == sorted(cid for cid, _, _ in tool.CASES), "the tool's list and the recorded one differ"
    got = tool.Replay().table()
    bad = {cid: (want[cid], got[cid]) for cid in want if got[cid] != want[cid]}
    assert not bad, (len(bad), sorted(bad.items())[:5])


def test_the_list_covers_what_it_must():
    tool = _tool()
    want = json.load(open(GOLDEN))["cases"]
    assert all(rc < 0 and text for rc, text in want.values())
    fns = {fn for _, fn, _ in tool.CASES}
    assert fns == set(tool.CALLS) | set(tool.WS) and len(tool.CALLS) == 10 and len(tool.WS) == 6
    two = [cid for cid, _, kw in tool.CASES if "/two:" in cid]
    assert len(two) >= 12 and len({want[cid][1].split(": ", 1)[1] for cid in two}) >= 12     # a dozen different first refusals
    # every refusal text in the decode part of csrc/fa_api.hip is reached by some case (a literal that spans lines is matched
    # by its first line), apart from those of the two functions there that are no decode call
    src = open(os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd", "csrc", "fa_api.hip")).read()
    decode = src[src.index("// ---- decoding attention over a padded KV cache"):]
    texts = set(re.findall(r'"%s: ([^"%]+)"', decode))
    assert len(texts) > 40
    reached = {text.split(": ", 1)[1] for _, text in want.values()}
    unreached = {t for t in texts if not any(r.startswith(t) for r in reached)}
    assert unreached <= {"total_q, B and H must be >= 1, H * total_q and B at most 2^24",              # fa_debug_ragged_plan
                         "dsinks must be 4-byte aligned", "lse and delta must be 16-byte aligned",      # fa_bwd_dsink
                         "total tokens must be >= 1", "B, H, S_q must be >= 1"}, unreached
