"""CPU tests of tests/racecheck.py and tests/racecases.py: the check refuses what it must (a changed element in run k, a NaN in the first result,
a first result that is not the undisturbed one, a written row no sequence owns, a cache that is not the reference) and
skips only when the control changes too -- fake launches on CPU tensors, the poison and the device calls stubbed; and its
case tables: every kernel stem of the built library is claimed by a case, every forced-family case is admitted by
fa_debug_pick / fa_debug_pick_ex, and the shapes are the edges the GPU files' docstrings name."""
import os
import re
import sys

import pytest
import torch

from conftest import ROOT
import racecases as rc      # the case tables; the names of the check (tests/racecheck.py) come with it

sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

CASE = dict(id="fake", stems=["fa_fake_kernel"])


class Dev:
    def __init__(self):
        self.poisons = self.syncs = 0

    def poison(self):
        self.poisons += 1

    def sync(self):
        self.syncs += 1


class Fake:
    """launch number n (0: the undisturbed one, 1: the first result, 2 + k: run k) writes base + what `wrong` adds"""

    def __init__(self, wrong=None, ws=None):
        self.n, self.wrong, self.ws = 0, wrong or {}, ws
        self.base = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
        self.outs = [rc.Out("O", self.base.to(torch.bfloat16)), rc.Out("LSE", self.base[..., 0].contiguous())]

    def __call__(self, xs):
        for x in xs + ([self.ws] if self.ws is not None else []):      # every output and the workspace arrive filled
            assert (x.view(torch.uint8) == 0xFF).all()
        xs[0].copy_(self.base)
        xs[1].copy_(self.base[..., 0])
        if self.ws is not None:
            self.ws.zero_()
        if self.n in self.wrong:
            self.wrong[self.n](xs)
        self.n += 1


def bump(xs):
    xs[0][1, 2, 3] += 1


def test_clean_launches_pass_and_every_launch_is_filled_and_poisoned():
    for mode in rc.MODES:
        dev, decoys = Dev(), []
        f = Fake(ws=torch.zeros(5))
        res = rc.check(CASE, f, f.outs, mode, decoy=lambda: decoys.append(1), scratch=[f.ws], control=lambda: [], runs=7, dev=dev)
        assert res["changed"] == [] and res["control"] is None and f.n == 9
        assert (dev.poisons, len(decoys)) == ((8, 0) if mode == "nan" else (0, 8))      # not before the undisturbed launch
        assert torch.equal(res["plain"][0], f.base.to(torch.bfloat16))


@pytest.mark.parametrize("mode", rc.MODES)
def test_one_changed_element_in_run_k_fails_and_names_the_run(mode):
    f = Fake({2 + 5: bump})
    with pytest.raises(AssertionError, match=r"launches \[5\] of 9"):
        rc.check(CASE, f, f.outs, mode, decoy=lambda: None, control=lambda: [], runs=9, dev=Dev())
    f = Fake({2 + 5: lambda xs: xs[1].view(torch.int32)[0, 0].bitwise_xor_(1)})       # one bit of LSE
    with pytest.raises(AssertionError, match=r"launches \[5\] of 9"):
        rc.check(CASE, f, f.outs, mode, decoy=lambda: None, control=lambda: [], runs=9, dev=Dev())


def test_a_nan_left_in_the_first_result_fails():
    def skip_one(xs):
        rc.fill_ff(xs[0][1, 2])
    f = Fake({n: skip_one for n in range(20)})         # every launch leaves the same row unwritten: bit-identical runs
    with pytest.raises(AssertionError, match="NaN in the first result"):
        rc.check(CASE, f, f.outs, "nan", control=lambda: [], runs=3, dev=Dev())


def test_a_first_result_that_is_not_the_undisturbed_one_fails():
    f = Fake({0: bump})                                 # the disturbed launches agree with each other
    with pytest.raises(AssertionError, match=r"launches \['plain'\]"):
        rc.check(CASE, f, f.outs, "nan", control=lambda: [], runs=3, dev=Dev())


def test_skips_only_when_the_control_changes_too():
    f = Fake({4: bump})
    with pytest.raises(pytest.skip.Exception, match="control changed"):
        rc.check(CASE, f, f.outs, "nan", control=lambda: [1, 3], runs=4, dev=Dev())
    f = Fake({4: bump})
    with pytest.raises(AssertionError, match="the control did not"):
        rc.check(CASE, f, f.outs, "nan", control=lambda: [], runs=4, dev=Dev())
    f = Fake({4: bump})                                 # a case that is its own control: no control, no skip
    with pytest.raises(AssertionError, match="nothing excuses it"):
        rc.check(CASE, f, f.outs, "nan", control=None, runs=4, dev=Dev())
    called = []
    f = Fake()
    rc.check(CASE, f, f.outs, "nan", control=lambda: called.append(1) or [2], runs=4, dev=Dev())
    assert not called                                   # a clean series never consults the control


def test_rows_no_sequence_owns_must_keep_their_fill_and_a_cache_its_reference():
    own = torch.tensor([True, False])

    def two_rows(xs):
        xs[0][1].fill_(float("nan"))
        rc.fill_ff(xs[1][1])
    f = Fake({n: two_rows for n in range(20)})
    f.outs = [rc.Out("O", f.outs[0].like, owned=own), rc.Out("LSE", f.outs[1].like, owned=own)]
    with pytest.raises(AssertionError, match="a row no sequence owns was written"):      # a NaN, but not the fill's bytes
        rc.check(CASE, f, f.outs, "nan", control=lambda: [], runs=2, dev=Dev())
    f.n, f.wrong = 0, {n: (lambda xs: (rc.fill_ff(xs[0][1]), rc.fill_ff(xs[1][1]))) for n in range(20)}
    rc.check(CASE, f, f.outs, "nan", control=lambda: [], runs=2, dev=Dev())
    # a cache: copied in before every launch, compared with the reference after it
    cache = torch.arange(8, dtype=torch.uint8).view(torch.float8_e4m3fn)
    want = cache.clone()
    want.view(torch.uint8)[3] = 0x55

    def append(byte):
        def launch(xs):
            assert torch.equal(xs[0].view(torch.uint8), cache.view(torch.uint8))
            xs[0].view(torch.uint8)[3] = byte
        return launch
    outs = [rc.Out("K cache", cache, init=cache, expect=want)]
    rc.check(CASE, append(0x55), outs, "nan", control=lambda: [], runs=2, dev=Dev())
    with pytest.raises(AssertionError, match="reference cache"):
        rc.check(CASE, append(0x54), outs, "nan", control=lambda: [], runs=2, dev=Dev())


def test_records_one_line_per_check(tmp_path, monkeypatch):
    import json
    path = tmp_path / "race.jsonl"
    monkeypatch.setenv("MI355FA_RACE_JSONL", str(path))
    f = Fake({3: bump})
    with pytest.raises(AssertionError):
        rc.check(CASE, f, f.outs, "nan", control=lambda: [], runs=4, dev=Dev())
    f = Fake()
    rc.check(CASE, f, f.outs, "decoy", decoy=lambda: None, control=lambda: [], runs=4, dev=Dev())
    a, b = (json.loads(x) for x in path.read_text().splitlines())
    assert (a["id"], a["mode"], a["runs"], a["changed"], a["control"], a["stems"]) == ("fake", "nan", 4, [1], [], ["fa_fake_kernel"])
    assert (b["mode"], b["changed"], b["control"]) == ("decoy", [], None) and b["seconds"] >= 0
    # the summary of a run: a line per (table, stems, mode); what changed stays named by its check
    rc.check(dict(CASE, id="fake2"), f, f.outs, "decoy", decoy=lambda: None, control=lambda: [], runs=4, dev=Dev())
    s, t = (json.loads(x) for x in rc.summarise(path.read_text().splitlines()))
    assert (s["mode"], s["checks"], s["runs"], s["changed"], s["control"]) == ("nan", 1, 4, {"fake": [1]}, {"fake": []})
    assert (t["mode"], t["checks"], t["changed"], t["control"], t["stems"]) == ("decoy", 2, {}, {}, ["fa_fake_kernel"])


# ---------------------------------------------------------------- the case tables
def all_cases():
    return rc.FAMILY_CASES + rc.HEADLINE_CASES + rc.VARIANT_CASES + rc.DECODE_CASES


def test_every_kernel_of_the_library_is_claimed_by_a_case():
    built = {re.search(r"(fa_[a-z0-9_]+?_kernel)", k["name"]).group(1) for k in codeobj.kernels()}
    assert len(built) >= 28 and "fa_poison_kernel" in built
    claimed = {s for c in all_cases() for s in c["stems"]}
    assert all(c["stems"] for c in all_cases())
    assert built - {"fa_poison_kernel"} == claimed, (sorted(built - claimed), sorted(claimed - built))
    ids = [c["id"] for c in all_cases()]
    assert len(set(ids)) == len(ids) and len(rc.ALL_CASES) == len(ids)


def test_every_forced_family_case_is_admitted():
    """fa_debug_pick and fa_debug_pick_ex answer the forced family: the case runs the kernel it names.  The headline table
    keeps the one launch family 4 does not take (the fp16 causal dK/dV: no instance), which tests/test_gpu_race.py skips."""
    try:
        for c in rc.FAMILY_CASES + rc.HEADLINE_CASES:
            rc.force(c["kern"], c["fam"])
            if c.get("headline") and (c["kern"], c["dtype"], c["causal"]) == ("dkv", rc.F16, True):
                assert rc.picked(c) == (3, 3)
                continue
            assert rc.picked(c) == (c["fam"], c["fam"]), (c["id"], rc.picked(c))
            assert c["stems"] == [rc.STEMS[c["kern"], c["fam"]]]
    finally:
        rc.force(None, 0)
    # every instance the library has: (kernel, family, D, dtype, mask)
    have = {(c["kern"], c["fam"], c["D"], c["dtype"], c["causal"]) for c in rc.FAMILY_CASES}
    want = {(k, f, D, t, m) for (k, f), g in rc.GEOMETRY.items() for D in g["D"] for t in (rc.F16, rc.BF16) for m in (False, True)}
    assert want - have == {("dkv", 4, 64, rc.F16, True)}
    per_stem = {}
    for k in codeobj.kernels():
        stem = re.search(r"(fa_[a-z0-9_]+?_kernel)", k["name"]).group(1)
        per_stem[stem] = per_stem.get(stem, 0) + 1
    for (k, f), g in rc.GEOMETRY.items():
        if f != 1:       # (family 1 also has its dropout and occupancy instances)
            assert per_stem[rc.STEMS[k, f]] == len([x for x in have if x[:2] == (k, f)]), (k, f)


def test_family_shapes_reach_the_edges():
    by = {}
    for c in rc.FAMILY_CASES:
        by.setdefault((c["kern"], c["fam"], c["D"], c["dtype"], c["causal"]), []).append(c)
    for (kern, fam, D, dtype, causal), cases in by.items():
        g = rc.GEOMETRY[kern, fam]
        T, R, BM = g["T"][D], g["R"][D], g["BM"]
        streamed = lambda c: c["Sq"] if kern == "dkv" else c["Sk"]
        resident = lambda c: c["Sk"] if kern == "dkv" else c["Sq"]
        tiles = {-(-streamed(c) // T) for c in cases}
        key = (kern, fam, D, causal)
        if fam == 4 and causal and kern == "dkv":
            # S_q in 128-row tiles at or above S_k, S_k in 256-key tiles (fa_kernels.h pick_dkv_impl): key tile j streams
            # S_q / 128 - 2 j - 2 query tiles behind its two diagonal ones -- none, 1, 2, R and R + 1 of them
            assert all(c["Sq"] % 128 == 0 and c["Sk"] % 256 == 0 and c["Sq"] >= c["Sk"] for c in cases), key
            past = {c["Sq"] // 128 - 2 * j - 2 for c in cases for j in range(c["Sk"] // 256)}
            assert {0, 1, 2, R, R + 1} <= past and {2, 3, R + 2, R + 3} <= tiles, (key, past, tiles)
        elif fam == 4 and causal:        # S_k in multiples of 256 only: 2 and 4 tiles of 128, 4 .. 16 of 64
            assert {256 // T, 512 // T, 768 // T, 1024 // T} <= tiles, key
        else:
            assert {1, 2, R, R + 1} <= tiles, key
        if fam != 4 or (kern == "fwd" and not causal):
            assert any(streamed(c) % T for c in cases) and any(streamed(c) % T == 0 for c in cases), key
            assert any(resident(c) % BM and resident(c) > 2 * BM for c in cases), key
        if not (fam == 4 and kern == "dkv"):
            assert any(resident(c) < BM for c in cases), key
        if causal:
            assert any(c["Sq"] < c["Sk"] for c in cases) or kern == "dkv" and fam == 4, key
            assert any(c["Sq"] > c["Sk"] for c in cases) or kern != "dkv" and fam == 4, key
        assert all(c["B"] * c["H"] == 6 for c in cases if not re.search("busy|grid", c["id"])), key
        busy = [c for c in cases if c["id"].endswith("busy")]
        assert len(busy) == 1 and busy[0]["H"] == 32 and busy[0]["B"] >= 4, key
        b = busy[0]
        assert rc.workgroups(kern, fam, b["B"], 32, b["Sq"], b["Sk"], causal) > 512 and -(-streamed(b) // T) >= R + 1, key
        if fam == 4:
            P = rc.PERSISTENT_GRID
            items = lambda c: rc.family4_items(kern, c["B"], c["H"], c["Sq"], c["Sk"], causal)
            assert all(items(c) < P for c in cases if c["B"] * c["H"] == 6), key
            one_or_two = [c for c in cases if c["id"].endswith("grid-1or2")]
            three = [c for c in cases if c["id"].endswith("grid-3plus")]
            assert len(one_or_two) == 1 and P < items(one_or_two[0]) < 2 * P, key
            assert len(three) == 1 and items(three[0]) >= 3 * P and three[0]["Sq"] == three[0]["Sk"] == 256, key
    assert rc.PERSISTENT_GRID == __import__("test_gpu_families").cu_count()


def test_variant_and_decode_tables_hold_what_their_files_name():
    mods = [c for c in rc.VARIANT_CASES if c["kind"] == "mod"]
    for variant, D, dtype in __import__("itertools").product(rc.VARIANTS, (64, 128), (rc.F16, rc.BF16)):
        mine = [c for c in mods if (c["variant"], c["D"], c["dtype"]) == (variant, D, dtype)]
        for kern in ("fwd", "dq", "dkv"):
            assert {c["window"] for c in mine if c["kern"] == kern} == set(rc.WINDOWS) == {(-1, -1), (-1, 0), (70, 0), (40, 25)}
            if dtype == rc.BF16 and kern != "fwd":
                assert {c["ws"] for c in mine if c["kern"] == kern} == {False, True}
        assert any(c["kern"] == "dsink" for c in mine) == (variant == "sink")
        assert all((c["B"], c["Sq"], c["Sk"]) == (2, 200, 333) for c in mine)
    assert {v: rc.VARIANTS[v][:2] for v in rc.VARIANTS} == dict(window=(6, 6), gqa4=(8, 2), gqa3=(6, 2), softcap=(6, 2), alibi=(6, 2),
                                                                sink=(6, 2))
    for kind in ("dropout", "packed", "packed-mod"):
        got = {(c["kern"], c["D"], c["dtype"]) for c in rc.VARIANT_CASES if c["kind"] == kind}
        assert len(got) == 12, kind
    assert rc.PACKED_LENS == [(0, 5), (37, 37), (200, 333), (64, 1)] and rc.DROPOUT[0] == 0.25
    # decode: every case runs all twelve (splits, S_q) pairs; a ragged one every split count over its packed query counts
    for c in rc.DECODE_CASES:
        if c["layout"] == "ragged":
            assert c["configs"] == [(n, None) for n in (0, 1, 3, 7)], c["id"]
        else:
            assert sorted(c["configs"]) == [(n, s) for n in (0, 1, 3, 7) for s in (1, 4, 9)], c["id"]
    have = {(c["layout"], c["variant"], c["D"], c["dtype"], c["page"]) for c in rc.DECODE_CASES}
    inst = {(D, t) for D in (64, 128) for t in (rc.F16, rc.BF16)}
    for v in rc.DECODE_VARIANTS:
        assert {(D, t) for lay, vv, D, t, _ in have if lay == "padded" and vv == v} == inst
        assert {(D, t, p) for lay, vv, D, t, p in have if lay == "paged" and vv == v} == {(D, t, p) for D, t in inst for p in (32, 64)}
    for v in ("plain", "fp8_sink"):
        assert {(D, t, p) for lay, vv, D, t, p in have if lay == "ragged" and vv == v} == {(D, t, p) for D, t in inst for p in (32, 64)}
    assert {vv for lay, vv, *_ in have if lay == "ragged"} == {"plain", "fp8_sink"}
    assert any(c["window"] == (200, 0) for c in rc.DECODE_CASES) and any(c["transposed"] for c in rc.DECODE_CASES)
    assert (rc.DECODE_FILLS, rc.DECODE_NEW, rc.RAGGED_S) == ((0, 300, 650), 2, (0, 1, 9, 3))
