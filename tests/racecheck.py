"""The poisoned repeat-launch check every race test shares, and its case tables (not a test module).

series() / check() take a `launch(outs)` callable and the outputs it writes and repeat it RUNS times on fixed inputs.
Before EVERY launch each output and each caller-owned scratch buffer (split workspace, ragged plan, q_scaled) is filled
with 0xFF bytes -- a NaN in fp32, fp16 and bf16, -1 in the int32 plan -- and then, by mode,

    nan     fa_debug_poison runs: NaN patterns in every CU's LDS and in every vector / accumulator register;
    decoy   the same entry point runs once on independent inputs of the same shape (another seed) into scratch outputs:
            plausible FINITE stale data in LDS and registers, for the paths that swallow a stale NaN (the kernels'
            fmaxf drops a NaN operand).

The first result may hold no NaN where the kernel owns the element (rows past cu_seqlens[batch] must keep the fill), a
cache output must equal its reference byte for byte, every later result must equal the first bit for bit
(blockcheck.same_bits), and so must one launch made without poison or decoy ("plain" in the list of changed runs).  If
runs change, the caller's control -- the barrier-synchronised family-1 plain kernel for training cases, the same call at
one forced split for decode cases -- is repeated the same way: the check skips only if the control changes too (the card
does not reproduce its own results, tests/conftest.py), otherwise it fails and names the changed runs.  A case that IS its
control (a forced family 1, a decode call at one forced split) passes control=None: there a changed run fails, always.  Once per case the
unpoisoned result is checked against attn_ref.attention_fp64 under the bounds of the kernel's own test file.

The case tables and the problems behind them are tests/racecases.py.  With MI355FA_RACE_JSONL=path in the environment every
check appends a line (id, stems, mode, runs, seconds, changed runs, control) to that file.
"""
import ctypes
import json
import os
import time

import pytest
import torch

import blockcheck as bc

F16, BF16 = torch.float16, torch.bfloat16
RUNS = 120
MODES = ("nan", "decoy")
DT = {F16: "fp16", BF16: "bf16"}


# ---------------------------------------------------------------- the check
def fill_ff(t):
    """every byte of the contiguous tensor `t` = 0xFF"""
    t.view(torch.uint8).fill_(0xFF)
    return t


def _same(a, b):
    if a.element_size() in (2, 4):
        return bc.same_bits(a, b)
    return a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


class Out:
    """One output of a launch.  like: a tensor of its shape, dtype and device; init: None (0xFF bytes before every launch)
    or the tensor copied into it before every launch (a cache the call appends to); expect: the bytes a cache must hold
    after the call; owned: bool mask over the leading dimensions, the elements the kernel writes (None: all) -- the others
    must keep the fill."""

    def __init__(self, name, like, init=None, expect=None, owned=None):
        self.name, self.like, self.init, self.expect, self.owned = name, like, init, expect, owned


class Gpu:
    """the device calls of the check; tests/test_host_racecheck.py passes a stub"""

    def __init__(self):
        import _mi355fa as fa
        self.fn = fa.lib.fa_debug_poison
        self.fn.argtypes = [ctypes.c_void_p]
        self.fn.restype = ctypes.c_int

    def poison(self):
        assert self.fn(torch.cuda.current_stream().cuda_stream) == 0

    def sync(self):
        torch.cuda.synchronize()


def series(launch, outs, mode, decoy=None, scratch=(), runs=RUNS, dev=None, disturb=True):
    """One unpoisoned launch, one disturbed launch (the first result) and `runs` more: returns (the unpoisoned results,
    the changed runs: "plain" and / or the indices of the later runs whose bits are not the first result's).  Asserts
    what the first result must satisfy on its own.  disturb=False: the plain repeat without poison or decoy."""
    assert mode in MODES, mode
    assert mode != "decoy" or decoy is not None
    dev = dev or Gpu()
    bufs = lambda: [torch.empty_like(o.like) for o in outs]

    def once(xs, disturbed):
        for o, x in zip(outs, xs):
            x.copy_(o.init) if o.init is not None else fill_ff(x)
        for s in scratch:
            fill_ff(s)
        if disturbed and mode == "nan":
            dev.poison()
        elif disturbed:
            decoy()
        launch(xs)

    plain, first, later = bufs(), bufs(), bufs()
    once(plain, False)
    dev.sync()
    once(first, disturb)
    dev.sync()
    for o, x in zip(outs, first):
        if o.expect is not None:
            assert _same(x, o.expect), (o.name, "is not the reference cache byte for byte")
            continue
        nan = torch.isnan(x.float()) if x.is_floating_point() else torch.zeros_like(x, dtype=torch.bool)
        if o.owned is None:
            assert not nan.any(), (o.name, "NaN in the first result", int(nan.sum()))
        else:
            own = o.owned.to(x.device)
            assert not nan[own].any(), (o.name, "NaN in the first result", int(nan[own].sum()))
            assert _same(x[~own].contiguous(), fill_ff(torch.empty_like(x[~own].contiguous()))), (o.name, "a row no sequence owns was written")
    changed = [] if all(_same(a, b) for a, b in zip(plain, first)) else ["plain"]
    for i in range(runs):
        once(later, disturb)
        if not all(_same(a, b) for a, b in zip(first, later)):
            changed.append(i)
    return plain, changed


def record(case, mode, runs, seconds, changed, control):
    path = os.environ.get("MI355FA_RACE_JSONL")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(id=case["id"], stems=sorted(case["stems"]), mode=mode, runs=runs, seconds=round(seconds, 3),
                                    changed=changed, control=control)) + "\n")


def check(case, launch, outs, mode, decoy=None, scratch=(), control=None, runs=RUNS, dev=None):
    """series() under the control rule of the module docstring.  case: dict with "id" and "stems"; control: a callable
    that repeats the case through its control and returns that series' changed runs.  Returns dict(plain=the unpoisoned
    results, changed, control, seconds)."""
    t0 = time.time()
    changed, ctl = ["not run"], None
    try:
        plain, changed = series(launch, outs, mode, decoy, scratch, runs, dev)
        if changed and control is not None:
            ctl = control()
    finally:
        seconds = time.time() - t0
        record(case, mode, runs, seconds, changed, ctl)
    if changed and ctl:
        pytest.skip("this GPU does not reproduce its own results: the control changed in launches %s of %d too" % (ctl[:8], runs))
    assert not changed, "%s [%s]: launches %s of %d gave other bits than the first (%s)" % (
        case["id"], mode, changed[:8], runs, "the control did not" if control is not None else "this launch is the control: nothing excuses it")
    return dict(plain=plain, changed=changed, control=ctl, seconds=seconds)
