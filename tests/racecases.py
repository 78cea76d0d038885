"""The case tables of the race tests and the problems behind them (not a test module); the check is tests/racecheck.py.

The case tables: FAMILY_CASES (plain entry points with the family forced, tests/test_gpu_race_families.py), HEADLINE_CASES
(tests/test_gpu_race.py), VARIANT_CASES (the family-1 *_mod instances, dropout and packed batches,
tests/test_gpu_race_variants.py) and DECODE_CASES (tests/test_gpu_race_decode.py).  Every case lists the kernel stems it
launches; tests/test_host_racecheck.py holds the tables to the built library and to fa_debug_pick_ex on the CPU, and
tools/race_stress.py --case ID runs one case with any number of runs.  profiles/race_cases.jsonl is summarise() of a full
run's lines (tools/race_stress.py --summarise FILE).
"""
import ctypes
import functools
import itertools
import json

import pytest
import torch

import attn_ref as ar
import blockcheck as bc
from racecheck import BF16, DT, F16, MODES, RUNS, Out, check, fill_ff, series  # noqa: F401  (the tests reach the check through here)


# ---------------------------------------------------------------- the library's debug hooks
def _lib():
    import _mi355fa as fa
    lib = fa.lib
    lib.fa_debug_force_impl.argtypes = [ctypes.c_int] * 3
    lib.fa_debug_force_impl.restype = None
    lib.fa_debug_pick.argtypes = [ctypes.c_int] * 8
    lib.fa_debug_pick.restype = ctypes.c_int
    lib.fa_debug_pick_ex.argtypes = [ctypes.c_int] * 11
    lib.fa_debug_pick_ex.restype = ctypes.c_int
    return fa, lib


KERNELS = ("fwd", "dq", "dkv")
STEMS = {("fwd", 1): "fa_fwd_kernel", ("fwd", 2): "fa_fwd2_kernel", ("fwd", 3): "fa_fwd3_kernel", ("fwd", 4): "fa_fwd4_kernel",
         ("dq", 1): "fa_bwd_dq_kernel", ("dq", 3): "fa_bwd_dq3_kernel", ("dq", 4): "fa_bwd_dq4_kernel",
         ("dkv", 1): "fa_bwd_dkv_kernel", ("dkv", 2): "fa_bwd_dkv2_kernel", ("dkv", 3): "fa_bwd_dkv3_kernel",
         ("dkv", 4): "fa_bwd_dkv4_kernel"}


def force(kern, fam):
    """pin `kern`'s schedule family (the two other kernels follow the automatic rule); kern None: nothing pinned"""
    _lib()[1].fa_debug_force_impl(*(fam if k == kern else 0 for k in KERNELS))


def picked(c):
    """(fa_debug_pick, fa_debug_pick_ex) for a family case under the current forcing"""
    lib = _lib()[1]
    a = (KERNELS.index(c["kern"]), c["D"], int(c["dtype"] == BF16), int(c["causal"]), c["B"], c["H"], c["Sq"], c["Sk"])
    return lib.fa_debug_pick(*a), lib.fa_debug_pick_ex(*a, 0, 1, 0)


# ---------------------------------------------------------------- plain entry points, the family forced
# (kernel, family) -> the head dims it has an instance for, the streamed tile T, the ring depth R (the kernel's *Cfg) and
# the resident side's workgroup tile.  The streamed side is the keys for the forward and dQ, the queries for dK/dV.
GEOMETRY = {
    ("fwd", 1): dict(D=(64, 128), T={64: 64, 128: 64}, R={64: 2, 128: 2}, BM=128),
    ("fwd", 2): dict(D=(64,), T={64: 64}, R={64: 3}, BM=256),
    ("fwd", 3): dict(D=(64,), T={64: 64}, R={64: 3}, BM=128),
    ("fwd", 4): dict(D=(64, 128), T={64: 128, 128: 64}, R={64: 3, 128: 4}, BM=256),
    ("dq", 1): dict(D=(64, 128), T={64: 64, 128: 64}, R={64: 2, 128: 2}, BM=128),
    ("dq", 3): dict(D=(64,), T={64: 64}, R={64: 3}, BM=128),
    ("dq", 4): dict(D=(64,), T={64: 128}, R={64: 3}, BM=256),
    ("dkv", 1): dict(D=(64, 128), T={64: 64, 128: 64}, R={64: 2, 128: 2}, BM=128),
    ("dkv", 2): dict(D=(64, 128), T={64: 128, 128: 128}, R={64: 2, 128: 2}, BM=128),
    ("dkv", 3): dict(D=(64,), T={64: 128}, R={64: 2}, BM=256),
    ("dkv", 4): dict(D=(64,), T={64: 128}, R={64: 3}, BM=256),
}
PERSISTENT_GRID = 256     # fa_kernels.h persistent_grid on the MI355X: one workgroup per CU


def family4_items(kern, B, H, Sq, Sk, causal):
    """work items of a family-4 launch: 256-row (dK/dV: 256-key) tiles per (batch, head), causal tile pairs (i, n-1-i)
    when the launcher pairs -- the forward always, dQ and dK/dV by fa_kernels.h want_pairs"""
    n = -(-(Sk if kern == "dkv" else Sq) // 256)
    pair = causal and (kern == "fwd" or ((n + 1) // 2) * B * H >= 256)
    return ((n + 1) // 2 if pair else n) * B * H


def workgroups(kern, fam, B, H, Sq, Sk, causal):
    """workgroups of a launch of families 1-3 (blockcheck.grid_size), work items of a family-4 launch"""
    if fam == 4:
        return family4_items(kern, B, H, Sq, Sk, causal)
    return bc.grid_size(KERNELS.index(kern), fam, B, H, Sq, Sk, causal)


def _orient(kern, streamed, resident):
    """(S_q, S_k) from the streamed and the resident side"""
    return (streamed, resident) if kern == "dkv" else (resident, streamed)


def family_shapes(kern, fam, D, dtype, causal):
    """[(tag, B, H, S_q, S_k)] of one kernel instance (module docstring of tests/test_gpu_race_families.py)"""
    g = GEOMETRY[kern, fam]
    T, R, BM = g["T"][D], g["R"][D], g["BM"]
    ladder = sorted({1, 2, R, R + 1})
    out = []
    if fam != 4 or (kern == "fwd" and not causal):
        # every size is admitted: whole tiles and a ragged tail on the streamed side
        for n in ladder:
            for s in (n * T, n * T - 11):
                out.append(("t%d-%d" % (n, s), 2, 3) + (_orient(kern, s, BM + 37) if not causal else (s, s)))
        top = (R + 1) * T - 11
        if not causal:
            out.append(("res37", 2, 3) + _orient(kern, top, 37))
            out.append(("res2x", 2, 3) + _orient(kern, top, 2 * BM + 37))
        else:
            lo = max(top, BM + 37)
            out.append(("sq<sk", 2, 3, lo, lo + BM + 27))
            out.append(("sq>sk", 2, 3, lo + BM + 27, lo))
        S = 1000 if BM == 128 else 1100
        busy = [S, S]
    elif kern == "fwd" or kern == "dq":
        # family 4, causal (and dQ): S_k in whole 128-key tiles, under the mask S_k % 256 == 0 and >= S_q rounded up to 256
        if causal:
            for s in (256, 512, 768, 1024):
                out += [("k%d" % s, 2, 3, s, s), ("k%d-ragged-q" % s, 2, 3, s - 11, s)]
            out += [("sq<sk", 2, 3, 256, 512), ("res37", 2, 3, 37, 256)]
        else:
            for n in ladder:
                out.append(("t%d-%d" % (n, n * T), 2, 3, BM + 37, n * T))
            out += [("res37", 2, 3, 37, (R + 1) * T), ("res2x", 2, 3, 2 * BM + 37, (R + 1) * T)]
        busy = [1024, 1024]
    else:
        # dK/dV family 4: S_q in whole 128-row tiles, S_k in whole 256-key tiles, under the mask S_q >= S_k (bf16 only).
        # The mask is top-left aligned: key tile j streams S_q / 128 - 2 j - 2 query tiles behind its two diagonal ones --
        # an even number while S_q is a multiple of 256; S_q = 384 and 640 give 1 and 3 (= R), 768 gives 4 (= R + 1)
        if causal:
            for s in (256, 512, 768, 1024):
                out.append(("q%d" % s, 2, 3, s, s))
            out += [("sq>sk", 2, 3, 512, 256), ("sq>>sk", 2, 3, 1024, 256), ("past1", 2, 3, 384, 256), ("past3", 2, 3, 640, 256),
                    ("past4", 2, 3, 768, 256)]
        else:
            for n in ladder:
                out.append(("t%d-%d" % (n, n * T), 2, 3, n * T, 256))
            out += [("res3x", 2, 3, (R + 1) * T, 768)]
        busy = [1024, 1024]
    # the busy case: more than 512 workgroups (work items), at least R + 1 streamed tiles
    B = next(b for b in (4, 5, 6, 8, 10, 12, 16, 24) if workgroups(kern, fam, b, 32, busy[0], busy[1], causal) > 512)
    out.append(("busy", B, 32, busy[0], busy[1]))
    if fam == 4:
        # the persistent grid: fewer items than workgroups (every B2.H3 case above), one or two passes per workgroup, at
        # least three passes -- at the smallest admissible S (one 256-row tile per (batch, head))
        out.append(("grid-1or2", 3, 128, 256, 256))
        out.append(("grid-3plus", 4, 200, 256, 256))
    return out


def _family_cases():
    cases = []
    for (kern, fam), g in GEOMETRY.items():
        for D, dtype, causal in itertools.product(g["D"], (F16, BF16), (False, True)):
            if (kern, fam) == ("dkv", 4) and causal and dtype == F16:
                continue                      # no instance: the fp16 causal dK/dV stays with family 3 (fa_bwd_dkv_v4.hip)
            for tag, B, H, Sq, Sk in family_shapes(kern, fam, D, dtype, causal):
                cid = "%s%d-d%d-%s-%s-%s" % (kern, fam, D, DT[dtype], "causal" if causal else "full", tag)
                cases.append(dict(id=cid, kern=kern, fam=fam, D=D, dtype=dtype, causal=causal, B=B, H=H, Sq=Sq, Sk=Sk,
                                  stems=[STEMS[kern, fam]]))
    return cases


FAMILY_CASES = _family_cases()
# tests/test_gpu_race.py: family 4 at the headline shape (BASELINE configs[2] / [3]: 1024-2048 work items, 4-8 passes per
# persistent workgroup), uniform randn inputs
HEADLINE_CASES = [dict(id="%s-%s-%s" % (name, DT[dtype], "causal" if causal else "full"), kern=kern, fam=4, D=D, dtype=dtype,
                       causal=bool(causal), B=4, H=32, Sq=4096, Sk=4096, stems=[STEMS[kern, 4]], headline=True)
                  for (kern, D, name), dtype, causal in itertools.product(
                      (("fwd", 64, "fwd"), ("dq", 64, "dq"), ("dkv", 64, "dkv"), ("fwd", 128, "fwd-d128")), (BF16, F16), (1, 0))]


def _plain_inputs(c, seed):
    B, H, Sq, Sk, D, dtype = c["B"], c["H"], c["Sq"], c["Sk"], c["D"], c["dtype"]
    if c.get("headline"):
        g = torch.Generator(device="cuda").manual_seed(c["Sq"] + int(c["causal"]) + seed)
        Q, dO = (torch.randn(B, H, Sq, D, device="cuda", generator=g).to(dtype) for _ in range(2))
        K, V = (torch.randn(B, H, Sk, D, device="cuda", generator=g).to(dtype) for _ in range(2))
        return Q, K, V, dO, None
    return bc.make_inputs(B, H, H, Sq, Sk, D, dtype, seed)


class PlainProblem:
    """fa_fwd / fa_bwd_dq / fa_bwd_dkv on one set of inputs; O, LSE and delta from the automatic rule for the backward"""

    def __init__(self, c, seed):
        fa, lib = _lib()
        self.c, self.lib = c, lib
        self.Q, self.K, self.V, self.dO, self.groups = _plain_inputs(c, seed)
        self.dims = (c["B"], c["H"], c["Sq"], c["Sk"], c["D"], int(c["dtype"] == BF16), int(c["causal"]), c["D"] ** -0.5)
        self.O, self.LSE = torch.empty_like(self.Q), torch.empty(c["B"], c["H"], c["Sq"], device="cuda")
        self.dQ, self.delta = torch.empty_like(self.Q), torch.empty_like(self.LSE)
        force(None, 0)
        self.launch("fwd", [self.O, self.LSE])
        self.launch("dq", [self.dQ, self.delta])
        self.outs = {"fwd": [Out("O", self.Q), Out("LSE", self.LSE)], "dq": [Out("dQ", self.Q), Out("delta", self.LSE)],
                     "dkv": [Out("dK", self.K), Out("dV", self.V)]}[c["kern"]]
        self.scratch_outs = [torch.empty_like(o.like) for o in self.outs]

    def launch(self, kern, xs):
        P = lambda t: t.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        Q, K, V, dO = self.Q, self.K, self.V, self.dO
        if kern == "fwd":
            rc = self.lib.fa_fwd(P(Q), P(K), P(V), P(xs[0]), P(xs[1]), *self.dims, st)
        elif kern == "dq":
            rc = self.lib.fa_bwd_dq(P(Q), P(K), P(V), P(self.O), P(dO), P(self.LSE), P(xs[0]), P(xs[1]), *self.dims, st)
        else:
            rc = self.lib.fa_bwd_dkv(P(Q), P(K), P(V), P(dO), P(self.LSE), P(self.delta), P(xs[0]), P(xs[1]), *self.dims, st)
        assert rc == 0, (kern, rc)


def check_plain_truth(c, p, got):
    """the unpoisoned result against attention_fp64 under tests/test_gpu_families.py's bounds"""
    from test_gpu_families import BOUNDS
    vis = ar.visible(c["Sq"], c["Sk"], -1, 0 if c["causal"] else -1, "cuda")
    gt = ar.attention_fp64(p.Q, p.K, p.V, p.dO, c["D"] ** -0.5, vis)
    # that file's LSE bound a + u * SABS is stated for its reference's SABS (fa_oracle.attention_fp64_chunked): per row the
    # largest sum_d |q_d k_d| * scale over the visible keys, the scale of a score's rounding error -- not the largest |score|
    sabs = (p.Q.double().abs() @ p.K.double().abs().transpose(-1, -2)) * c["D"] ** -0.5
    gt["SABS"] = sabs.masked_fill(~vis, 0.0).amax(-1)
    names = {"fwd": ("O", "LSE"), "dq": ("dQ", "delta"), "dkv": ("dK", "dV")}[c["kern"]]
    res = dict(zip(names, got))
    if c["kern"] == "dq":
        res["O"] = p.O
    few = bc.few_rows(vis)
    if p.groups is None:      # uniform inputs: no structural zeros, one group
        return bc.check_outputs(c["id"], gt, res, p.dO, None, None, c["dtype"], "raw", BOUNDS, few=few)
    return bc.check_outputs(c["id"], gt, res, p.dO, p.groups, p.groups, c["dtype"], "raw", BOUNDS, V=p.V, few=few)


def run_family_case(c, modes=MODES, runs=RUNS, truth=True, admitted=True):
    """A FAMILY_CASES / HEADLINE_CASES entry in every mode.  admitted: the forced family must take the launch (an
    assertion); False keeps tests/test_gpu_race.py's skip for a launch family 4 does not take."""
    kern, fam = c["kern"], c["fam"]
    try:
        p, d = PlainProblem(c, 1), PlainProblem(c, 2)
        force(kern, fam)
        if not admitted and picked(c)[0] != fam:
            pytest.skip("family %d does not take this launch (fa_kernels.h)" % fam)
        assert picked(c) == (fam, fam), (c["id"], "the forced family does not take this launch", picked(c))

        def control(mode):
            force(kern, 1)
            try:
                return series(lambda xs: p.launch(kern, xs), p.outs, mode, lambda: d.launch(kern, d.scratch_outs), runs=runs)[1]
            finally:
                force(kern, fam)
        res = {}
        for mode in modes:
            res[mode] = check(c, lambda xs: p.launch(kern, xs), p.outs, mode, decoy=lambda: d.launch(kern, d.scratch_outs),
                              control=functools.partial(control, mode) if fam != 1 else None, runs=runs)   # family 1 IS the control
        if truth:
            check_plain_truth(c, p, res[modes[0]]["plain"])
        return res
    finally:
        force(None, 0)


# ---------------------------------------------------------------- the family-1 *_mod instances, dropout, packed batches
WINDOWS = [(-1, -1), (-1, 0), (70, 0), (40, 25)]
PACKED_LENS = [(0, 5), (37, 37), (200, 333), (64, 1)]
MOD_STEMS = {"fwd": "fa_fwd_mod_kernel", "dq": "fa_bwd_dq_mod_kernel", "dkv": "fa_bwd_dkv_mod_kernel", "dsink": "fa_bwd_dsink_kernel"}
# variant -> (H, H_kv, the (fwd, dQ, dK/dV) entry points)
VARIANTS = {
    "window": (6, 6, ("fa_fwd_local", "fa_bwd_dq_local", "fa_bwd_dkv_local")),
    "gqa4": (8, 2, ("fa_fwd_gqa", "fa_bwd_dq_gqa", "fa_bwd_dkv_gqa")),
    "gqa3": (6, 2, ("fa_fwd_gqa", "fa_bwd_dq_gqa", "fa_bwd_dkv_gqa")),
    "softcap": (6, 2, ("fa_fwd_softcap", "fa_bwd_dq_softcap", "fa_bwd_dkv_softcap")),
    "alibi": (6, 2, ("fa_fwd_alibi", "fa_bwd_dq_alibi", "fa_bwd_dkv_alibi")),
    "sink": (6, 2, ("fa_fwd_sink", "fa_bwd_dq_gqa", "fa_bwd_dkv_gqa")),
}
# The soft cap of the training and decode cases.  Q is scaled so that the scores' standard deviation is 0.6 cap, and bf16
# rounds the scale-folded Q to 2^-9 relative: a score of D products moves by about 1.1e-3 * 0.6 cap, which at cap = 30 is
# 2e-2 -- above the a = 1.5e-2 of tests/test_gpu_softcap.py's LSE bound on a row that sees one key (a causal row 0), where
# LSE is that score.  That file runs its causal bf16 rows at cap = 5 (3e-3, a fifth of a); so do these cases.
CAP = 5.0


def _variant_cases():
    cases = []
    for i, (variant, D, dtype) in enumerate(itertools.product(VARIANTS, (64, 128), (F16, BF16))):
        for j, window in enumerate(WINDOWS):
            for kern in ("fwd", "dq", "dkv") + (("dsink",) if variant == "sink" else ()):
                if kern == "dsink" and j:
                    continue                          # fa_bwd_dsink reads LSE and delta only: one window is every window
                for ws in ((False, True) if dtype == BF16 and kern in ("dq", "dkv") else (False,)):
                    cid = "%s-%s-d%d-%s-w%dx%d%s" % (variant, kern, D, DT[dtype], window[0], window[1], "-ws" if ws else "")
                    cases.append(dict(id=cid, kind="mod", variant=variant, kern=kern, D=D, dtype=dtype, window=window, ws=ws,
                                      B=2, Sq=200, Sk=333, stems=[MOD_STEMS[kern]]))
    for D, dtype, causal, kern in itertools.product((64, 128), (F16, BF16), (False, True), KERNELS):
        cid = "dropout-%s-d%d-%s-%s" % (kern, D, DT[dtype], "causal" if causal else "full")
        cases.append(dict(id=cid, kind="dropout", kern=kern, D=D, dtype=dtype, causal=causal, B=2, H=6, Sq=200, Sk=333,
                          stems=[STEMS[kern, 1]]))
    for D, dtype, kern in itertools.product((64, 128), (F16, BF16), KERNELS):
        cases.append(dict(id="packed-%s-d%d-%s" % (kern, D, DT[dtype]), kind="packed", kern=kern, D=D, dtype=dtype, H=6,
                          stems=[STEMS[kern, 1]]))
        cases.append(dict(id="packed-gqa3-%s-d%d-%s" % (kern, D, DT[dtype]), kind="packed-mod", variant="gqa3", kern=kern, D=D,
                          dtype=dtype, window=(-1, 0), ws=dtype == BF16 and kern != "fwd", stems=[MOD_STEMS[kern]]))
    return cases


VARIANT_CASES = _variant_cases()
DROPOUT = (0.25, 1234, 7)      # p, seed, offset


class ModProblem:
    """One set of inputs of a *_mod case through variantcheck.raw_run, stage by stage; packed: the causal packed batch."""

    def __init__(self, c, seed, packed=False):
        import variantcheck as vck
        self.vck, self.c = vck, c
        H, Hkv, self.names = VARIANTS[c["variant"]]
        D, dtype = c["D"], c["dtype"]
        self.scale = D ** -0.5
        amp = 0.6 * CAP / (self.scale * D ** 0.5) if c["variant"] == "softcap" else 1.0   # score std 0.6 cap (test_gpu_softcap._amp)
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.kw = {}
        if c["variant"] == "softcap":
            self.extra, self.kw = (CAP,), dict(cap=CAP)
        elif c["variant"] == "alibi":
            self.slopes = vck.M().alibi_slopes(H, device="cuda")
            self.extra, self.kw = (self.slopes.data_ptr(), 0), dict(slopes=self.slopes)
        elif c["variant"] == "sink":
            self.sinks = torch.linspace(0.0, 8.0, H, device="cuda", dtype=torch.float32)
            self.extra, self.kw = (self.sinks.data_ptr(),), dict(sinks=self.sinks)
        else:
            self.extra = ()
        self.dsink = self.sinks if c["variant"] == "sink" else None
        self.packed = None
        if packed:
            tq, tk = sum(a for a, _ in PACKED_LENS), sum(b for _, b in PACKED_LENS)
            self.Q = (torch.randn(tq, H, D, device="cuda", generator=g) * amp).to(dtype)
            self.K, self.V = (torch.randn(tk, Hkv, D, device="cuda", generator=g).to(dtype) for _ in range(2))
            self.dO = torch.randn(tq, H, D, device="cuda", generator=g).to(dtype)
            self.cu = [torch.tensor([0] + list(itertools.accumulate(x[i] for x in PACKED_LENS)), dtype=torch.int32, device="cuda")
                       for i in (0, 1)]
            self.packed = (self.cu[0], self.cu[1], len(PACKED_LENS), max(a for a, _ in PACKED_LENS), max(b for _, b in PACKED_LENS))
            lse = torch.empty(H, tq, device="cuda")
        else:
            self.Q, self.K, self.V, self.dO = vck.inputs(c["B"], H, Hkv, c["Sq"], c["Sk"], D, dtype, seed, amp)
            lse = torch.empty(c["B"], H, c["Sq"], device="cuda")
        Q, K, V = self.Q, self.K, self.V
        self.bufs = dict(O=torch.empty_like(Q), LSE=lse, dQ=torch.empty_like(Q), dK=torch.empty_like(K), dV=torch.empty_like(V),
                         delta=torch.empty_like(lse), qs=torch.empty_like(Q), dz=torch.empty(H, device="cuda"))
        self.run(("fwd", "dq"), self.bufs)            # what the later stages read
        names = {"fwd": ("O", "LSE"), "dq": ("dQ", "delta") + (("qs",) if c["ws"] else ()), "dkv": ("dK", "dV"), "dsink": ("dz",)}[c["kern"]]
        self.names_out = names
        self.outs = [Out(n, self.bufs[n]) for n in names]
        self.scratch_outs = [torch.empty_like(self.bufs[n]) for n in names]

    def run(self, stages, bufs):
        c = self.c
        self.vck.raw_run(self.names, self.extra, self.Q, self.K, self.V, self.dO, c["window"], self.scale, c["ws"], dsink=self.dsink,
                         bufs=bufs, stages=stages, packed=self.packed)

    def launch(self, xs):
        self.run((self.c["kern"],), dict(self.bufs, **dict(zip(self.names_out, xs))))


def _rel_bounds(c, p, gt, vis):
    """relFro bound per output of a *_mod case, from the variant's own test file: test_gpu_softcap / _alibi / _sink REL
    and RAW_BF16_DKV; test_gpu_local.rel_tol for the window and GQA files (tests/test_gpu_gqa.py: "as in test_gpu_local")"""
    import test_gpu_softcap as tsc
    import test_gpu_local as tlo
    dtype = c["dtype"]
    if c["variant"] in ("softcap", "alibi", "sink"):
        rel = {n: tsc.REL[dtype] for n in ("O", "dQ", "dK", "dV")}
    else:
        level = ar.sdpa_bf16_level(p.Q, p.K, p.V, p.dO, vis, gt) if dtype == BF16 else dict.fromkeys(("O", "dQ", "dK", "dV"))
        rel = {n: tlo.rel_tol(dtype, level[n]) for n in ("O", "dQ", "dK", "dV")}
    if dtype == BF16 and not c["ws"]:
        rel["dK"] = rel["dV"] = tsc.RAW_BF16_DKV
    return rel


def check_mod_truth(c, p, got):
    import fa_oracle as fo
    import test_gpu_softcap as tsc
    import test_gpu_alibi as tal
    import test_gpu_sink as tsk
    import test_gpu_local as tlo
    wl, wr = c["window"]
    vis = ar.visible(c["Sq"], c["Sk"], wl, wr, "cuda")
    kw = dict(p.kw)
    if "slopes" in kw:
        kw["dist"] = ar.distance(c["Sq"], c["Sk"], "cuda")
    gt = ar.attention_fp64(p.Q, p.K, p.V, p.dO, p.scale, vis, **kw)
    res = dict(zip(p.names_out, got))
    if c["kern"] == "dsink":
        err = ((res["dz"].double() - gt["dz"]).abs() / gt["den"].clamp_min(1e-300)).max().item()
        assert err <= tsk.DZ_BOUND[c["dtype"]], (c["id"], "dz", err)
        return
    rel = _rel_bounds(c, p, gt, vis)
    for n in ("O", "dQ", "dK", "dV"):
        if n in res:
            err = fo.rel_fro(gt[n], res[n])
            print(c["id"], n, "relFro %.3e (bound %.1e)" % (err, rel[n]))
            assert err <= rel[n], (c["id"], n, err, rel[n])
            zero = ~vis.any(-1) if n in ("O", "dQ") else ~vis.any(-2)      # queries without a key, keys without a query
            assert (res[n][:, :, zero] == 0).all(), (c["id"], n, "structural zeros")
    if "LSE" in res:
        L, R = res["LSE"].double(), gt["LSE"]
        fin = torch.isfinite(R)
        assert torch.equal(torch.isneginf(res["LSE"]), torch.isneginf(R)), (c["id"], "LSE = -inf exactly on the keyless rows")
        if c["variant"] in ("softcap", "alibi", "sink"):
            a, u = {"softcap": tsc, "alibi": tal, "sink": tsk}[c["variant"]].BOUNDS["LSE_BOUND"][c["dtype"]]
            assert ((L - R).abs()[fin] <= (a + u * gt["SABS"])[fin]).all(), (c["id"], "LSE")
        else:
            assert ((L - R).abs()[fin] < tlo.lse_tol(c["dtype"])).all(), (c["id"], "LSE")


class PlainExProblem:
    """fa_*_dropout (kind "dropout") or fa_*_varlen on the causal packed batch (kind "packed"), family 1 forced"""

    def __init__(self, c, seed):
        fa, lib = _lib()
        self.c, self.lib = c, lib
        D, dtype, H = c["D"], c["dtype"], c["H"]
        g = torch.Generator(device="cuda").manual_seed(seed)
        r = lambda *s: torch.randn(*s, device="cuda", generator=g).to(dtype)
        dt = int(dtype == BF16)
        if c["kind"] == "dropout":
            B, Sq, Sk = c["B"], c["Sq"], c["Sk"]
            self.Q, self.K, self.V, self.dO = r(B, H, Sq, D), r(B, H, Sk, D), r(B, H, Sk, D), r(B, H, Sq, D)
            lse = torch.empty(B, H, Sq, device="cuda")
            self.fns = (lib.fa_fwd_dropout, lib.fa_bwd_dq_dropout, lib.fa_bwd_dkv_dropout)
            self.head, self.tail = (), (B, H, Sq, Sk, D, dt, int(c["causal"]), D ** -0.5) + DROPOUT
        else:
            tq, tk = sum(a for a, _ in PACKED_LENS), sum(b for _, b in PACKED_LENS)
            self.Q, self.K, self.V, self.dO = r(tq, H, D), r(tk, H, D), r(tk, H, D), r(tq, H, D)
            lse = torch.empty(H, tq, device="cuda")
            self.cu = [torch.tensor([0] + list(itertools.accumulate(x[i] for x in PACKED_LENS)), dtype=torch.int32, device="cuda")
                       for i in (0, 1)]
            self.fns = (lib.fa_fwd_varlen, lib.fa_bwd_dq_varlen, lib.fa_bwd_dkv_varlen)
            self.head = (self.cu[0].data_ptr(), self.cu[1].data_ptr())
            self.tail = (len(PACKED_LENS), H, tq, tk, max(a for a, _ in PACKED_LENS), max(b for _, b in PACKED_LENS), D, dt, 1, D ** -0.5)
        Q, K, V = self.Q, self.K, self.V
        self.bufs = dict(O=torch.empty_like(Q), LSE=lse, dQ=torch.empty_like(Q), delta=torch.empty_like(lse),
                         dK=torch.empty_like(K), dV=torch.empty_like(V))
        self.names_out = {"fwd": ("O", "LSE"), "dq": ("dQ", "delta"), "dkv": ("dK", "dV")}[c["kern"]]
        self.launch_kern("fwd", self.bufs)
        self.launch_kern("dq", self.bufs)
        self.outs = [Out(n, self.bufs[n]) for n in self.names_out]
        self.scratch_outs = [torch.empty_like(self.bufs[n]) for n in self.names_out]

    def launch_kern(self, kern, b):
        P = lambda t: t.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        Q, K, V, dO = self.Q, self.K, self.V, self.dO
        if kern == "fwd":
            rc = self.fns[0](P(Q), P(K), P(V), P(b["O"]), P(b["LSE"]), *self.head, *self.tail, st)
        elif kern == "dq":
            rc = self.fns[1](P(Q), P(K), P(V), P(b["O"]), P(dO), P(b["LSE"]), P(b["dQ"]), P(b["delta"]), *self.head, *self.tail, st)
        else:
            rc = self.fns[2](P(Q), P(K), P(V), P(dO), P(b["LSE"]), P(b["delta"]), P(b["dK"]), P(b["dV"]), *self.head, *self.tail, st)
        assert rc == 0, (kern, rc, self.lib.fa_last_error())

    def launch(self, xs):
        self.launch_kern(self.c["kern"], dict(self.bufs, **dict(zip(self.names_out, xs))))


def check_packed_truth(c, p, got, kw=None):
    """A packed batch per sequence against attention_fp64: relFro over the whole packed tensor, structural zeros, LSE = -inf
    exactly on the keyless rows and its values elsewhere.  fa_*_varlen under tests/test_gpu_varlen.py's REL, its raw bf16
    dK / dV bound (stated per block: no whole tensor is above its worst block) and its LSE bound a + u SABS; the GQA
    instance under the packed checks' bound (variantcheck.check_packed with the variant files' REL) and
    test_gpu_local.lse_tol, the window and GQA files' LSE tolerance."""
    import fa_oracle as fo
    import test_gpu_local as tlo
    import test_gpu_softcap as tsc
    import test_gpu_varlen as tv
    plain = c["kind"] == "packed"
    bound, raw = (tv.REL[c["dtype"]], tv.PACKED_BOUNDS["BLOCK_BOUND_RAW_BF16_DKV"]) if plain else (tsc.REL[c["dtype"]], tsc.RAW_BF16_DKV)
    H = p.Q.shape[1]
    gt = {n: torch.zeros(t.shape, dtype=torch.float64, device="cuda") for n, t in (("O", p.Q), ("dQ", p.Q), ("dK", p.K), ("dV", p.V))}
    gt["LSE"] = torch.full((H, p.Q.shape[0]), float("-inf"), dtype=torch.float64, device="cuda")
    sabs = torch.zeros_like(gt["LSE"])
    cq, ck = p.cu[0].tolist(), p.cu[1].tolist()
    for i, (a, b) in enumerate(PACKED_LENS):
        if a == 0 or b == 0:
            continue
        sq, sk = slice(cq[i], cq[i + 1]), slice(ck[i], ck[i + 1])
        per = lambda t, s: t[s].permute(1, 0, 2)[None]
        r = ar.attention_fp64(per(p.Q, sq), per(p.K, sk), per(p.V, sk), per(p.dO, sq), c["D"] ** -0.5, ar.visible(a, b, -1, 0, "cuda"),
                              **(kw or {}))
        for n, s in (("O", sq), ("dQ", sq), ("dK", sk), ("dV", sk)):
            gt[n][s] = r[n][0].permute(1, 0, 2)
        gt["LSE"][:, sq] = r["LSE"][0]
        if plain:     # as in check_plain_truth: per row the largest sum_d |q_d k_d| * scale over the visible keys
            s = (per(p.Q, sq).double().abs() @ per(p.K, sk).double().abs().transpose(-1, -2)) * c["D"] ** -0.5
            sabs[:, sq] = s.masked_fill(~ar.visible(a, b, -1, 0, "cuda"), 0.0).amax(-1)[0]
    res = dict(zip(p.names_out, got))
    for n in ("O", "dQ", "dK", "dV"):
        if n in res:
            err = fo.rel_fro(gt[n], res[n])
            b = raw if (c["dtype"] == BF16 and n in ("dK", "dV") and not c.get("ws")) else bound
            print(c["id"], n, "relFro %.3e (bound %.1e)" % (err, b))
            assert err <= b, (c["id"], n, err, b)
            zero = (gt["O"] == 0).all(-1) if n in ("O", "dQ") else (gt["dV"] == 0).all(-1)
            assert (res[n][zero] == 0).all(), (c["id"], n, "structural zeros")
    if "LSE" in res:
        assert torch.equal(torch.isneginf(res["LSE"]), torch.isneginf(gt["LSE"])), c["id"]
        fin = torch.isfinite(gt["LSE"])
        err = (res["LSE"].double() - gt["LSE"]).abs()[fin]
        a, u = tv.PACKED_BOUNDS["LSE_BOUND"][c["dtype"]] if plain else (tlo.lse_tol(c["dtype"]), 0.0)
        print(c["id"], "LSE largest error %.3e (bound %.1e + %.1e SABS)" % (err.max().item(), a, u))
        assert (err <= (a + u * sabs)[fin]).all(), (c["id"], "LSE")


def check_dropout_truth(c, p, got):
    """fa_oracle's fp64 attention with the kernels' own keep mask, under tests/test_gpu_dropout.py's REL; bf16 dK / dV
    without the q_scaled workspace under that file's raw bound (stated per block: no whole tensor is above its worst block)"""
    import fa_oracle as fo
    import test_gpu_dropout as td
    gt = fo.attention_fp64_chunked(p.Q, p.K, p.V, p.dO, window=(-1, 0) if c["causal"] else None, dropout=DROPOUT)
    res = dict(zip(p.names_out, got))
    for n in ("O", "dQ", "dK", "dV"):
        if n in res:
            err = fo.rel_fro(gt[n], res[n])
            bound = td.REL[c["dtype"]] if c["dtype"] == F16 or n in ("O", "dQ") else td.SCALE_BOUNDS["BLOCK_BOUND_RAW_BF16_DKV"]
            print(c["id"], n, "relFro %.3e (bound %.1e)" % (err, bound))
            assert err <= bound, (c["id"], n, err, bound)


def _family1_control(c, mode, runs):
    """the barrier-synchronised family-1 plain forward at a *_mod case's shape"""
    H = VARIANTS[c["variant"]][0] if "variant" in c else c["H"]
    pc_ = dict(id=c["id"] + "-control", kern="fwd", fam=1, D=c["D"], dtype=c["dtype"], causal=False, B=c.get("B", 2), H=H,
               Sq=c.get("Sq", 200), Sk=c.get("Sk", 333))
    p, d = PlainProblem(pc_, 1), PlainProblem(pc_, 2)
    force("fwd", 1)
    try:
        return series(lambda xs: p.launch("fwd", xs), p.outs, mode, lambda: d.launch("fwd", d.scratch_outs), runs=runs)[1]
    finally:
        force(None, 0)


def run_variant_case(c, modes=MODES, runs=RUNS, truth=True):
    try:
        force(None, 0)
        if c["kind"] in ("dropout", "packed"):
            _lib()[1].fa_debug_force_impl(1, 1, 1)
            p, d = PlainExProblem(c, 1), PlainExProblem(c, 2)
        else:
            p, d = (ModProblem(c, s, packed=c["kind"] == "packed-mod") for s in (1, 2))
        res = {}
        for mode in modes:
            res[mode] = check(c, p.launch, p.outs, mode, decoy=lambda: d.launch(d.scratch_outs),
                              control=functools.partial(_family1_control, c, mode, runs), runs=runs)
        if truth:
            got = res[modes[0]]["plain"]
            if c["kind"] == "mod":
                check_mod_truth(c, p, got)
            elif c["kind"] == "dropout":
                check_dropout_truth(c, p, got)
            elif c["kind"] == "packed":
                check_packed_truth(c, p, got)
            elif c["kern"] != "dsink":
                check_packed_truth(c, p, got, p.kw)
        return res
    finally:
        force(None, 0)


# ---------------------------------------------------------------- the decode path
DECODE_SPLITS = (0, 1, 3, 7)
DECODE_SQ = (1, 4, 9)                   # with g = 4, S_q = 9 is two 32-row blocks
DECODE_FILLS, DECODE_NEW = (0, 300, 650), 2
RAGGED_S, RAGGED_FILLS, RAGGED_PAD = (0, 1, 9, 3), (300, 0, 650, 40), 5
DECODE_VARIANTS = ("plain", "softcap", "alibi", "sink", "fp8", "fp8_sink")


def _decode_stems(layout, variant, splits):
    fp8 = variant.startswith("fp8")
    s = {"padded": ["fa_decode_mod_kernel", "fa_kvcache_append_fp8_kernel" if fp8 else "fa_kvcache_append_kernel"],
         "paged": ["fa_decode_paged_kernel", "fa_kvcache_append_paged_fp8_kernel" if fp8 else "fa_kvcache_append_paged_kernel"],
         "ragged": ["fa_decode_ragged_kernel", "fa_decode_ragged_plan_kernel",
                    "fa_kvcache_append_ragged_fp8_kernel" if fp8 else "fa_kvcache_append_ragged_kernel"]}[layout]
    if any(n != 1 for n in splits):
        s.append("fa_decode_combine_ragged_kernel" if layout == "ragged" else "fa_decode_combine_kernel")
    return s


DECODE_CONFIGS = list(itertools.product(DECODE_SPLITS, DECODE_SQ))      # every (forced splits, S_q) pair, in every case
PAGED_INSTANCES = list(itertools.product((32, 64), (64, 128), (F16, BF16)))           # (page, D, dtype)


def _decode_cases():
    cases = []

    def add(layout, variant, D, dtype, **kw):
        configs = kw.pop("configs", DECODE_CONFIGS)
        cid = "%s-%s-d%d-%s" % (layout, variant, D, DT[dtype]) + "".join("-%s%s" % (k, v) for k, v in kw.items() if k in ("page", "tag"))
        cases.append(dict(dict(id=cid, layout=layout, variant=variant, D=D, dtype=dtype, configs=configs, window=(-1, -1), page=0,
                               transposed=False, stems=_decode_stems(layout, variant, [n for n, _ in configs])), **kw))
    for variant, D, dtype in itertools.product(DECODE_VARIANTS, (64, 128), (F16, BF16)):
        add("padded", variant, D, dtype)
    for variant, (page, D, dtype) in itertools.product(DECODE_VARIANTS, PAGED_INSTANCES):
        add("paged", variant, D, dtype, page=page)
    for variant, (page, D, dtype) in itertools.product(("plain", "fp8_sink"), PAGED_INSTANCES):
        add("ragged", variant, D, dtype, page=page, configs=[(n, None) for n in DECODE_SPLITS])
    add("padded", "plain", 64, BF16, tag="w200x0", window=(200, 0))
    add("padded", "plain", 128, F16, tag="transposed", transposed=True)
    return cases


DECODE_CASES = _decode_cases()


class DecodeProblem:
    """One decode step of a DECODE_CASES entry on one set of inputs: the raw C entry point of its layout with o, lse, the
    caches (fresh clones of NaN-padded caches, the append writes them) and the workspace owned by the caller."""

    def __init__(self, c, Sq, seed):
        import _mi355fa as fa
        import pagedcheck as pc
        import variantcheck as vck
        self.fa, self.c, self.pc = fa, c, pc
        M = vck.M()
        D, dtype, layout, variant = c["D"], c["dtype"], c["layout"], c["variant"]
        self.fp8 = variant.startswith("fp8")
        H, Hkv = 8, 2
        ragged = layout == "ragged"
        self.S = list(RAGGED_S) if ragged else None
        fills = list(RAGGED_FILLS if ragged else DECODE_FILLS)
        B = len(fills)
        new = self.S if ragged else [DECODE_NEW] * B
        self.Ls = [f + n for f, n in zip(fills, new)]
        page = c["page"]
        Sc = 700 if layout == "padded" else -(-700 // page) * page
        self.scale = D ** -0.5
        g = torch.Generator(device="cuda").manual_seed(seed * 1000 + D + (Sq or 0))
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)
        amp = 0.6 * CAP / (self.scale * D ** 0.5) if variant == "softcap" else 1.0
        if ragged:
            self.T = sum(self.S) + RAGGED_PAD
            self.q = (r(self.T, H, D) * amp).to(dtype)
            self.kn, self.vn = r(self.T, Hkv, D).to(dtype), r(self.T, Hkv, D).to(dtype)
            self.cu = torch.tensor([0] + list(itertools.accumulate(self.S)), dtype=torch.int32, device="cuda")
        else:
            self.q = (r(B, H, Sq, D) * amp).to(dtype)
            self.kn, self.vn = r(B, Hkv, DECODE_NEW, D).to(dtype), r(B, Hkv, DECODE_NEW, D).to(dtype)
        k, v = r(B, Hkv, Sc, D), r(B, Hkv, Sc, D) * (1.7 if self.fp8 else 1.0)
        self.kd = self.vd = None
        if self.fp8:
            k, self.kd = M.quantize_kv_fp8(k)
            v, self.vd = M.quantize_kv_fp8(v)
        else:
            k, v = k.to(dtype), v.to(dtype)
        # the clean caches with the new rows in place (the reference's K and V) and their bytes as the append must leave them
        kr, vr = k.clone(), v.clone()
        at = 0
        for b in range(B):
            if ragged:
                kb, vb = (x[at:at + new[b]].transpose(0, 1)[None] for x in (self.kn, self.vn))
                at += new[b]
            else:
                kb, vb = self.kn[b:b + 1], self.vn[b:b + 1]
            if self.fp8:
                kb, vb = M.quantize_kv_fp8(kb, self.kd[b:b + 1])[0], M.quantize_kv_fp8(vb, self.vd[b:b + 1])[0]
            pc._bytes(kr)[b, :, fills[b]:self.Ls[b]] = pc._bytes(kb)[0]
            pc._bytes(vr)[b, :, fills[b]:self.Ls[b]] = pc._bytes(vb)[0]
        self.kr, self.vr = kr, vr
        self.sl = torch.tensor(fills, dtype=torch.int32, device="cuda")
        if layout == "padded":
            def padded(x, lens):
                x = x.clone()
                for b, L in enumerate(lens):
                    pc.fill_nan(x[b, :, L:])
                return x
            self.k0, self.v0, self.kx, self.vx = padded(k, fills), padded(v, fills), padded(kr, self.Ls), padded(vr, self.Ls)
            if c["transposed"]:         # [B, S_cache, H_kv, D] storage seen as [B, H_kv, S_cache, D]
                self.k0, self.v0, self.kx, self.vx = (x.transpose(1, 2).contiguous() for x in (self.k0, self.v0, self.kx, self.vx))
        else:
            self.MP = Sc // page
            pages = sum(pc.pages_of(L, page) for L in self.Ls)
            (self.k0, self.v0), self.table = pc.scatter([k, v], fills, page, pages + 5, self.MP, seed, alloc=self.Ls)
            (self.kx, self.vx), _ = pc.scatter([kr, vr], self.Ls, page, pages + 5, self.MP, 0, table=self.table.cpu())
        self.mods = {}
        if variant == "softcap":
            self.mods = dict(softcap=CAP)
        elif variant == "alibi":
            self.mods = dict(alibi_slopes=M.alibi_slopes(H, device="cuda"))
        elif variant in ("sink", "fp8_sink"):
            self.mods = dict(sinks=torch.linspace(0.0, 8.0, H, device="cuda", dtype=torch.float32))
        self.B, self.H, self.Hkv, self.Sq, self.Sc = B, H, Hkv, Sq, Sc
        o = torch.empty_like(self.q)
        lse = torch.empty((H, self.T) if ragged else (B, H, Sq), device="cuda")
        own_o = own_l = None
        if ragged:
            tail = sum(self.S)
            own_o = torch.arange(self.T) < tail
            own_l = (torch.arange(self.T) < tail)[None, :].expand(H, self.T)
        self.outs = [Out("O", o, owned=own_o), Out("LSE", lse, owned=own_l),
                     Out("K cache", self.k0, init=self.k0, expect=self.kx), Out("V cache", self.v0, init=self.v0, expect=self.vx)]
        self.scratch_outs = [torch.empty_like(x.like) if x.init is None else x.init.clone() for x in self.outs]   # the decoy's
        self.ws = torch.empty(max(self.need(n) for n in (0, 7)) + 16, dtype=torch.uint8, device="cuda")
        self.keep = []

    def need(self, n=None):
        """the workspace bytes the call asks for at the forced split count in force (n: force it first)"""
        import variantcheck as vck
        fa, c = self.fa, self.c
        if n is not None:
            vck.splits(n)
        cdt = fa.PAGED_CACHE_FP8_E4M3 if self.fp8 else fa.PAGED_CACHE_16BIT
        if c["layout"] == "padded":
            f = fa.lib.fa_fwd_kvcache_fp8_workspace_bytes if self.fp8 else fa.lib.fa_fwd_kvcache_workspace_bytes
            return f(self.B, self.H, self.Hkv, self.Sq, self.Sc, DECODE_NEW, c["D"])
        if c["layout"] == "paged":
            return fa.lib.fa_fwd_kvcache_paged_workspace_bytes(self.B, self.H, self.Hkv, self.Sq, self.MP, c["page"], DECODE_NEW, c["D"], cdt)
        return fa.lib.fa_fwd_kvcache_ragged_workspace_bytes(self.T, self.B, self.H, self.Hkv, self.MP, c["page"], c["D"], cdt)

    def launch(self, xs):
        fa, c, m = self.fa, self.c, self.mods
        o, lse, kc, vc = xs
        P = lambda t: None if t is None else t.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        need = self.need()
        assert need <= self.ws.numel()
        B, H, Hkv, D = self.B, self.H, self.Hkv, c["D"]
        dt, (wl, wr) = int(c["dtype"] == BF16), c["window"]
        if c["layout"] == "padded":
            opts = None
            if c["transposed"]:
                s3 = lambda t: ctypes.cast((ctypes.c_longlong * 3)(t.stride(0), t.stride(2), t.stride(1)), ctypes.POINTER(ctypes.c_longlong))
                self.keep = [s3(kc), s3(vc)]
                opts = ctypes.byref(fa.Opts.make(k_strides=self.keep[0], v_strides=self.keep[1]))
            extra = {"plain": (), "fp8": (), "softcap": (m.get("softcap"),), "alibi": (P(m.get("alibi_slopes")), 0),
                     "sink": (P(m.get("sinks")),), "fp8_sink": (P(m.get("sinks")),)}[c["variant"]]
            name = "fa_fwd_kvcache" + {"plain": "", "fp8": "_fp8"}.get(c["variant"], "_" + c["variant"])
            tail = (self.scale, *extra, wl, wr, opts, st)
            if self.fp8:
                rc = getattr(fa.lib, name)(P(self.q), P(kc), P(vc), P(self.kn), P(self.vn), P(self.sl), P(self.kd), P(self.vd), Hkv, P(o),
                                           P(lse), P(self.ws), need, B, H, Hkv, self.Sq, self.Sc, DECODE_NEW, D, dt, fa.KV_FP8_E4M3, *tail)
            else:
                rc = getattr(fa.lib, name)(P(self.q), P(kc), P(vc), P(self.kn), P(self.vn), P(self.sl), P(o), P(lse), P(self.ws), need,
                                           B, H, Hkv, self.Sq, self.Sc, DECODE_NEW, D, dt, *tail)
        else:
            cdt = fa.PAGED_CACHE_FP8_E4M3 if self.fp8 else fa.PAGED_CACHE_16BIT
            mods = fa.PagedMods(softcap=m.get("softcap", 0.0), alibi_slopes=P(m.get("alibi_slopes")), slopes_batch_stride=0,
                                sinks=P(m.get("sinks")), k_descale=P(self.kd), v_descale=P(self.vd),
                                descale_bstride=Hkv if self.fp8 else 0)
            NP, page, MP = kc.shape[0], c["page"], self.MP
            if c["layout"] == "paged":
                name = "fa_fwd_kvcache_paged"
                rc = fa.lib.fa_fwd_kvcache_paged(P(self.q), P(kc), P(vc), P(self.kn), P(self.vn), P(self.sl), P(self.table), P(o), P(lse),
                                                 P(self.ws), need, B, H, Hkv, self.Sq, NP, page, MP, MP, DECODE_NEW, D, dt, cdt,
                                                 self.scale, wl, wr, ctypes.byref(mods), None, st)
            else:
                name = "fa_fwd_kvcache_ragged"
                rc = fa.lib.fa_fwd_kvcache_ragged(P(self.q), P(kc), P(vc), P(self.kn), P(self.vn), P(self.cu), P(self.sl), P(self.table),
                                                  P(o), P(lse), P(self.ws), need, self.T, B, H, Hkv, NP, page, MP, MP, D, dt, cdt,
                                                  self.scale, wl, wr, ctypes.byref(mods), None, st)
        fa.check(rc, name)


def check_decode_truth(c, p, got):
    """O and LSE of the unpoisoned call against attention_fp64 on the reference cache: plain and fp8 under
    tests/test_gpu_kvcache.py / test_gpu_kvcache_fp8.py's tol and check_lse, the score transforms under their files' REL and
    LSE_BOUND; a ragged step sequence by sequence (tests/test_gpu_ragged.py)"""
    import fa_oracle as fo
    import test_gpu_kvcache as tk
    import test_gpu_kvcache_fp8 as tk8
    import test_gpu_softcap as tsc
    import test_gpu_alibi as tal
    import test_gpu_sink as tsk
    variant, dtype = c["variant"], c["dtype"]
    wl, wr = c["window"]
    o, lse = got[0], got[1]
    if p.fp8:
        K, V = tk8.deq(p.kr, p.kd), tk8.deq(p.vr, p.vd)
    else:
        K, V = p.kr, p.vr
    m = p.mods
    kw = {}
    if "softcap" in m:
        kw["cap"] = m["softcap"]
    if "sinks" in m:
        kw["sinks"] = m["sinks"]
    if c["layout"] == "ragged":
        seqs, at = [], 0
        for b, s in enumerate(p.S):
            seqs.append((p.q[at:at + s].transpose(0, 1)[None], o[at:at + s].transpose(0, 1)[None], lse[:, at:at + s][None], b))
            at += s
    else:
        seqs = [(p.q, o, lse, None)]
    for q, o_, lse_, b in seqs:
        Sq = q.shape[2]
        if Sq == 0:
            continue
        sel = slice(None) if b is None else slice(b, b + 1)
        Ls = p.Ls if b is None else [p.Ls[b]]
        vis = torch.stack([ar.visible(Sq, p.Sc, wl, wr, "cuda", L=L) for L in Ls])[:, None]
        k2 = dict(kw)
        if "alibi_slopes" in m:
            k2.update(slopes=m["alibi_slopes"], dist=torch.stack([ar.distance(Sq, p.Sc, "cuda", L=L) for L in Ls])[:, None])
        gt = ar.attention_fp64(q, K[sel], V[sel], None, p.scale, vis, **k2)
        err = fo.rel_fro(gt["O"], o_)
        if variant in ("plain", "fp8"):
            Kd, Vd = (K[sel], V[sel]) if not p.fp8 else (K[sel].to(dtype), V[sel].to(dtype))
            bound = 1e-3 if dtype == F16 else max(2 * tk.sdpa_level(q, Kd, Vd, Ls, wl, wr, gt["O"]), 4e-3)
            print(c["id"], "O relFro %.3e (bound %.1e)" % (err, bound))
            assert err < bound, (c["id"], b, err, bound)
            tk.check_lse(lse_, gt["LSE"])
        else:
            mod = {"softcap": tsc, "alibi": tal, "sink": tsk, "fp8_sink": tsk}[variant]
            print(c["id"], "O relFro %.3e (bound %.1e)" % (err, mod.REL[dtype]))
            assert err <= mod.REL[dtype], (c["id"], b, err)
            fin = torch.isfinite(gt["LSE"])
            assert torch.equal(torch.isneginf(lse_), ~fin), (c["id"], b, "LSE = -inf exactly on the keyless rows")
            a, u = mod.BOUNDS["LSE_BOUND"][dtype]
            assert ((lse_.double() - gt["LSE"]).abs()[fin] <= (a + u * gt["SABS"])[fin]).all(), (c["id"], b, "LSE")
        assert (o_[(gt["O"] == 0).all(-1)] == 0).all(), (c["id"], b, "rows without a key")


def run_decode_case(c, modes=MODES, runs=RUNS, truth=True):
    import variantcheck as vck
    res = {}
    try:
        for n, Sq in c["configs"]:
            p, d = DecodeProblem(c, Sq, 1), DecodeProblem(c, Sq, 2)
            vck.splits(n)

            def control(mode):
                vck.splits(1)
                try:
                    return series(p.launch, p.outs, mode, lambda: d.launch(d.scratch_outs), [p.ws], runs)[1]
                finally:
                    vck.splits(n)
            sub = dict(c, id="%s/n%d-sq%s" % (c["id"], n, Sq))
            for mode in modes:
                res[n, Sq, mode] = check(sub, p.launch, p.outs, mode, decoy=lambda: d.launch(d.scratch_outs), scratch=[p.ws],
                                         control=functools.partial(control, mode) if n != 1 else None, runs=runs)   # n = 1 IS it
            if truth:
                check_decode_truth(c, p, res[n, Sq, modes[0]]["plain"])
        return res
    finally:
        vck.splits(0)


ALL_CASES = {c["id"]: (run, c) for run, cases in ((run_family_case, FAMILY_CASES), (run_variant_case, VARIANT_CASES),
                                                   (run_decode_case, DECODE_CASES)) for c in cases}
ALL_CASES.update({"headline-" + c["id"]: (run_family_case, c) for c in HEADLINE_CASES})


def summarise(lines):
    """The lines record() wrote during a full run, folded for profiles/race_cases.jsonl (4000 lines that all say "nothing
    changed" are no reading): one line per (table, kernel stems, mode) with the number of checks (a case, or one (splits,
    S_q) pair of a decode case), the runs of each, their seconds in all and the slowest one, and -- by check id -- every
    list of changed runs and every control result there was: both empty after a clean run."""
    tables = {run_family_case: "families", run_variant_case: "variants", run_decode_case: "decode"}
    groups = {}
    for r in map(json.loads, lines):
        table = tables[ALL_CASES[r["id"].split("/")[0]][0]] if r["id"].split("/")[0] in ALL_CASES else "headline"
        g = groups.setdefault((table, tuple(r["stems"]), r["mode"]), dict(
            table=table, stems=r["stems"], mode=r["mode"], checks=0, runs=r["runs"], seconds=0.0, slowest=["", 0.0], changed={}, control={}))
        assert g["runs"] == r["runs"], r
        g["checks"] += 1
        g["seconds"] = round(g["seconds"] + r["seconds"], 3)
        g["slowest"] = max(g["slowest"], [r["id"], r["seconds"]], key=lambda x: x[1])
        if r["changed"]:
            g["changed"][r["id"]] = r["changed"]
        if r["control"] is not None:
            g["control"][r["id"]] = r["control"]
    return [json.dumps(g) for g in groups.values()]
