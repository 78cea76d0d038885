#!/usr/bin/env python3
"""Packed MLA decoding (mla_ragged_kvcache.flash_attention_mla_kvcache_ragged) against the rectangular call
(mla_kvcache.flash_attention_mla_kvcache) on the same pool, in ONE process, the calls alternating round by round.  Timed with
HIP events over --iters back-to-back calls after a warm-up of all, best of --rounds; spread = the larger (max - min) / min of
the two calls' rounds.  There is no pass mark: nobody had measured this step, and each point is written down whichever way it falls.

Settings: bf16, 64-key pages under a permuted table.  Points:
  pure_decode_h128 / _h16   B 8, one query per sequence, L 16384, against the rectangular call at S_q = 1.  plan_ms is the plan
                kernel alone (fa_debug_ragged_plan with group = H, HIP events); `within` says whether packed <= rectangular +
                plan + spread * rectangular.
  mtp_verify    B 32, H 16, S_b = 1 .. 4 (b % 4 + 1), L 4096, causal, against the rectangular call on q left-padded to S_q = 4.
  mixed_step    one 256-row chunk over L 4096 plus 31 decode rows over L 4096, H 16, causal, against the two rectangular calls
                that cover it (B 1 S_q 256 and B 31 S_q 1), timed together.
  --sweep       forced split counts (fa_debug_kvcache_splits) at the four points: the rule's count (mla_splits over nb_max), the
                best forced count and how far the rule is off it.

One JSON line per point.  usage: tools/mla_ragged_bench.py [--iters N] [--warmup W] [--rounds R] [--sweep] [--out file.jsonl]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import _mi355fa as fa  # noqa: E402
import mla_kvcache as MLA  # noqa: E402
import mla_ragged_kvcache as MLAR  # noqa: E402
from decode_bench import set_splits, time_ms  # noqa: E402

PAGE = 64
D, DV = 576, 512
SWEEP = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)
BF = torch.bfloat16
#         name: (H, [S_b], [L_b])
POINTS = {
    "pure_decode_h128": (128, [1] * 8, [16384] * 8),
    "pure_decode_h16": (16, [1] * 8, [16384] * 8),
    "mtp_verify": (16, [b % 4 + 1 for b in range(32)], [4096] * 32),
    "mixed_step": (16, [256] + [1] * 31, [4096] * 32),
}


def nb_max(H, T, B):
    return (H * T + 31 * B) // 32


def plan_bytes(H, T, B):
    return (16 + 8 * nb_max(H, T, B) + 15) // 16 * 16


def packed_splits(H, T, B, mp):
    ws = fa.lib.fa_fwd_kvcache_mla_ragged_workspace_bytes(T, B, H, mp, PAGE) - plan_bytes(H, T, B)
    return max(1, ws // (H * T * (DV + 2) * 4))


def rect_splits(B, H, Sq, mp):
    ws = fa.lib.fa_fwd_kvcache_mla_workspace_bytes(B, H, Sq, mp, PAGE, 0)
    return max(1, ws // (B * H * Sq * (DV + 2) * 4))


def setup(H, S, lens):
    B, T, L = len(S), sum(S), max(lens)
    g = torch.Generator(device="cuda").manual_seed(L + H + T)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=BF, generator=g)
    q, kv = mk(T, H, D), mk(B, L, D)
    n = B * (L // PAGE)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
    pool = torch.empty(n, PAGE, D, device="cuda", dtype=BF).index_copy_(0, perm, kv.view(n, PAGE, D))
    table = perm.view(B, L // PAGE).to(torch.int32)
    cu = torch.tensor([sum(S[:b]) for b in range(B + 1)], dtype=torch.int32, device="cuda")
    return q, pool, table, cu, torch.tensor(lens, dtype=torch.int32, device="cuda")


def rect_calls(name, q, pool, table, sl, S, causal):
    """the rectangular launches that cover the step, as one function, their split counts, and their result in packed order
    (None where the comparison pads)"""
    H, B, mp = q.shape[1], len(S), table.shape[1]
    if name == "mixed_step":
        qa, qb = q[:S[0]].transpose(0, 1)[None], q[S[0]:, None].transpose(1, 2)          # [1, H, 256, D], [31, H, 1, D]
        fa_ = lambda: MLA.flash_attention_mla_kvcache(qa, pool, sl[:1], table[:1], is_causal=True)
        fb_ = lambda: MLA.flash_attention_mla_kvcache(qb, pool, sl[1:], table[1:], is_causal=True)

        def both():
            return fa_(), fb_()
        packed = lambda: torch.cat([fa_()[0].transpose(0, 1), fb_()[:, :, 0]], 0)
        return both, [rect_splits(1, H, S[0], mp), rect_splits(B - 1, H, 1, mp)], packed
    Sq = max(S)
    qr = torch.zeros(B, H, Sq, D, device="cuda", dtype=BF)                               # left-padded: the last S_b rows are b's
    at = 0
    for b, s in enumerate(S):
        qr[b, :, Sq - s:] = q[at:at + s].transpose(0, 1)
        at += s
    f = lambda: MLA.flash_attention_mla_kvcache(qr, pool, sl, table, is_causal=causal)
    packed = lambda: torch.cat([f()[b, :, Sq - s:].transpose(0, 1) for b, s in enumerate(S)], 0)
    return f, [rect_splits(B, H, Sq, mp)], packed


def rounds_of(fns, a):
    """[[ms per round] per function], the functions interleaved round by round after the warm-up of all"""
    for _ in range(a.warmup):
        for f in fns:
            f()
    out = [[] for _ in fns]
    for _ in range(a.rounds):
        for i, f in enumerate(fns):
            out[i].append(time_ms(f, a.iters))
    return out


def plan_ms(cu, T, B, H, a):
    ws = torch.empty(plan_bytes(H, T, B), dtype=torch.uint8, device="cuda")
    fn = fa.lib.fa_debug_ragged_plan
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p], ctypes.c_int
    s = torch.cuda.current_stream().cuda_stream
    f = lambda: fa.check(fn(cu.data_ptr(), ws.data_ptr(), T, B, H, 1, s), "fa_debug_ragged_plan")
    return min(rounds_of([f], a)[0])


def spread(t):
    return (max(t) - min(t)) / min(t)


def bench_point(name, a):
    H, S, lens = POINTS[name]
    causal = name != "pure_decode_h128" and name != "pure_decode_h16"
    q, pool, table, cu, sl = setup(H, S, lens)
    B, T, mp = len(S), sum(S), table.shape[1]
    ours = lambda: MLAR.flash_attention_mla_kvcache_ragged(q, pool, cu, sl, table, is_causal=causal)
    rect, rsplits, rect_packed = rect_calls(name, q, pool, table, sl, S, causal)
    o, ref = ours(), rect_packed()
    line = {"point": name, "B": B, "H": H, "total_q": T, "S_b_max": max(S), "L": max(lens), "dtype": "bf16", "page_size": PAGE,
            "causal": causal, "splits": packed_splits(H, T, B, mp), "rect_splits": rsplits, "nb_max": nb_max(H, T, B),
            "finite": bool(torch.isfinite(o).all()),
            "rel_diff_vs_rect": round(float((o.float() - ref.float()).norm() / ref.float().norm()), 6)}
    tp, tr = rounds_of([ours, rect], a)
    ms, ms_rect, sp = min(tp), min(tr), max(spread(tp), spread(tr))
    line.update({"packed_ms": round(ms, 4), "rect_ms": round(ms_rect, 4), "ratio_to_rect": round(ms / ms_rect, 4), "spread": round(sp, 4)})
    if not causal:
        pm = plan_ms(cu, T, B, H, a)
        line.update({"plan_ms": round(pm, 4), "over_rect_plus_plan_ms": round(ms - ms_rect - pm, 4),
                     "within": bool(ms <= ms_rect + pm + sp * ms_rect)})
    line.update({"TFLOPS": round(2 * H * sum(s * L for s, L in zip(S, lens)) * (D + DV) / (ms * 1e-3) / 1e12, 1),
                 "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)})
    return line


def sweep_point(name, a):
    H, S, lens = POINTS[name]
    causal = not name.startswith("pure_decode")
    q, pool, table, cu, sl = setup(H, S, lens)
    B, T, mp = len(S), sum(S), table.shape[1]
    ours = lambda: MLAR.flash_attention_mla_kvcache_ragged(q, pool, cu, sl, table, is_causal=causal)
    n0 = packed_splits(H, T, B, mp)
    res = {"point": name + "_sweep", "B": B, "H": H, "total_q": T, "L": max(lens), "dtype": "bf16", "page_size": PAGE, "nb_max": nb_max(H, T, B),
           "formula": n0}
    for n in sorted(set(SWEEP) | {n0}):
        set_splits(n)
        res["ms_n%d" % n] = round(min(rounds_of([ours], a)[0]), 4)
    set_splits(0)
    best = min((v, k) for k, v in res.items() if k.startswith("ms_n"))
    res["best"], res["formula_over_best"] = best[1], round(res["ms_n%d" % n0] / best[0] - 1, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true", help="forced split counts instead of the points")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no fallback"
    lines = []
    for name in POINTS:
        line = sweep_point(name, a) if a.sweep else bench_point(name, a)
        print(json.dumps(line), flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x.get("finite", True) for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
