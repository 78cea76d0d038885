#!/usr/bin/env python3
"""The top-k selection kernel (mla_indexer.mla_indexer_select) against the path it replaces, mla_indexer.mla_indexer_topk
(torch.topk, a where, a cast and a pad), on the same logits in ONE process, the two calls alternating round by round.

Timed with HIP events over --iters back-to-back calls after a warm-up of both, best of --rounds; the spread of each call's own
rounds ((max - min) / min) is reported.  The pass mark: the kernel beats the torch path by more than the larger of the two
spreads ("beats_torch").  Each time is also set against two references: one read of the rows' live part at the 6.3 TB/s copy rate
the README uses ("row_read_ms"), and the logits call's 0.0119 ms at B8, L 32768 (profiles/mla_indexer_bench_lines.jsonl).

Points: B 8, S_q 1, topk 2048, normal logits; W 32768 (resident), W 131072 (streaming), and W 131072 with lengths 32768 -- what
the bound on the scan saves (the torch path has no such bound and scans all W).  The kernel writes into a given `out`.  One JSON
line per point.

usage: tools/mla_select_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import mla_indexer as IDX  # noqa: E402
from decode_bench import time_ms  # noqa: E402

B, SQ, TOPK, COPY_TBPS, LOGITS_MS = 8, 1, 2048, 6.3, 0.0119
POINTS = [(32768, None), (131072, None), (131072, 32768)]


def bench_point(W, length, a):
    g = torch.Generator(device="cuda").manual_seed(W)
    logits = torch.randn(B, SQ, W, device="cuda", generator=g)
    lengths = None if length is None else torch.full((B,), length, dtype=torch.int32, device="cuda")
    out = torch.empty(B, SQ, TOPK, dtype=torch.int32, device="cuda")
    fns = (lambda: IDX.mla_indexer_select(logits, TOPK, lengths=lengths, out=out), lambda: IDX.mla_indexer_topk(logits, TOPK))
    live = W if length is None else length
    same = torch.equal(fns[0](), IDX.mla_indexer_topk(logits[..., :live], TOPK).sort(-1).values)
    for _ in range(a.warmup):
        for f in fns:
            f()
    t = [[], []]
    for _ in range(a.rounds):
        for k, f in enumerate(fns):
            t[k].append(time_ms(f, a.iters))
    ms, ms_t = min(t[0]), min(t[1])
    sp = lambda x: round((max(x) - min(x)) / min(x), 4)
    read_ms = B * SQ * live * 4 / (COPY_TBPS * 1e12) * 1e3
    return {"B": B, "S_q": SQ, "W": W, "lengths": length, "topk": TOPK, "instance": "resident" if W <= 32768 else "streaming",
            "same_set_as_torch": bool(same), "kernel_ms": round(ms, 4), "torch_ms": round(ms_t, 4), "speedup": round(ms_t / ms, 2),
            "spread": sp(t[0]), "spread_torch": sp(t[1]), "beats_torch": bool(ms_t / ms - 1 > max(sp(t[0]), sp(t[1]))),
            "row_read_ms": round(read_ms, 5), "times_row_read": round(ms / read_ms, 1), "times_logits_call": round(ms / LOGITS_MS, 2),
            "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no fallback"
    lines = []
    for W, length in POINTS:
        lines.append(bench_point(W, length, a))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x["same_set_as_torch"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
