#!/usr/bin/env python3
"""The indexer logits kernel (mla_indexer.mla_indexer_logits_fp8) against what a user does without it, in ONE process, the two
calls alternating round by round: the PyTorch construction -- gather the pages through the table, dequantise to bf16, einsum,
relu, weighted sum over the heads, times the key scales.

Timed with HIP events over --iters back-to-back calls after a warm-up of both, best of --rounds; the spread of each call's own
rounds ((max - min) / min) is reported, with TB/s of the 132 bytes per cached key and its share of the 6.3 TB/s copy rate the
README uses.  There is no pass mark beyond beating the construction by more than the spread.

Settings: B 8, H_i 64, L 32768, 64-key pages under a permuted table, S_q 1 and 2.  One JSON line per point.

usage: tools/mla_indexer_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl]"""
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

B, HI, L, PAGE, COPY_TBPS = 8, 64, 32768, 64, 6.3
F8 = torch.float8_e4m3fn


def setup(Sq):
    g = torch.Generator(device="cuda").manual_seed(Sq)
    mp = L // PAGE
    q = torch.randn(B, Sq, HI, 128, device="cuda", generator=g).to(F8)
    w = torch.randn(B, Sq, HI, device="cuda", generator=g) * HI ** -0.5
    pool = torch.randn(B * mp, PAGE, 128, device="cuda", generator=g).to(F8)
    scale = torch.rand(B * mp, PAGE, device="cuda", generator=g) + 0.5
    table = torch.randperm(B * mp, device="cuda", generator=g).to(torch.int32).view(B, mp)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    return q, w, pool, scale, sl, table


def construction(q, w, pool, scale, sl, table):
    """the logits in PyTorch (every sequence holds L keys here, so no column is hidden)"""
    k = pool.view(torch.uint8)[table.long()].view(B, L, 128).view(F8).to(torch.bfloat16)
    s = scale[table.long()].view(B, L)
    score = torch.einsum("bihd,btd->biht", q.to(torch.bfloat16), k).float().relu_()
    return (score * w[..., None]).sum(2) * s[:, None]


def bench_point(Sq, a):
    args = setup(Sq)
    fns = (lambda: IDX.mla_indexer_logits_fp8(*args), lambda: construction(*args))
    o, ref = fns[0](), fns[1]()
    line = {"B": B, "H_i": HI, "S_q": Sq, "L": L, "page_size": PAGE, "finite": bool(torch.isfinite(o).all()),
            "rel_diff_vs_torch_bf16": round(float((o - ref).norm() / ref.norm()), 6)}
    for _ in range(a.warmup):
        for f in fns:
            f()
    t = [[], []]
    for _ in range(a.rounds):
        for k, f in enumerate(fns):
            t[k].append(time_ms(f, a.iters))
    ms, ms_t = min(t[0]), min(t[1])
    sp = lambda x: round((max(x) - min(x)) / min(x), 4)
    tbps = B * L * 132 / (ms * 1e-3) / 1e12
    line.update({"kernel_ms": round(ms, 4), "torch_ms": round(ms_t, 4), "speedup": round(ms_t / ms, 2), "spread": sp(t[0]),
                 "spread_torch": sp(t[1]), "TBps_132B_per_key": round(tbps, 3), "share_of_copy_rate": round(tbps / COPY_TBPS, 3),
                 "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)})
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no fallback"
    lines = []
    for Sq in (1, 2):
        lines.append(bench_point(Sq, a))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x["finite"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
