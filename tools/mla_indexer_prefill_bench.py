#!/usr/bin/env python3
"""The prefill indexer logits kernel (mla_indexer.mla_indexer_logits_fp8_prefill) against the two things a user has without it,
in ONE process, the three calls alternating round by round:

  (a) today's path: mla_indexer_logits_fp8 on the same keys laid into a paged pool (64-key pages), per sequence B = 1, S_q = the
      sequence's rows, is_causal=True -- one call per sequence at the packed point;
  (b) the PyTorch construction: dequantise to bf16, einsum, relu, weighted sum over the heads, times the key scales, mask.

Timed with HIP events over back-to-back calls (a window of about 0.1 s, at least --iters calls) after a warm-up of all three,
best of --rounds; the spread of each call's own rounds ((max - min) / min) is reported, with the FP8 TFLOP/s over the VISIBLE products (2 * 128 * H_i per visible logit) and
the rate at which the [M, N] fp32 result is written.  "faster than (a)" holds only where the gap exceeds the larger spread.

Points, H_i 64: one causal prompt M = N = 4096; a chunk M = 2048 behind 14336 cached keys (N = 16384); eight packed sequences of
512 (M = N = 4096).  One JSON line per point.

usage: tools/mla_indexer_prefill_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl]"""
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

HI, PAGE = 64, 64
F8 = torch.float8_e4m3fn
# name: (rows, keys) of every sequence; a sequence's rows are its last keys (causal, bottom-right aligned)
POINTS = {"causal-prompt": [(4096, 4096)], "chunk-with-context": [(2048, 16384)], "packed-8x512": [(512, 512)] * 8}


def setup(seqs):
    g = torch.Generator(device="cuda").manual_seed(len(seqs))
    M, N = sum(m for m, _ in seqs), sum(n for _, n in seqs)
    q = torch.randn(M, HI, 128, device="cuda", generator=g).to(F8)
    w = torch.randn(M, HI, device="cuda", generator=g) * HI ** -0.5
    k = torch.randn(N, 128, device="cuda", generator=g).to(F8)
    s = torch.rand(N, device="cuda", generator=g) + 0.5
    ks, ke, m0, n0 = [], [], 0, 0
    for m, n in seqs:
        ks += [n0] * m
        ke += [n0 + n - m + i + 1 for i in range(m)]
        m0, n0 = m0 + m, n0 + n
    dev = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")
    return q, w, k, s, dev(ks), dev(ke)


def paged_path(seqs, q, w, k, s):
    """(a): the call per sequence over its keys as pages of one pool; returns the closure and its per-sequence results"""
    calls, m0, n0 = [], 0, 0
    for m, n in seqs:
        assert n % PAGE == 0
        args = (q[m0:m0 + m].unsqueeze(0), w[m0:m0 + m].unsqueeze(0), k[n0:n0 + n].view(n // PAGE, PAGE, 128),
                s[n0:n0 + n].view(n // PAGE, PAGE), torch.tensor([n], dtype=torch.int32, device="cuda"),
                torch.arange(n // PAGE, dtype=torch.int32, device="cuda").view(1, -1))
        calls.append(args)
        m0, n0 = m0 + m, n0 + n
    return lambda: [IDX.mla_indexer_logits_fp8(*a, is_causal=True) for a in calls]


def construction(q, w, k, s, ks, ke):
    score = torch.einsum("mhd,td->mht", q.to(torch.bfloat16), k.to(torch.bfloat16)).relu_()
    out = torch.einsum("mht,mh->mt", score, w.to(torch.bfloat16)).float() * s
    t = torch.arange(k.shape[0], device="cuda")
    return out.masked_fill_((t < ks[:, None]) | (t >= ke[:, None]), float("-inf"))


def bench_point(name, a):
    seqs = POINTS[name]
    args = setup(seqs)
    q, w, k, s, ks, ke = args
    M, N = q.shape[0], k.shape[0]
    fns = (lambda: IDX.mla_indexer_logits_fp8_prefill(*args), paged_path(seqs, q, w, k, s), lambda: construction(*args))
    o, pa, ref = fns[0](), fns[1](), fns[2]()
    vis = torch.isfinite(ref)
    m0 = n0 = 0
    same = True
    for (m, n), x in zip(seqs, pa):          # (a) computes the same sums in the same order
        same = same and torch.equal(o[m0:m0 + m, n0:n0 + n], x[0])
        m0, n0 = m0 + m, n0 + n
    line = {"point": name, "M": M, "N": N, "H_i": HI, "sequences": len(seqs), "visible": int(vis.sum()),
            "hidden_is_neg_inf": bool((o[~vis] == float("-inf")).all()) and bool(torch.isfinite(o[vis]).all()),
            "same_bits_as_paged_path": bool(same),
            "rel_diff_vs_torch_bf16": round(float((o[vis] - ref[vis]).norm() / ref[vis].norm()), 6)}
    del o, pa, ref
    for _ in range(a.warmup):
        for f in fns:
            f()
    # a timed window of about 0.1 s per call: --iters is the least number of calls in it
    iters = [max(a.iters, min(2000, int(100.0 / time_ms(f, 3)))) for f in fns]
    t = [[], [], []]
    for _ in range(a.rounds):
        for j, f in enumerate(fns):
            t[j].append(time_ms(f, iters[j]))
    ms, ms_a, ms_b = (min(x) for x in t)
    sp = lambda x: round((max(x) - min(x)) / min(x), 4)
    line.update({"kernel_ms": round(ms, 4), "paged_path_ms": round(ms_a, 4), "torch_ms": round(ms_b, 4),
                 "speedup_vs_paged_path": round(ms_a / ms, 2), "speedup_vs_torch": round(ms_b / ms, 2),
                 "spread": sp(t[0]), "spread_paged_path": sp(t[1]), "spread_torch": sp(t[2]),
                 "faster_than_paged_path_beyond_spread": bool(ms_a / ms - 1 > max(sp(t[0]), sp(t[1]))),
                 "fp8_tflops_visible": round(line["visible"] * 2 * 128 * HI / (ms * 1e-3) / 1e12, 1),
                 "output_write_TBps": round(M * N * 4 / (ms * 1e-3) / 1e12, 3),
                 "iters": iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)})
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no fallback"
    lines = []
    for name in POINTS:
        lines.append(bench_point(name, a))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x["hidden_is_neg_inf"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
