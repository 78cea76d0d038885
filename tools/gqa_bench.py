#!/usr/bin/env python3
"""Grouped-query attention against the expanded-K/V path, fwd+bwd, in ONE process: for each point the same inputs go
through (a) flash_attention_gqa and (b) what a GQA caller does without it -- K and V repeat_interleave'd to H heads,
flash_attention (the table-picked kernels; flash_attention_local for a windowed point), and autograd's sum of the
per-head dK / dV back into H_kv heads.  Timed with HIP events, interleaved, best of --rounds.  Per path also the peak
memory a step allocates above the resident inputs (torch.cuda.max_memory_allocated).  One JSON line per point; ratio =
gqa_ms / expanded_ms (below 1: GQA is faster).

usage: tools/gqa_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))

import torch  # noqa: E402

import My_FlashAttention_optimized as M  # noqa: E402

# (B, H, H_kv, S, D, window): bf16 causal at H_kv = 8 and 1 (multi-query), and one windowed point
POINTS = [(4, 32, hk, S, D, (-1, 0)) for S in (4096, 16384) for D in (64, 128) for hk in (8, 1)]
POINTS.append((4, 32, 8, 16384, 64, (1023, 0)))


def step_fn(q, k, v, do, window, gqa):
    g = q.shape[1] // k.shape[1]
    wl, wr = window
    if gqa:
        return lambda: M.flash_attention_gqa(q, k, v, window_size=window).backward(do)

    def expanded():
        ke, ve = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
        o = M.flash_attention(q, ke, ve, is_causal=True) if (wl, wr) == (-1, 0) else M.flash_attention_local(q, ke, ve, wl, wr)
        o.backward(do)
    return expanded


def time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def peak_extra_bytes(fn, leaves):
    """Peak allocation of one step above what is resident before it (gradients cleared)."""
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved gqa / expanded rounds; the best of each is kept")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for B, H, Hkv, S, D, w in POINTS:
        g = torch.Generator(device="cuda").manual_seed(S + D + Hkv)
        mk = lambda h: torch.randn(B, h, S, D, device="cuda", dtype=torch.bfloat16, generator=g)
        q, k, v, do = mk(H), mk(Hkv), mk(Hkv), mk(H)
        for t in (q, k, v):
            t.requires_grad_(True)
        fa, fb = step_fn(q, k, v, do, w, True), step_fn(q, k, v, do, w, False)
        # one step of each: finite, and the two paths agree to bf16 accuracy
        fa()
        ga = [t.grad.clone() for t in (q, k, v)]
        for t in (q, k, v):
            t.grad = None
        fb()
        gb = [t.grad for t in (q, k, v)]
        finite = all(bool(torch.isfinite(x).all()) for x in ga + gb)
        rel = max(float((x.float() - y.float()).norm() / y.float().norm()) for x, y in zip(ga, gb))
        del ga, gb
        mem_a, mem_b = peak_extra_bytes(fa, (q, k, v)), peak_extra_bytes(fb, (q, k, v))
        for _ in range(a.warmup):
            fa()
            fb()
        ta, tb = [], []
        for _ in range(a.rounds):
            q.grad = k.grad = v.grad = None
            ta.append(time_ms(fa, a.iters))
            q.grad = k.grad = v.grad = None
            tb.append(time_ms(fb, a.iters))
        ms_a, ms_b = min(ta), min(tb)
        fl = M.local_attention_flops(B, H, S, S, D, w[0], w[1], "fwd_bwd")
        line = {"B": B, "H": H, "H_kv": Hkv, "S": S, "D": D, "dtype": "bf16", "window": list(w),
                "gqa_ms": round(ms_a, 4), "expanded_ms": round(ms_b, 4), "ratio": round(ms_a / ms_b, 4),
                "gqa_tflops": round(fl / (ms_a * 1e-3) / 1e12, 1), "expanded_tflops": round(fl / (ms_b * 1e-3) / 1e12, 1),
                "gqa_peak_extra_MiB": round(mem_a / 2**20, 1), "expanded_peak_extra_MiB": round(mem_b / 2**20, 1),
                "grad_rel_diff": round(rel, 5), "finite": finite, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del q, k, v, do
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x["finite"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
