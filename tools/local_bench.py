#!/usr/bin/env python3
"""Sliding-window (local) attention against causal attention, fwd+bwd, in ONE process: for each point the same inputs go
through flash_attention_local and through flash_attention(is_causal=True) (the table-picked kernels), timed with HIP
events, interleaved.  One JSON line per point: ms per fwd+bwd step, TFLOPS credited from the visible (query, key) pairs
(My_FlashAttention_optimized.local_attention_flops; causal = the (-1, 0) window), and local / causal.

usage: tools/local_bench.py [--iters N] [--warmup W] [--out file.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))

import torch  # noqa: E402

import My_FlashAttention_optimized as M  # noqa: E402

POINTS = [(4, 32, S, 64, w) for S in (4096, 16384) for w in ((255, 0), (1023, 0), (511, 511))]


def step_fn(q, k, v, do, window):
    if window is None:
        return lambda: M.flash_attention(q, k, v, is_causal=True).backward(do)
    return lambda: M.flash_attention_local(q, k, v, window[0], window[1]).backward(do)


def time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved local / causal rounds; the best of each is kept")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for B, H, S, D, w in POINTS:
        g = torch.Generator(device="cuda").manual_seed(S + w[0])
        mk = lambda: torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16, generator=g)
        q, k, v, do = (mk() for _ in range(4))
        q.requires_grad_(True)
        k.requires_grad_(True)
        v.requires_grad_(True)
        # the outputs of one local step must be finite (rows always see their own key under these windows)
        o = M.flash_attention_local(q, k, v, w[0], w[1])
        o.backward(do)
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(o).all() and torch.isfinite(q.grad).all() and torch.isfinite(k.grad).all()
                      and torch.isfinite(v.grad).all())
        fl, fc = step_fn(q, k, v, do, w), step_fn(q, k, v, do, None)
        for _ in range(a.warmup):
            fl()
            fc()
        ml, mc = [], []
        for _ in range(a.rounds):
            q.grad = k.grad = v.grad = None
            ml.append(time_ms(fl, a.iters))
            q.grad = k.grad = v.grad = None
            mc.append(time_ms(fc, a.iters))
        ms_l, ms_c = min(ml), min(mc)
        f_l = M.local_attention_flops(B, H, S, S, D, w[0], w[1], "fwd_bwd")
        f_c = M.local_attention_flops(B, H, S, S, D, -1, 0, "fwd_bwd")
        line = {"B": B, "H": H, "S": S, "D": D, "dtype": "bf16", "window": list(w), "local_ms": round(ms_l, 4),
                "causal_ms": round(ms_c, 4), "ratio": round(ms_l / ms_c, 4), "pairs_ratio": round(f_l / f_c, 4),
                "local_tflops": round(f_l / (ms_l * 1e-3) / 1e12, 1), "causal_tflops": round(f_c / (ms_c * 1e-3) / 1e12, 1),
                "finite": finite, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del q, k, v, do, o
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x["finite"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
