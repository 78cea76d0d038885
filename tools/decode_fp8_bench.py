#!/usr/bin/env python3
"""Decoding attention over an FP8 (e4m3) KV cache (flash_attention_kvcache_fp8) against flash_attention_kvcache on a
bf16 cache of the same shape, in ONE process: the points of tools/decode_bench.py with L >= 4096, the two calls
alternating round by round.  Timed with HIP events over --iters back-to-back calls after warm-up, best of --rounds; the
spread of each call's own rounds ((max - min) / min) is reported, and `faster` says whether the fp8 step beats the bf16
step by more than the larger of the two spreads.

Per point: both times and their ratio (fp8 / bf16; the bound from bytes is 0.5 plus the unchanged Q / O / partial
traffic), the split count, the fp8 call's algorithmic bytes (the K/V rows some query can see at 1 byte per element + Q + O)
and bytes/s as a share of the 6.3 TB/s a copy reaches, and the relative difference of the two outputs (quantisation error:
the bf16 cache holds the unquantised data).  One JSON line per point.

--sweep instead times forced split counts (fa_debug_kvcache_splits) of the fp8 call: the data behind its split rule.

usage: tools/decode_fp8_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl] [--sweep]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import _mi355fa as fa  # noqa: E402
import My_FlashAttention_optimized as M  # noqa: E402
from decode_bench import COPY_BW, POINTS as ALL_POINTS, SWEEP as ALL_SWEEP, set_splits, time_ms, visible_rows  # noqa: E402

POINTS = [p for p in ALL_POINTS if (p[5] if isinstance(p[5], int) else max(p[5])) >= 4096]
# (two more D = 64 points: the fp8 rule allows D = 64 twice the workgroups)
SWEEP = [p for p in ALL_SWEEP if p[5] >= 4096] + [(32, 32, 8, 1, 64, 4096), (1, 32, 8, 1, 64, 32768)]


def splits_of(B, H, Hkv, Sq, Sc, D):
    ws = fa.lib.fa_fwd_kvcache_fp8_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D)
    return max(1, ws // (B * H * Sq * (D + 2) * 4))


def setup(B, H, Hkv, Sq, D, lens, bf16_too=True):
    Sc = max(lens)
    g = torch.Generator(device="cuda").manual_seed(Sc + D + Hkv + Sq)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16, generator=g)
    q, kc, vc = mk(B, H, Sq, D), mk(B, Hkv, Sc, D), mk(B, Hkv, Sc, D)
    k8, kd = M.quantize_kv_fp8(kc)
    v8, vd = M.quantize_kv_fp8(vc)
    if not bf16_too:
        kc = vc = None
    return q, kc, vc, k8, v8, kd, vd, torch.tensor(lens, dtype=torch.int32, device="cuda")


def bench_point(B, H, Hkv, Sq, D, lens, causal, window, a):
    uniform = isinstance(lens, int)
    lens = [lens] * B if uniform else list(lens)
    q, kc, vc, k8, v8, kd, vd, sl = setup(B, H, Hkv, Sq, D, lens)
    wl, wr = (window[0], 0) if causal else window
    f16 = lambda: M.flash_attention_kvcache(q, kc, vc, sl, is_causal=causal, window_size=window)
    f8 = lambda: M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd, is_causal=causal, window_size=window)
    rows = sum(visible_rows(L, Sq, wl, wr)[0] for L in lens)
    qo = 2 * B * H * Sq * D * 2
    nbytes = rows * Hkv * 2 * D * 1 + qo
    line = {"B": B, "H": H, "H_kv": Hkv, "S_q": Sq, "D": D, "dtype": "bf16", "kv_dtype": "e4m3",
            "L": lens[0] if uniform else lens, "causal": causal, "window": list(window),
            "splits": splits_of(B, H, Hkv, Sq, max(lens), D)}
    o8, o16 = f8(), f16()
    line["rel_diff_vs_bf16_cache"] = round(float((o8.float() - o16.float()).norm() / o16.float().norm()), 5)
    line["finite"] = bool(torch.isfinite(o8).all())
    for _ in range(a.warmup):
        f16()
        f8()
    t16, t8 = [], []
    for _ in range(a.rounds):
        t16.append(time_ms(f16, a.iters))
        t8.append(time_ms(f8, a.iters))
    ms8, ms16 = min(t8), min(t16)
    spread = max((max(t8) - ms8) / ms8, (max(t16) - ms16) / ms16)
    bw = nbytes / (ms8 * 1e-3)
    line.update({"fp8_ms": round(ms8, 4), "bf16_ms": round(ms16, 4), "ratio": round(ms8 / ms16, 4),
                 "spread": round(spread, 4), "faster": bool(ms8 * (1 + spread) < ms16),
                 "bytes": nbytes, "bytes_ratio": round(nbytes / (rows * Hkv * 2 * D * 2 + qo), 4),
                 "TBps": round(bw / 1e12, 3), "share_of_copy_6p3": round(bw / COPY_BW, 3),
                 "device": torch.cuda.get_device_name(0)})
    return line


def sweep(a):
    out = []
    for B, H, Hkv, Sq, D, L in SWEEP:
        q, _, _, k8, v8, kd, vd, sl = setup(B, H, Hkv, Sq, D, [L] * B, bf16_too=False)
        res = {"B": B, "H": H, "H_kv": Hkv, "S_q": Sq, "D": D, "L": L, "kv_dtype": "e4m3",
               "formula": splits_of(B, H, Hkv, Sq, L, D)}
        for n in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 128):
            if n > 1 and L // n < 64:
                continue
            set_splits(n)
            f8 = lambda: M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd)
            for _ in range(a.warmup):
                f8()
            res["ms_n%d" % n] = round(min(time_ms(f8, a.iters) for _ in range(a.rounds)), 4)
        set_splits(0)
        print(json.dumps(res), flush=True)
        out.append(res)
        del q, k8, v8
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true", help="forced split counts instead of the points")
    a = ap.parse_args()
    if a.sweep:
        lines = sweep(a)
    else:
        lines = []
        for pt in POINTS:
            line = bench_point(*pt, a)
            print(json.dumps(line), flush=True)
            lines.append(line)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x.get("finite", True) for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
