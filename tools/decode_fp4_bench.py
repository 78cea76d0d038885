#!/usr/bin/env python3
"""Decoding attention over an MXFP4 KV cache (fp4_kvcache.flash_attention_kvcache_fp4) against
flash_attention_kvcache_fp8 on an e4m3 cache and flash_attention_kvcache on a bf16 cache of the same shape, in ONE process,
the three calls alternating round by round.  Timed with HIP events over --iters back-to-back calls after warm-up, best of
--rounds; the spread of each call's own rounds ((max - min) / min) is reported, and `faster_than_fp8` says whether the fp4
step beats the fp8 step by more than the larger of their two spreads.  There is no pass mark.

Points: B8 H32 H_kv 8 S_q 1 L16384 at D 128 and 64, bf16, padded, and the same over 128-key pages under a permuted table
(the fp8 and bf16 steps paged as well).  Per point: the three times, the fp4 / fp8 and fp4 / bf16 ratios (from bytes alone
the first is (D / 2 + D / 32) / D = 0.53), the split count, the fp4 call's algorithmic bytes (elements AND scales of the
visible rows + Q + O), bytes/s and its share of the 6.3 TB/s a copy reaches, and the relative difference of the fp4 output
from the bf16-cache output (quantisation error: the bf16 cache holds the unquantised data).  One JSON line per point.

--sweep instead times forced split counts (fa_debug_kvcache_splits) of the padded fp4 call: the data behind its split rule.

usage: tools/decode_fp4_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl] [--sweep]"""
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
import fp4_kvcache as F4  # noqa: E402
import paged_kvcache as PG  # noqa: E402
from decode_bench import COPY_BW, set_splits, time_ms  # noqa: E402

PAGE = 128
# (B, H, H_kv, S_q, D, L, paged)
POINTS = [(8, 32, 8, 1, D, 16384, paged) for paged in (False, True) for D in (128, 64)]
SWEEP = [(1, 32, 8, 1, 128, 4096), (1, 32, 8, 1, 128, 32768), (8, 32, 8, 1, 128, 4096), (8, 32, 8, 1, 128, 16384),
         (8, 32, 8, 1, 64, 16384), (32, 32, 8, 1, 128, 4096)]


def splits_of(B, H, Hkv, Sq, Sc, D):
    ws = fa.lib.fa_fwd_kvcache_fp4_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D)
    return max(1, ws // (B * H * Sq * (D + 2) * 4))


def setup(B, H, Hkv, Sq, D, L, others=True):
    g = torch.Generator(device="cuda").manual_seed(L + D + Hkv + Sq)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16, generator=g)
    q, kc, vc = mk(B, H, Sq, D), mk(B, Hkv, L, D), mk(B, Hkv, L, D)
    k4, ks = F4.quantize_kv_mxfp4(kc)
    v4, vs = F4.quantize_kv_mxfp4(vc)
    k8 = v8 = kd = vd = None
    if others:
        k8, kd = M.quantize_kv_fp8(kc)
        v8, vd = M.quantize_kv_fp8(vc)
    else:
        kc = vc = None
    return q, (kc, vc), (k8, v8, kd, vd), (k4, v4, ks, vs), torch.full((B,), L, dtype=torch.int32, device="cuda")


def to_pages(t, perm):
    """[B, H_kv, L, w] -> the pool [B * L / PAGE, H_kv, PAGE, w] with sequence b's page i at perm[b * L / PAGE + i]"""
    B, Hkv, L, w = t.shape
    pool = t.view(B, Hkv, L // PAGE, PAGE, w).permute(0, 2, 1, 3, 4).reshape(B * (L // PAGE), Hkv, PAGE, w)
    return torch.empty_like(pool).index_copy_(0, perm, pool)


def bench_point(B, H, Hkv, Sq, D, L, paged, a):
    q, (kc, vc), (k8, v8, kd, vd), (k4, v4, ks, vs), sl = setup(B, H, Hkv, Sq, D, L)
    if paged:
        n = B * (L // PAGE)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
        table = perm.view(B, L // PAGE).to(torch.int32)
        kc, vc, k4, v4, ks, vs = (to_pages(t, perm) for t in (kc, vc, k4, v4, ks, vs))
        k8, v8 = (to_pages(t.view(torch.uint8), perm).view(torch.float8_e4m3fn) for t in (k8, v8))
        f16 = lambda: PG.flash_attention_kvcache_paged(q, kc, vc, sl, table)
        f8 = lambda: PG.flash_attention_kvcache_paged(q, k8, v8, sl, table, k_descale=kd, v_descale=vd)
        f4 = lambda: F4.flash_attention_kvcache_fp4_paged(q, k4, v4, ks, vs, sl, table)
    else:
        f16 = lambda: M.flash_attention_kvcache(q, kc, vc, sl)
        f8 = lambda: M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd)
        f4 = lambda: F4.flash_attention_kvcache_fp4(q, k4, v4, ks, vs, sl)
    rows, qo = B * L, 2 * B * H * Sq * D * 2
    nbytes = rows * Hkv * 2 * (D // 2 + D // 32) + qo
    nbytes8 = rows * Hkv * 2 * D + qo
    line = {"B": B, "H": H, "H_kv": Hkv, "S_q": Sq, "D": D, "dtype": "bf16", "kv_dtype": "mxfp4", "L": L,
            "page_size": PAGE if paged else 0, "splits": splits_of(B, H, Hkv, Sq, L, D)}
    o4, o8, o16 = f4(), f8(), f16()
    line["rel_diff_vs_bf16_cache"] = round(float((o4.float() - o16.float()).norm() / o16.float().norm()), 5)
    line["fp8_rel_diff_vs_bf16_cache"] = round(float((o8.float() - o16.float()).norm() / o16.float().norm()), 5)
    line["finite"] = bool(torch.isfinite(o4).all())
    for _ in range(a.warmup):
        f16()
        f8()
        f4()
    t16, t8, t4 = [], [], []
    for _ in range(a.rounds):
        t16.append(time_ms(f16, a.iters))
        t8.append(time_ms(f8, a.iters))
        t4.append(time_ms(f4, a.iters))
    ms4, ms8, ms16 = min(t4), min(t8), min(t16)
    sp = lambda t: (max(t) - min(t)) / min(t)
    spread = max(sp(t4), sp(t8))
    bw = nbytes / (ms4 * 1e-3)
    line.update({"fp4_ms": round(ms4, 4), "fp8_ms": round(ms8, 4), "bf16_ms": round(ms16, 4),
                 "ratio_to_fp8": round(ms4 / ms8, 4), "ratio_to_bf16": round(ms4 / ms16, 4),
                 "spread": round(spread, 4), "spread_bf16": round(sp(t16), 4), "faster_than_fp8": bool(ms4 * (1 + spread) < ms8),
                 "bytes": nbytes, "bytes_ratio_to_fp8": round(nbytes / nbytes8, 4),
                 "TBps": round(bw / 1e12, 3), "share_of_copy_6p3": round(bw / COPY_BW, 3),
                 "fp8_TBps": round(nbytes8 / (ms8 * 1e-3) / 1e12, 3), "iters": a.iters, "rounds": a.rounds,
                 "device": torch.cuda.get_device_name(0)})
    return line


def sweep(a):
    out = []
    for B, H, Hkv, Sq, D, L in SWEEP:
        q, _, _, (k4, v4, ks, vs), sl = setup(B, H, Hkv, Sq, D, L, others=False)
        res = {"B": B, "H": H, "H_kv": Hkv, "S_q": Sq, "D": D, "L": L, "kv_dtype": "mxfp4", "formula": splits_of(B, H, Hkv, Sq, L, D)}
        for n in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64):
            if n > 1 and L // n < 64:
                continue
            set_splits(n)
            f4 = lambda: F4.flash_attention_kvcache_fp4(q, k4, v4, ks, vs, sl)
            for _ in range(a.warmup):
                f4()
            res["ms_n%d" % n] = round(min(time_ms(f4, a.iters) for _ in range(a.rounds)), 4)
        set_splits(0)
        print(json.dumps(res), flush=True)
        out.append(res)
        del q, k4, v4, ks, vs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true", help="forced split counts instead of the points")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no fallback"
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
