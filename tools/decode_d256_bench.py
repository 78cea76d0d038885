#!/usr/bin/env python3
"""Decoding attention at head dim 256 (the decode calls' third head dim: csrc/fa_decode_body.inc, "D = 256") in ONE process,
timed with HIP events over --iters back-to-back calls after warm-up, interleaved, best of --rounds.  For each point:

  d256     the call at H 16, H_kv 8, D 256 (Gemma-2-9B-like heads)
  d128     the same call at H 32, H_kv 16, D 128: the same B and L, the same number of cache bytes.  Timed twice in the same
           run (d128_ms, d128_again_ms): the difference between the two is the run's own spread
  sdpa     what a caller has without the decode path: torch.nn.functional.scaled_dot_product_attention(enable_gqa=True) on
           the bf16 cache sliced to L (for an e4m3 point: on the dequantised bf16 cache; it has no soft cap, so the soft-capped
           point is compared with the uncapped SDPA)

Per point: the three times, the split count, the algorithmic bytes (K/V rows below L, q and o), bytes/s of d256 and of d128,
rate_vs_d128 = d256 bytes/s / d128 bytes/s (the better d128 time), spread_d128 = |d128 - d128_again| / their smaller, and
ratio_vs_sdpa = d256 time / sdpa time (below 1: the decode path is faster).  One JSON line per point.

--sweep instead times forced split counts (fa_debug_kvcache_splits) at three of the points, at more batch sizes and cache
lengths and on e4m3 caches: the data behind the split rule at D = 256 (csrc/fa_decode.hip kvcache_splits).

usage: tools/decode_d256_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl] [--sweep]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import My_FlashAttention_optimized as M  # noqa: E402
from decode_bench import set_splits, time_ms  # noqa: E402
from paged_kvcache import flash_attention_kvcache_paged  # noqa: E402
from ragged_kvcache import flash_attention_kvcache_ragged  # noqa: E402

import _mi355fa as fa  # noqa: E402

PAGE = 128
# (name, kind, B, L)
POINTS = [("padded", "padded", 8, 16384), ("fp8", "fp8", 8, 16384), ("paged", "paged", 8, 16384), ("packed", "ragged", 8, 16384),
          ("B1-L32768", "padded", 1, 32768), ("B32-L4096", "padded", 32, 4096), ("softcap", "softcap", 8, 16384)]
SWEEP = [("padded", "padded", 8, 16384), ("B1-L32768", "padded", 1, 32768), ("B32-L4096", "padded", 32, 4096),
         ("B1-L4096", "padded", 1, 4096), ("B1-L131072", "padded", 1, 131072), ("B8-L4096", "padded", 8, 4096),
         ("B8-L1024", "padded", 8, 1024), ("fp8", "fp8", 8, 16384), ("fp8-B1-L32768", "fp8", 1, 32768), ("fp8-B1-L4096", "fp8", 1, 4096)]
HEADS = {256: (16, 8), 128: (32, 16)}   # D -> (H, H_kv): the same cache bytes per key
CAP = 50.0


def make_call(kind, B, L, D, seed):
    """(the call, the cache's bytes per element, what SDPA gets: q, K, V [B, H_kv, L, D] bf16)"""
    H, Hkv = HEADS[D]
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16, generator=g)
    q = mk(B, H, 1, D)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    if kind in ("padded", "softcap", "fp8"):
        kc, vc = mk(B, Hkv, L, D), mk(B, Hkv, L, D)
        if kind == "padded":
            return (lambda: M.flash_attention_kvcache(q, kc, vc, sl)), 2, (q, kc, vc)
        if kind == "softcap":
            return (lambda: M.flash_attention_kvcache_softcap(q, kc, vc, sl, CAP)), 2, (q, kc, vc)
        k8, kd = M.quantize_kv_fp8(kc.float())
        v8, vd = M.quantize_kv_fp8(vc.float())
        return (lambda: M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd)), 1, (q, kc, vc)
    mp = L // PAGE                                            # pages per sequence; a permuted table over the whole pool
    kp, vp = mk(B * mp, Hkv, PAGE, D), mk(B * mp, Hkv, PAGE, D)
    table = torch.randperm(B * mp, generator=torch.Generator().manual_seed(seed)).to(torch.int32).view(B, mp).cuda()
    gathered = lambda pool: pool[table.long()].permute(0, 2, 1, 3, 4).reshape(B, Hkv, L, D)
    if kind == "paged":
        return (lambda: flash_attention_kvcache_paged(q, kp, vp, sl, table)), 2, (q, gathered(kp), gathered(vp))
    qp = q[:, :, 0].contiguous()                              # pure decode: one packed row per sequence
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
    return (lambda: flash_attention_kvcache_ragged(qp, kp, vp, cu, sl, table)), 2, (q, gathered(kp), gathered(vp))


def splits_of(kind, B, L, D):
    H, Hkv = HEADS[D]
    f = fa.lib.fa_fwd_kvcache_fp8_workspace_bytes if kind == "fp8" else fa.lib.fa_fwd_kvcache_workspace_bytes
    return max(1, f(B, H, Hkv, 1, L, 0, D) // (B * H * (D + 2) * 4))


def bench_point(name, kind, B, L, a):
    f256, esize, (q, K, V) = make_call(kind, B, L, 256, seed=L + B)
    fsdpa = lambda: F.scaled_dot_product_attention(q, K, V, enable_gqa=True)
    o, ref = f256(), fsdpa()
    line = {"point": name, "kind": kind, "B": B, "L": L, "S_q": 1, "dtype": "bf16", "d256": dict(zip(("H", "H_kv"), HEADS[256])),
            "d128": dict(zip(("H", "H_kv"), HEADS[128])), "splits_d256": splits_of(kind, B, L, 256),
            "splits_d128": splits_of(kind, B, L, 128), "finite": bool(torch.isfinite(o).all())}
    if kind != "softcap":
        line["rel_diff_vs_sdpa"] = round(float((o.float().reshape(ref.shape) - ref.float()).norm() / ref.float().norm()), 5)
    f128, _, keep = make_call(kind, B, L, 128, seed=L + B + 1)
    for _ in range(a.warmup):
        f256(), f128(), fsdpa()
    t256, t128, t128b, tsd = [], [], [], []
    for _ in range(a.rounds):
        t256.append(time_ms(f256, a.iters))
        t128.append(time_ms(f128, a.iters))
        tsd.append(time_ms(fsdpa, max(1, a.iters // 4)))
        t128b.append(time_ms(f128, a.iters))
    nbytes = lambda D: B * L * HEADS[D][1] * 2 * D * esize + 2 * B * HEADS[D][0] * D * 2
    ms, m1, m2, msd = min(t256), min(t128), min(t128b), min(tsd)
    bw256, bw128 = nbytes(256) / (ms * 1e-3), nbytes(128) / (min(m1, m2) * 1e-3)
    line.update({"d256_ms": round(ms, 4), "d128_ms": round(m1, 4), "d128_again_ms": round(m2, 4), "sdpa_ms": round(msd, 4),
                 "bytes_d256": nbytes(256), "bytes_d128": nbytes(128), "d256_TBps": round(bw256 / 1e12, 3),
                 "d128_TBps": round(bw128 / 1e12, 3), "rate_vs_d128": round(bw256 / bw128, 4),
                 "spread_d128": round(abs(m1 - m2) / min(m1, m2), 4), "ratio_vs_sdpa": round(ms / msd, 4),
                 "device": torch.cuda.get_device_name(0)})
    return line


def sweep(a):
    out = []
    for name, kind, B, L in SWEEP:
        f256, _, keep = make_call(kind, B, L, 256, seed=L + B)
        res = {"point": name, "kind": kind, "B": B, "H": HEADS[256][0], "H_kv": HEADS[256][1], "S_q": 1, "D": 256, "L": L,
               "formula": splits_of(kind, B, L, 256)}
        for n in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64):
            if n > 1 and L // n < 64:
                continue
            set_splits(n)
            for _ in range(a.warmup):
                f256()
            res["ms_n%d" % n] = round(min(time_ms(f256, a.iters) for _ in range(a.rounds)), 4)
        set_splits(0)
        print(json.dumps(res), flush=True)
        out.append(res)
        del f256, keep
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
