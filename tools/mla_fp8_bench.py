#!/usr/bin/env python3
"""MLA decoding over the FP8 latent cache (mla_fp8_kvcache.flash_attention_mla_kvcache_fp8) against the 16-bit call
(mla_kvcache.flash_attention_mla_kvcache) on the same logical cache, in ONE process, the calls alternating round by round.
Timed with HIP events over --iters back-to-back calls after a warm-up of both, best of --rounds; spread = the larger
(max - min) / min of the two calls' rounds.  There is no pass mark: each point is written down whichever way it falls.

Settings: bf16, B 8, one query per sequence, L 16384, 64-key pages under a permuted table.  Points: H 16 (bound by the bytes of
the cache) and H 128 (bound by the MFMAs).  TB/s counts 656 bytes per cached key for the FP8 call and 1152 for the 16-bit one.
  --sweep   forced split counts (fa_debug_kvcache_splits) for both calls: the rule's count (mla_splits, shared), the best
            forced count of each and how far the rule is off it.

One JSON line per point.  usage: tools/mla_fp8_bench.py [--iters N] [--warmup W] [--rounds R] [--sweep] [--out file.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import _mi355fa as fa  # noqa: E402
import mla_fp8_kvcache as F8  # noqa: E402
import mla_kvcache as MLA  # noqa: E402
from decode_bench import set_splits, time_ms  # noqa: E402
from mla_ragged_bench import rounds_of, spread  # noqa: E402

PAGE, B, L = 64, 8, 16384
D, DV = 576, 512
SWEEP = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)
BF = torch.bfloat16
POINTS = {"b8_h16": 16, "b8_h128": 128}


def setup(H):
    """q, the 16-bit pool holding the DEQUANTISED rows (the same logical cache), the byte pool, the table, the lengths"""
    g = torch.Generator(device="cuda").manual_seed(L + H)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=BF, generator=g)
    q, kv = mk(B, H, 1, D), mk(B, L, D)
    rows = F8.quantize_mla_latent_fp8(kv)
    kv16 = F8.dequantize_mla_latent_fp8(rows, BF).to(BF)
    n = B * (L // PAGE)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
    pool8 = torch.empty(n, PAGE, F8.MLA_FP8_ROW_BYTES, device="cuda", dtype=torch.uint8).index_copy_(0, perm, rows.view(n, PAGE, -1))
    pool16 = torch.empty(n, PAGE, D, device="cuda", dtype=BF).index_copy_(0, perm, kv16.view(n, PAGE, D))
    return q, pool16, pool8, perm.view(B, L // PAGE).to(torch.int32), torch.full((B,), L, dtype=torch.int32, device="cuda")


def splits(H, mp):
    ws = fa.lib.fa_fwd_kvcache_mla_fp8_workspace_bytes(B, H, 1, mp, PAGE, 0)
    return max(1, ws // (B * H * (DV + 2) * 4))


def calls(H):
    q, pool16, pool8, table, sl = setup(H)
    f8 = lambda: F8.flash_attention_mla_kvcache_fp8(q, pool8, sl, table)
    f16 = lambda: MLA.flash_attention_mla_kvcache(q, pool16, sl, table)
    return f8, f16, table.shape[1]


def bench_point(name, a):
    H = POINTS[name]
    f8, f16, mp = calls(H)
    o, ref = f8(), f16()
    line = {"point": name, "B": B, "H": H, "S_q": 1, "L": L, "dtype": "bf16", "page_size": PAGE, "splits": splits(H, mp),
            "finite": bool(torch.isfinite(o).all()),
            "rel_diff_vs_16bit": round(float((o.float() - ref.float()).norm() / ref.float().norm()), 6)}
    t8, t16 = rounds_of([f8, f16], a)
    ms8, ms16 = min(t8), min(t16)
    line.update({"fp8_ms": round(ms8, 4), "bf16_ms": round(ms16, 4), "ratio_to_16bit": round(ms8 / ms16, 4),
                 "spread": round(max(spread(t8), spread(t16)), 4),
                 "fp8_TBps": round(B * L * F8.MLA_FP8_ROW_BYTES / (ms8 * 1e-3) / 1e12, 3),
                 "bf16_TBps": round(B * L * D * 2 / (ms16 * 1e-3) / 1e12, 3),
                 "fp8_TFLOPS": round(2 * H * B * L * (D + DV) / (ms8 * 1e-3) / 1e12, 1),
                 "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)})
    return line


def sweep_point(name, a):
    H = POINTS[name]
    f8, f16, mp = calls(H)
    n0 = splits(H, mp)
    res = {"point": name + "_sweep", "B": B, "H": H, "L": L, "dtype": "bf16", "page_size": PAGE, "formula": n0}
    for n in sorted(set(SWEEP) | {n0}):
        set_splits(n)
        t8, t16 = rounds_of([f8, f16], a)
        res["fp8_ms_n%d" % n], res["bf16_ms_n%d" % n] = round(min(t8), 4), round(min(t16), 4)
    set_splits(0)
    for k in ("fp8", "bf16"):
        best = min((v, key) for key, v in res.items() if key.startswith(k + "_ms_n"))
        res[k + "_best"], res[k + "_formula_over_best"] = best[1], round(res["%s_ms_n%d" % (k, n0)] / best[0] - 1, 4)
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
