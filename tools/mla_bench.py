#!/usr/bin/env python3
"""MLA decoding over a paged latent cache (mla_kvcache.flash_attention_mla_kvcache) against PyTorch's
scaled_dot_product_attention(q, k[:, None], k[:, None, ..., :512], enable_gqa=True) on the gathered cache, in ONE process, the
two calls alternating round by round.  Timed with HIP events over --iters back-to-back calls after a warm-up of both, best of
--rounds; the spread of each call's own rounds ((max - min) / min) is reported.  There is no pass mark: nobody had measured this
kernel, and each point is written down whichever way it falls.

Settings: bf16, 64-key pages under a permuted table.  Points: B8 H128 S_q 1 L16384 (no tensor parallelism), B8 H16 S_q 1 L16384
(TP 8), B8 H128 S_q 2 L16384 (an MTP draft; our call causal, SDPA unmasked: it has no bottom-right aligned mask) and B32 H16 S_q 1
L4096.  Per point: the time, TB/s over the latent bytes counted once (B * L * 576 * 2) and its share of the 6.3 TB/s a copy
reaches, TFLOPS counted as 2 * rows * L * (576 + 512), the split count, SDPA's time and the ratio.  One JSON line per point.

--sweep instead times forced split counts (fa_debug_kvcache_splits) at the same points: the data behind the split rule
(csrc/fa_decode_mla.hip mla_splits).

usage: tools/mla_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl] [--sweep]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import _mi355fa as fa  # noqa: E402
import mla_kvcache as MLA  # noqa: E402
from decode_bench import COPY_BW, set_splits, time_ms  # noqa: E402

PAGE = 64
D, DV = 576, 512
# (B, H, S_q, L)
POINTS = [(8, 128, 1, 16384), (8, 16, 1, 16384), (8, 128, 2, 16384), (32, 16, 1, 4096)]


def splits_of(B, H, Sq, L):
    ws = fa.lib.fa_fwd_kvcache_mla_workspace_bytes(B, H, Sq, L // PAGE, PAGE, 0)
    return max(1, ws // (B * H * Sq * (DV + 2) * 4))


def setup(B, H, Sq, L):
    g = torch.Generator(device="cuda").manual_seed(L + H + Sq)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16, generator=g)
    q, kv = mk(B, H, Sq, D), mk(B, L, D)
    n = B * (L // PAGE)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
    pool = torch.empty(n, PAGE, D, device="cuda", dtype=torch.bfloat16).index_copy_(0, perm, kv.view(n, PAGE, D))
    table = perm.view(B, L // PAGE).to(torch.int32)
    return q, kv, pool, table, torch.full((B,), L, dtype=torch.int32, device="cuda")


def bench_point(B, H, Sq, L, a):
    q, kv, pool, table, sl = setup(B, H, Sq, L)
    ours = lambda: MLA.flash_attention_mla_kvcache(q, pool, sl, table, is_causal=Sq > 1)
    k = kv[:, None]
    sdpa = lambda: F.scaled_dot_product_attention(q, k, k[..., :DV], enable_gqa=True)
    line = {"B": B, "H": H, "S_q": Sq, "L": L, "dtype": "bf16", "page_size": PAGE, "causal": Sq > 1, "splits": splits_of(B, H, Sq, L)}
    o, ref = ours(), sdpa()
    line["finite"] = bool(torch.isfinite(o).all())
    if Sq == 1:   # (S_q 2: the two calls mask differently)
        line["rel_diff_vs_sdpa"] = round(float((o.float() - ref.float()).norm() / ref.float().norm()), 5)
    for _ in range(a.warmup):
        ours()
        sdpa()
    tm, ts = [], []
    for _ in range(a.rounds):
        tm.append(time_ms(ours, a.iters))
        ts.append(time_ms(sdpa, a.iters))
    ms, ms_sdpa = min(tm), min(ts)
    sp = lambda t: (max(t) - min(t)) / min(t)
    nbytes, flops = B * L * D * 2, 2 * B * H * Sq * L * (D + DV)
    bw = nbytes / (ms * 1e-3)
    line.update({"mla_ms": round(ms, 4), "sdpa_ms": round(ms_sdpa, 4), "ratio_to_sdpa": round(ms / ms_sdpa, 4),
                 "spread": round(sp(tm), 4), "spread_sdpa": round(sp(ts), 4), "latent_bytes": nbytes, "TBps": round(bw / 1e12, 3),
                 "share_of_copy_6p3": round(bw / COPY_BW, 3), "TFLOPS": round(flops / (ms * 1e-3) / 1e12, 1),
                 "sdpa_TFLOPS": round(flops / (ms_sdpa * 1e-3) / 1e12, 1), "iters": a.iters, "rounds": a.rounds,
                 "device": torch.cuda.get_device_name(0)})
    return line


def sweep(a):
    out = []
    for B, H, Sq, L in POINTS:
        q, _, pool, table, sl = setup(B, H, Sq, L)
        res = {"B": B, "H": H, "S_q": Sq, "L": L, "dtype": "bf16", "page_size": PAGE, "formula": splits_of(B, H, Sq, L)}
        ours = lambda: MLA.flash_attention_mla_kvcache(q, pool, sl, table, is_causal=Sq > 1)
        for n in sorted({1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, res["formula"]}):   # (the rule's own count among them)
            set_splits(n)
            for _ in range(a.warmup):
                ours()
            res["ms_n%d" % n] = round(min(time_ms(ours, a.iters) for _ in range(a.rounds)), 4)
        set_splits(0)
        best = min((v, k) for k, v in res.items() if k.startswith("ms_n"))
        res["best"], res["formula_over_best"] = best[1], round(res["ms_n%d" % res["formula"]] / best[0] - 1, 4)
        print(json.dumps(res), flush=True)
        out.append(res)
        del q, pool, table
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
