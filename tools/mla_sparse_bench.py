#!/usr/bin/env python3
"""Sparse (top-k indexed) MLA decoding (mla_sparse_kvcache.flash_attention_mla_kvcache_sparse) against the two things a user of
the dense call (mla_kvcache.flash_attention_mla_kvcache) can do without it, in ONE process, the three calls alternating round
by round:
  (a) the dense call over the whole L-token cache: what a user does today;
  (b) the dense call over a cache of exactly topk tokens: the same bytes and flops, contiguous, so sparse / (b) is the price of
      the gather.
Timed with HIP events over --iters back-to-back calls after a warm-up of all three, best of --rounds; the spread of each call's
own rounds ((max - min) / min) is reported.  There is no pass mark: nobody had measured this kernel, and each point is written
down whichever way it falls.

Settings: bf16, 64-key pages under a permuted table, S_q 1, topk 2048 drawn without replacement from L = 32768.  Points: B8 H128
and B8 H16.  One JSON line per point, with each call's split count.

--fp8 instead measures the sparse call over the FP8 latent cache (mla_sparse_fp8_kvcache.flash_attention_mla_kvcache_sparse_fp8)
at the same points, again three calls alternating in one process: (s) that call over the 656-byte rows; (a) the 16-bit sparse
call of the same build over the dequantised rows; (b) the dense FP8 call (mla_fp8_kvcache.flash_attention_mla_kvcache_fp8) over
a cache of exactly topk contiguous tokens, the selected rows -- so (s) / (b) is the price of gathering byte rows.

--sweep instead times forced split counts (fa_debug_kvcache_splits) of the sparse call at the same points: the data behind its
split rule (csrc/fa_decode_mla_sparse.hip mla_sparse_splits).

usage: tools/mla_sparse_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl] [--sweep | --fp8]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import _mi355fa as fa  # noqa: E402
import mla_kvcache as MLA  # noqa: E402
import mla_sparse_kvcache as SPARSE  # noqa: E402
from decode_bench import set_splits, time_ms  # noqa: E402
from mla_bench import DV, PAGE, setup, splits_of  # noqa: E402

L, TOPK = 32768, 2048
# (B, H)
POINTS = [(8, 128), (8, 16)]


def sparse_splits_of(B, H):
    ws = fa.lib.fa_fwd_kvcache_mla_sparse_workspace_bytes(B, H, 1, TOPK, L // PAGE, PAGE, 0)
    return max(1, ws // (B * H * (DV + 2) * 4))


def calls(B, H):
    """the sparse call, (a) and (b) on one problem; (b)'s cache holds the selected rows, so the three agree up to rounding"""
    q, kv, pool, table, sl = setup(B, H, 1, L)
    g = torch.Generator().manual_seed(B + H)
    idx = torch.stack([torch.randperm(L, generator=g)[:TOPK] for _ in range(B)]).to(torch.int32)[:, None].cuda()
    picked = torch.gather(kv, 1, idx[:, 0].long()[..., None].expand(B, TOPK, kv.shape[-1]))
    _, _, pool_b, table_b, sl_b = setup(B, H, 1, TOPK)
    pool_b[table_b.long().view(-1)] = picked.view(-1, PAGE, kv.shape[-1])
    sparse = lambda: SPARSE.flash_attention_mla_kvcache_sparse(q, pool, idx, sl, table)
    whole = lambda: MLA.flash_attention_mla_kvcache(q, pool, sl, table)
    short = lambda: MLA.flash_attention_mla_kvcache(q, pool_b, sl_b, table_b)
    return sparse, whole, short


def bench_point(B, H, a):
    sparse, whole, short = calls(B, H)
    line = {"B": B, "H": H, "S_q": 1, "L": L, "topk": TOPK, "dtype": "bf16", "page_size": PAGE, "splits": sparse_splits_of(B, H),
            "splits_dense_L": splits_of(B, H, 1, L), "splits_dense_topk": splits_of(B, H, 1, TOPK)}
    o, ref = sparse(), short()
    line["finite"] = bool(torch.isfinite(o).all())
    line["rel_diff_vs_dense_topk"] = round(float((o.float() - ref.float()).norm() / ref.float().norm()), 5)
    fns = (sparse, whole, short)
    for _ in range(a.warmup):
        for f in fns:
            f()
    t = [[], [], []]
    for _ in range(a.rounds):
        for k, f in enumerate(fns):
            t[k].append(time_ms(f, a.iters))
    ms, ms_a, ms_b = (min(x) for x in t)
    sp = lambda x: round((max(x) - min(x)) / min(x), 4)
    line.update({"sparse_ms": round(ms, 4), "dense_L_ms": round(ms_a, 4), "dense_topk_ms": round(ms_b, 4),
                 "ratio_to_dense_L": round(ms / ms_a, 4), "ratio_to_dense_topk": round(ms / ms_b, 4), "spread": sp(t[0]),
                 "spread_dense_L": sp(t[1]), "spread_dense_topk": sp(t[2]),
                 "TBps_gathered": round(B * TOPK * 576 * 2 / (ms * 1e-3) / 1e12, 3), "iters": a.iters, "rounds": a.rounds,
                 "device": torch.cuda.get_device_name(0)})
    return line


def calls_fp8(B, H):
    """(s), (a) and (b) of --fp8 on one problem: the byte pool and the 16-bit pool hold the same logical cache"""
    import mla_fp8_kvcache as F8
    import mla_sparse_fp8_kvcache as SPARSE8
    q, kv, pool, table, sl = setup(B, H, 1, L)
    rows = F8.quantize_mla_latent_fp8(kv)
    slots = table.long().view(-1)
    pool8 = torch.empty(len(slots), PAGE, rows.shape[-1], device="cuda", dtype=torch.uint8).index_copy_(0, slots, rows.view(len(slots), PAGE, -1))
    pool.index_copy_(0, slots, F8.dequantize_mla_latent_fp8(rows, kv.dtype).to(kv.dtype).view(len(slots), PAGE, -1))
    g = torch.Generator().manual_seed(B + H)
    idx = torch.stack([torch.randperm(L, generator=g)[:TOPK] for _ in range(B)]).to(torch.int32)[:, None].cuda()
    picked = torch.gather(rows, 1, idx[:, 0].long()[..., None].expand(B, TOPK, rows.shape[-1]))
    _, _, _, table_b, sl_b = setup(B, H, 1, TOPK)
    pool8_b = torch.empty(B * TOPK // PAGE, PAGE, rows.shape[-1], device="cuda", dtype=torch.uint8)
    pool8_b[table_b.long().view(-1)] = picked.view(-1, PAGE, rows.shape[-1])
    sparse8 = lambda: SPARSE8.flash_attention_mla_kvcache_sparse_fp8(q, pool8, idx, sl, table)
    sparse16 = lambda: SPARSE.flash_attention_mla_kvcache_sparse(q, pool, idx, sl, table)
    short8 = lambda: F8.flash_attention_mla_kvcache_fp8(q, pool8_b, sl_b, table_b)
    return sparse8, sparse16, short8


def bench_point_fp8(B, H, a):
    fns = calls_fp8(B, H)
    ws = fa.lib.fa_fwd_kvcache_mla_sparse_fp8_workspace_bytes(B, H, 1, TOPK, L // PAGE, PAGE, 0)
    ws_b = fa.lib.fa_fwd_kvcache_mla_fp8_workspace_bytes(B, H, 1, TOPK // PAGE, PAGE, 0)
    per = B * H * (DV + 2) * 4
    line = {"B": B, "H": H, "S_q": 1, "L": L, "topk": TOPK, "dtype": "bf16", "page_size": PAGE, "cache": "fp8-656",
            "splits": max(1, ws // per), "splits_sparse_16bit": sparse_splits_of(B, H), "splits_dense_fp8_topk": max(1, ws_b // per)}
    o, o16, ref = (f() for f in fns)
    rel = lambda x: round(float((x.float() - ref.float()).norm() / ref.float().norm()), 5)
    line.update({"finite": bool(torch.isfinite(o).all()), "rel_diff_vs_dense_fp8_topk": rel(o), "rel_diff_16bit_vs_dense_fp8_topk": rel(o16)})
    for _ in range(a.warmup):
        for f in fns:
            f()
    t = [[], [], []]
    for _ in range(a.rounds):
        for k, f in enumerate(fns):
            t[k].append(time_ms(f, a.iters))
    ms, ms_a, ms_b = (min(x) for x in t)
    sp = lambda x: round((max(x) - min(x)) / min(x), 4)
    line.update({"sparse_fp8_ms": round(ms, 4), "sparse_16bit_ms": round(ms_a, 4), "dense_fp8_topk_ms": round(ms_b, 4),
                 "ratio_to_sparse_16bit": round(ms / ms_a, 4), "ratio_to_dense_fp8_topk": round(ms / ms_b, 4), "spread": sp(t[0]),
                 "spread_sparse_16bit": sp(t[1]), "spread_dense_fp8_topk": sp(t[2]),
                 "TBps_gathered": round(B * TOPK * 656 / (ms * 1e-3) / 1e12, 3), "iters": a.iters, "rounds": a.rounds,
                 "device": torch.cuda.get_device_name(0)})
    return line


def sweep(a):
    out = []
    for B, H in POINTS:
        sparse, _, _ = calls(B, H)
        res = {"B": B, "H": H, "S_q": 1, "L": L, "topk": TOPK, "dtype": "bf16", "page_size": PAGE, "formula": sparse_splits_of(B, H)}
        for n in sorted({1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, res["formula"]}):   # (the rule's own count among them)
            set_splits(n)
            for _ in range(a.warmup):
                sparse()
            res["ms_n%d" % n] = round(min(time_ms(sparse, a.iters) for _ in range(a.rounds)), 4)
        set_splits(0)
        best = min((v, k) for k, v in res.items() if k.startswith("ms_n"))
        res["best"], res["formula_over_best"] = best[1], round(res["ms_n%d" % res["formula"]] / best[0] - 1, 4)
        print(json.dumps(res), flush=True)
        out.append(res)
        del sparse
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true", help="forced split counts instead of the points")
    ap.add_argument("--fp8", action="store_true", help="the sparse call over the FP8 latent cache against its two parents")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no fallback"
    if a.sweep:
        lines = sweep(a)
    else:
        lines = []
        for pt in POINTS:
            line = bench_point_fp8(*pt, a) if a.fp8 else bench_point(*pt, a)
            print(json.dumps(line), flush=True)
            lines.append(line)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x.get("finite", True) for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
