#!/usr/bin/env python3
"""Decoding attention over a PAGED KV cache (paged_kvcache.flash_attention_kvcache_paged) against the padded step
(flash_attention_kvcache / flash_attention_kvcache_fp8) on the same keys, in ONE process: HIP events over --iters
back-to-back calls after warm-up, the two paths interleaved round by round, best of --rounds.  The padded kernels are the
parent commit's instruction for instruction (tools/isa_diff.py), so the ratio is a comparison against the parent's code.

Points: B8 H32 H_kv8 S_q1 L16384 at D128 and D64, bf16 and e4m3 caches; page sizes 32, 128 and 256; an identity table
(page i of sequence b at b * pages + i: the padded cache's own order) and a randomly permuted one.  Per line: both times,
ratio = paged / padded (best of rounds), the per-round ratios (their spread is the noise the ratio has to be read
against), the split count, and whether the paged result has the padded result's bits.  One JSON line per point.

usage: tools/paged_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))

import torch  # noqa: E402

import _mi355fa as fa  # noqa: E402
import My_FlashAttention_optimized as M  # noqa: E402
from paged_kvcache import flash_attention_kvcache_paged  # noqa: E402

B, H, HKV, SQ, L = 8, 32, 8, 1, 16384
PAGES = (32, 128, 256)


def time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def pool_of(cache, page, perm):
    """[B, H_kv, L, D] -> the pool [B * L / page, H_kv, page, D] with page n of the padded order stored at perm[n]"""
    Bc, Hk, S, D = cache.shape
    bits = cache.view(torch.uint8 if cache.element_size() == 1 else torch.int16)
    pages = bits.view(Bc, Hk, S // page, page, D).permute(0, 2, 1, 3, 4).reshape(Bc * (S // page), Hk, page, D)
    return torch.empty_like(pages).index_copy_(0, perm, pages).view(cache.dtype)


def bench(D, fp8, a):
    g = torch.Generator(device="cuda").manual_seed(D + fp8)
    q = torch.randn(B, H, SQ, D, device="cuda", dtype=torch.bfloat16, generator=g)
    kc, vc = (torch.randn(B, HKV, L, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
    kw = {}
    if fp8:
        (kc, kd), (vc, vd) = M.quantize_kv_fp8(kc), M.quantize_kv_fp8(vc)
        kw = dict(k_descale=kd, v_descale=vd)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    padded = M.flash_attention_kvcache_fp8 if fp8 else M.flash_attention_kvcache
    f_pad = lambda: padded(q, kc, vc, sl, **kw)
    ws = (fa.lib.fa_fwd_kvcache_fp8_workspace_bytes if fp8 else fa.lib.fa_fwd_kvcache_workspace_bytes)(B, H, HKV, SQ, L, 0, D)
    o_pad = f_pad()
    for page in PAGES:
        n = B * (L // page)
        for kind in ("identity", "permuted"):
            perm = torch.arange(n, device="cuda") if kind == "identity" else \
                torch.randperm(n, generator=torch.Generator().manual_seed(page)).cuda()
            kp, vp = pool_of(kc, page, perm), pool_of(vc, page, perm)
            table = perm.view(B, L // page).to(torch.int32).contiguous()
            f_pg = lambda: flash_attention_kvcache_paged(q, kp, vp, sl, table, **kw)
            same = torch.equal(f_pg().view(torch.int16), o_pad.view(torch.int16))
            for _ in range(a.warmup):
                f_pad()
                f_pg()
            t_pad, t_pg = [], []
            for _ in range(a.rounds):
                t_pad.append(time_ms(f_pad, a.iters))
                t_pg.append(time_ms(f_pg, a.iters))
            line = {"B": B, "H": H, "H_kv": HKV, "S_q": SQ, "L": L, "D": D, "cache": "e4m3" if fp8 else "bf16",
                    "page_size": page, "table": kind, "splits": max(1, ws // (B * H * SQ * (D + 2) * 4)),
                    "padded_ms": round(min(t_pad), 4), "paged_ms": round(min(t_pg), 4),
                    "ratio": round(min(t_pg) / min(t_pad), 4),
                    "round_ratios": [round(x / y, 4) for x, y in zip(t_pg, t_pad)], "same_bits": bool(same),
                    "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            yield line
            del kp, vp
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [line for D in (128, 64) for fp8 in (False, True) for line in bench(D, fp8, a)]
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x["same_bits"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
