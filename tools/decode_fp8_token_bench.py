#!/usr/bin/env python3
"""Decoding attention over a per-token-scaled e4m3 KV cache (fp8_token_kvcache.flash_attention_kvcache_fp8_token and its paged
and packed forms) against flash_attention_kvcache_fp8 on a per-tensor e4m3 cache and flash_attention_kvcache on a bf16 cache of
the same shape, in ONE process, the three calls alternating round by round.  Timed with HIP events over --iters back-to-back
calls after warm-up, best of --rounds; the spread of each call's own rounds ((max - min) / min) is reported.  There is no pass
mark: from bytes alone the step costs (D + 4) / D of the per-tensor e4m3 step, and `over_bytes_by` says how far the measured
ratio lies above that, to be read against `spread`.

Points: B8 H32 H_kv 8 S_q 1 L16384 at D 128 and 64, bf16: padded, over 128-key pages under a permuted table, and packed pure
decode (one row per sequence) over the same pages; and packed D 256 at B8 H16 H_kv 8.  Per point: the three times, the ratios to
the e4m3 and the bf16 step, the split count, the call's algorithmic bytes (bytes AND scales of the visible rows + Q + O),
bytes/s and its share of the 6.3 TB/s a copy reaches, and the relative difference of the output from the bf16-cache output
(quantisation error), beside the per-tensor e4m3 call's.  One JSON line per point.

--sweep instead times forced split counts (fa_debug_kvcache_splits) of the padded call at the points of
profiles/decode_fp8_split_sweep.jsonl: the data behind keeping the e4m3 split rule.

usage: tools/decode_fp8_token_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl] [--sweep]"""
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
import fp8_token_kvcache as FT  # noqa: E402
import paged_kvcache as PG  # noqa: E402
import ragged_kvcache as RG  # noqa: E402
from decode_bench import COPY_BW, set_splits, time_ms  # noqa: E402

PAGE = 128
F8 = torch.float8_e4m3fn
# (B, H, H_kv, D, L, geometry)
POINTS = [(8, 32, 8, D, 16384, geo) for geo in ("padded", "paged", "packed") for D in (128, 64)] + [(8, 16, 8, 256, 16384, "packed")]
SWEEP = [(1, 32, 8, 128, 4096), (1, 32, 8, 128, 32768), (1, 32, 8, 128, 131072), (8, 32, 8, 128, 4096), (8, 32, 8, 128, 16384),
         (8, 32, 8, 64, 16384), (32, 32, 8, 128, 4096), (8, 32, 1, 128, 16384), (8, 32, 32, 128, 16384), (32, 32, 8, 64, 4096),
         (1, 32, 8, 64, 32768)]


def splits_of(B, H, Hkv, D, L, packed):
    if packed:
        ws = fa.lib.fa_fwd_kvcache_fp8_token_ragged_workspace_bytes(B, B, H, Hkv, L // PAGE, PAGE, D)
        plan = (16 + 8 * ((H // Hkv * B + 31 * B) // 32) + 15) // 16 * 16
        return max(1, (ws - plan) // (H * B * (D + 2) * 4))
    ws = fa.lib.fa_fwd_kvcache_fp8_token_workspace_bytes(B, H, Hkv, 1, L, 0, D)
    return max(1, ws // (B * H * (D + 2) * 4))


def setup(B, H, Hkv, D, L, others=True):
    g = torch.Generator(device="cuda").manual_seed(L + D + Hkv)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16, generator=g)
    q, kc, vc = mk(B, H, 1, D), mk(B, Hkv, L, D), mk(B, Hkv, L, D)
    kt, kts = FT.quantize_kv_fp8_per_token(kc)
    vt, vts = FT.quantize_kv_fp8_per_token(vc)
    k8 = v8 = kd = vd = None
    if others:
        k8, kd = M.quantize_kv_fp8(kc)
        v8, vd = M.quantize_kv_fp8(vc)
    else:
        kc = vc = None
    return q, (kc, vc), (k8, v8, kd, vd), (kt, vt, kts, vts), torch.full((B,), L, dtype=torch.int32, device="cuda")


def to_pages(t, perm):
    """[B, H_kv, L, w] -> the pool [B * L / PAGE, H_kv, PAGE, w] with sequence b's page i at perm[b * L / PAGE + i]"""
    B, Hkv, L, w = t.shape
    pool = t.view(B, Hkv, L // PAGE, PAGE, w).permute(0, 2, 1, 3, 4).reshape(B * (L // PAGE), Hkv, PAGE, w)
    return torch.empty_like(pool).index_copy_(0, perm, pool)


def bench_point(B, H, Hkv, D, L, geo, a):
    q, (kc, vc), (k8, v8, kd, vd), (kt, vt, kts, vts), sl = setup(B, H, Hkv, D, L)
    if geo == "padded":
        f16 = lambda: M.flash_attention_kvcache(q, kc, vc, sl)
        f8 = lambda: M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd)
        ft = lambda: FT.flash_attention_kvcache_fp8_token(q, kt, vt, kts, vts, sl)
    else:
        n = B * (L // PAGE)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
        table = perm.view(B, L // PAGE).to(torch.int32)
        kc, vc = to_pages(kc, perm), to_pages(vc, perm)
        k8, v8, kt, vt = (to_pages(t.view(torch.uint8), perm).view(F8) for t in (k8, v8, kt, vt))
        kts, vts = (to_pages(t.unsqueeze(-1), perm).squeeze(-1).contiguous() for t in (kts, vts))
        if geo == "paged":
            f16 = lambda: PG.flash_attention_kvcache_paged(q, kc, vc, sl, table)
            f8 = lambda: PG.flash_attention_kvcache_paged(q, k8, v8, sl, table, k_descale=kd, v_descale=vd)
            ft = lambda: FT.flash_attention_kvcache_fp8_token_paged(q, kt, vt, kts, vts, sl, table)
        else:   # pure decode: one packed row per sequence
            qp = q.view(B, H, D)
            cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
            f16 = lambda: RG.flash_attention_kvcache_ragged(qp, kc, vc, cu, sl, table)
            f8 = lambda: RG.flash_attention_kvcache_ragged(qp, k8, v8, cu, sl, table, k_descale=kd, v_descale=vd)
            ft = lambda: FT.flash_attention_kvcache_fp8_token_ragged(qp, kt, vt, kts, vts, cu, sl, table)
    rows, qo = B * L, 2 * B * H * D * 2
    nbytes = rows * Hkv * 2 * (D + 4) + qo
    nbytes8 = rows * Hkv * 2 * D + qo
    line = {"B": B, "H": H, "H_kv": Hkv, "S_q": 1, "D": D, "dtype": "bf16", "kv_dtype": "e4m3_per_token", "L": L, "geometry": geo,
            "page_size": 0 if geo == "padded" else PAGE, "splits": splits_of(B, H, Hkv, D, L, geo == "packed")}
    ot, o8, o16 = ft(), f8(), f16()
    rel = lambda o: round(float((o.float() - o16.float()).norm() / o16.float().norm()), 5)
    line["rel_diff_vs_bf16_cache"], line["fp8_rel_diff_vs_bf16_cache"] = rel(ot), rel(o8)
    line["finite"] = bool(torch.isfinite(ot).all())
    for _ in range(a.warmup):
        f16()
        f8()
        ft()
    t16, t8, tt = [], [], []
    for _ in range(a.rounds):
        t16.append(time_ms(f16, a.iters))
        t8.append(time_ms(f8, a.iters))
        tt.append(time_ms(ft, a.iters))
    mst, ms8, ms16 = min(tt), min(t8), min(t16)
    sp = lambda t: (max(t) - min(t)) / min(t)
    spread = max(sp(tt), sp(t8))
    bw = nbytes / (mst * 1e-3)
    line.update({"token_ms": round(mst, 4), "fp8_ms": round(ms8, 4), "bf16_ms": round(ms16, 4),
                 "ratio_to_fp8": round(mst / ms8, 4), "ratio_to_bf16": round(mst / ms16, 4),
                 "bytes_ratio_to_fp8": round(nbytes / nbytes8, 4), "over_bytes_by": round(mst / ms8 - nbytes / nbytes8, 4),
                 "spread": round(spread, 4), "spread_bf16": round(sp(t16), 4), "bytes": nbytes,
                 "TBps": round(bw / 1e12, 3), "share_of_copy_6p3": round(bw / COPY_BW, 3),
                 "fp8_TBps": round(nbytes8 / (ms8 * 1e-3) / 1e12, 3), "iters": a.iters, "rounds": a.rounds,
                 "device": torch.cuda.get_device_name(0)})
    return line


def sweep(a):
    out = []
    for B, H, Hkv, D, L in SWEEP:
        q, _, _, (kt, vt, kts, vts), sl = setup(B, H, Hkv, D, L, others=False)
        res = {"B": B, "H": H, "H_kv": Hkv, "S_q": 1, "D": D, "L": L, "kv_dtype": "e4m3_per_token",
               "formula": splits_of(B, H, Hkv, D, L, False)}
        ft = lambda: FT.flash_attention_kvcache_fp8_token(q, kt, vt, kts, vts, sl)
        for n in sorted({1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, res["formula"]}):   # (the rule's own count among them)
            if n > 1 and L // n < 64:
                continue
            set_splits(n)
            for _ in range(a.warmup):
                ft()
            res["ms_n%d" % n] = round(min(time_ms(ft, a.iters) for _ in range(a.rounds)), 4)
        set_splits(0)
        best = min((v, k) for k, v in res.items() if k.startswith("ms_n"))
        res["best"], res["formula_over_best"] = best[1], round(res.get("ms_n%d" % res["formula"], float("nan")) / best[0] - 1, 4)
        print(json.dumps(res), flush=True)
        out.append(res)
        del q, kt, vt, kts, vts
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
