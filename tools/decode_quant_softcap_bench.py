#!/usr/bin/env python3
"""Soft-capped decoding over the three quantised KV-cache formats (quant_softcap_kvcache.py: per-tensor e4m3, per-token e4m3,
MXFP4) against the UNCAPPED call of the same format and geometry, in ONE process, the two calls alternating round by round.  The
uncapped call's kernels are instruction for instruction the previous commit's (profiles/decode_quant_softcap_isa_diff.txt), so
the ratio is the cost of the transform alone.  Timed with HIP events over --iters back-to-back calls after warm-up, best of
--rounds; the spread of each call's own rounds ((max - min) / min) is reported beside the ratio.  There is no pass mark: the
16-bit soft-capped step costs 1.02x its uncapped step at this point (README), `over_16bit_by` says how far a ratio lies above
that, to be read against `spread`.

Points, bf16, cap 50: B8 H32 H_kv 8 S_q 1 L16384 at D 128 and 64 -- padded, over 128-key pages under a permuted table, and packed
pure decode (one row per sequence) over the same pages -- and packed D 256 at B8 H16 H_kv 8, for each format.  One JSON line per
(format, point).

--sweep instead times forced split counts (fa_debug_kvcache_splits) of the padded capped call at the D 128 point of each
format: how far each format's split rule, kept as it is, lies from the best swept count.

usage: tools/decode_quant_softcap_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl] [--sweep]"""
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
import fp4_ragged_kvcache as R4  # noqa: E402
import fp8_token_kvcache as FT  # noqa: E402
import paged_kvcache as PG  # noqa: E402
import quant_softcap_kvcache as QS  # noqa: E402
import ragged_kvcache as RG  # noqa: E402
from decode_bench import set_splits, time_ms  # noqa: E402

PAGE = 128
CAP = 50.0
SOFTCAP_16BIT = 1.02     # the 16-bit soft-capped step over its uncapped step at B8 L16384 (README)
FORMATS = ("e4m3", "e4m3_per_token", "mxfp4")
FMT_ID = {"e4m3": fa.QUANT_E4M3, "e4m3_per_token": fa.QUANT_E4M3_TOKEN, "mxfp4": fa.QUANT_MXFP4}
# (B, H, H_kv, D, L, geometry)
POINTS = [(8, 32, 8, D, 16384, geo) for geo in ("padded", "paged", "packed") for D in (128, 64)] + [(8, 16, 8, 256, 16384, "packed")]


def splits_of(fmt, B, H, Hkv, D, L, packed):
    if packed:
        ws = fa.lib.fa_fwd_kvcache_quant_softcap_ragged_workspace_bytes(FMT_ID[fmt], B, B, H, Hkv, L // PAGE, PAGE, D)
        plan = (16 + 8 * ((H // Hkv * B + 31 * B) // 32) + 15) // 16 * 16
        return max(1, (ws - plan) // (H * B * (D + 2) * 4))
    ws = fa.lib.fa_fwd_kvcache_quant_softcap_workspace_bytes(FMT_ID[fmt], B, H, Hkv, 1, L, 0, D)
    return max(1, ws // (B * H * (D + 2) * 4))


def to_pages(t, perm):
    """[B, H_kv, L, ...] -> the pool [B * L / PAGE, H_kv, PAGE, ...] with sequence b's page i at perm[b * L / PAGE + i]"""
    if t.dtype == torch.float8_e4m3fn:   # (bytes: the copy is by index)
        return to_pages(t.view(torch.uint8), perm).view(torch.float8_e4m3fn)
    B, Hkv, L = t.shape[:3]
    rest = t.shape[3:]
    pool = t.reshape(B, Hkv, L // PAGE, PAGE, -1).permute(0, 2, 1, 3, 4).reshape(B * (L // PAGE), Hkv, PAGE, *rest)
    return torch.empty_like(pool).index_copy_(0, perm, pool)


def setup(fmt, B, H, Hkv, D, L):
    """q with the amplitude that puts the score standard deviation at 0.6 x cap, and the cache in the format: (k, v, the capped
    call's keywords)"""
    g = torch.Generator(device="cuda").manual_seed(L + D + Hkv)
    q = (torch.randn(B, H, 1, D, device="cuda", generator=g) * (0.6 * CAP)).to(torch.bfloat16)   # scale 1 / sqrt(D): amp = 0.6 cap
    kc, vc = (torch.randn(B, Hkv, L, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
    if fmt == "e4m3":
        (k, kd), (v, vd) = M.quantize_kv_fp8(kc), M.quantize_kv_fp8(vc)
        return q, k, v, dict(k_descale=kd, v_descale=vd)
    quant = FT.quantize_kv_fp8_per_token if fmt == "e4m3_per_token" else F4.quantize_kv_mxfp4
    (k, ks), (v, vs) = quant(kc), quant(vc)
    return q, k, v, dict(k_scale=ks, v_scale=vs)


def calls(fmt, geo, q, k, v, kw, sl, table):
    """(the capped call, the uncapped call of the same format and geometry)"""
    B, H, _, D = q.shape
    s = (kw.get("k_scale"), kw.get("v_scale"))
    if geo == "padded":
        capped = lambda: QS.flash_attention_kvcache_quant_softcap(q, k, v, sl, CAP, **kw)
        plain = {"e4m3": lambda: M.flash_attention_kvcache_fp8(q, k, v, sl, kw.get("k_descale"), kw.get("v_descale")),
                 "e4m3_per_token": lambda: FT.flash_attention_kvcache_fp8_token(q, k, v, *s, sl),
                 "mxfp4": lambda: F4.flash_attention_kvcache_fp4(q, k, v, *s, sl)}[fmt]
    elif geo == "paged":
        capped = lambda: QS.flash_attention_kvcache_quant_softcap_paged(q, k, v, sl, table, CAP, **kw)
        plain = {"e4m3": lambda: PG.flash_attention_kvcache_paged(q, k, v, sl, table, **kw),
                 "e4m3_per_token": lambda: FT.flash_attention_kvcache_fp8_token_paged(q, k, v, *s, sl, table),
                 "mxfp4": lambda: F4.flash_attention_kvcache_fp4_paged(q, k, v, *s, sl, table)}[fmt]
    else:   # pure decode: one packed row per sequence
        qp = q.view(B, H, D)
        cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
        capped = lambda: QS.flash_attention_kvcache_quant_softcap_ragged(qp, k, v, cu, sl, table, CAP, **kw)
        plain = {"e4m3": lambda: RG.flash_attention_kvcache_ragged(qp, k, v, cu, sl, table, **kw),
                 "e4m3_per_token": lambda: FT.flash_attention_kvcache_fp8_token_ragged(qp, k, v, *s, cu, sl, table),
                 "mxfp4": lambda: R4.flash_attention_kvcache_fp4_ragged(qp, k, v, *s, cu, sl, table)}[fmt]
    return capped, plain


def bench_point(fmt, B, H, Hkv, D, L, geo, a):
    q, k, v, kw = setup(fmt, B, H, Hkv, D, L)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    table = None
    if geo != "padded":
        n = B * (L // PAGE)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
        table = perm.view(B, L // PAGE).to(torch.int32)
        k, v = to_pages(k, perm), to_pages(v, perm)
        kw = {name: (to_pages(t, perm) if name.endswith("_scale") else t) for name, t in kw.items()}
    capped, plain = calls(fmt, geo, q, k, v, kw, sl, table)
    line = {"B": B, "H": H, "H_kv": Hkv, "S_q": 1, "D": D, "dtype": "bf16", "kv_dtype": fmt, "L": L, "geometry": geo, "softcap": CAP,
            "page_size": 0 if geo == "padded" else PAGE, "splits": splits_of(fmt, B, H, Hkv, D, L, geo == "packed")}
    oc, op = capped(), plain()
    line["finite"] = bool(torch.isfinite(oc).all())
    line["rel_diff_capped_vs_uncapped"] = round(float((oc.float() - op.float()).norm() / op.float().norm()), 4)   # the cap matters
    for _ in range(a.warmup):
        plain()
        capped()
    tp, tc = [], []
    for _ in range(a.rounds):
        tp.append(time_ms(plain, a.iters))
        tc.append(time_ms(capped, a.iters))
    sp = lambda t: (max(t) - min(t)) / min(t)
    ratio = min(tc) / min(tp)
    line.update({"capped_ms": round(min(tc), 4), "uncapped_ms": round(min(tp), 4), "ratio": round(ratio, 4),
                 "spread": round(max(sp(tc), sp(tp)), 4), "over_16bit_by": round(ratio - SOFTCAP_16BIT, 4), "iters": a.iters,
                 "rounds": a.rounds, "device": torch.cuda.get_device_name(0)})
    return line


def sweep(a):
    out = []
    B, H, Hkv, D, L = 8, 32, 8, 128, 16384
    for fmt in FORMATS:
        q, k, v, kw = setup(fmt, B, H, Hkv, D, L)
        sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
        capped, _ = calls(fmt, "padded", q, k, v, kw, sl, None)
        res = {"B": B, "H": H, "H_kv": Hkv, "S_q": 1, "D": D, "L": L, "kv_dtype": fmt, "softcap": CAP,
               "formula": splits_of(fmt, B, H, Hkv, D, L, False)}
        for n in sorted({1, 2, 3, 4, 6, 8, 12, 16, 24, 32, res["formula"]}):   # (the rule's own count among them)
            set_splits(n)
            for _ in range(a.warmup):
                capped()
            res["ms_n%d" % n] = round(min(time_ms(capped, a.iters) for _ in range(a.rounds)), 4)
        set_splits(0)
        best = min((t, name) for name, t in res.items() if name.startswith("ms_n"))
        res["best"], res["formula_over_best"] = best[1], round(res["ms_n%d" % res["formula"]] / best[0] - 1, 4)
        print(json.dumps(res), flush=True)
        out.append(res)
        del q, k, v, kw, capped
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
        for fmt in FORMATS:
            for pt in POINTS:
                line = bench_point(fmt, *pt, a)
                print(json.dumps(line), flush=True)
                lines.append(line)
                torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x.get("finite", True) for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
