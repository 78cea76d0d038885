#!/usr/bin/env python3
"""Packed variable-length decoding over paged MXFP4 pools (fp4_ragged_kvcache.flash_attention_kvcache_fp4_ragged) against the
calls it stands beside, in ONE process, the calls of a point alternating round by round.  Timed with HIP events over --iters
back-to-back calls after warm-up, best of --rounds; the spread of each call's own rounds ((max - min) / min) is reported.
There is no pass mark.

Points (bf16, L 16384, 128-key pages under a permuted table):
  decode      B 8, H 32, H_kv 8, D 128, one query per sequence: the packed MXFP4 call against
              flash_attention_kvcache_fp4_paged on the same pools (the baseline: existing code) and against
              flash_attention_kvcache_ragged over an e4m3 pool of the same shape
  verify      B 32, 1-8 queries per sequence: against flash_attention_kvcache_fp4_paged on q left-padded to 8
  decode_d256 B 8, H 16, H_kv 8, D 256: against flash_attention_kvcache_ragged over an e4m3 pool at D 256 and against the packed
              MXFP4 call at H 32, H_kv 16, D 128 (the same cache bytes)
Per point: the times, the ratios, the split count, the packed MXFP4 call's algorithmic bytes (nibbles AND scales of the
visible rows + Q + O) and bytes/s.  One JSON line per point.

--sweep instead times forced split counts (fa_debug_kvcache_splits) of the packed MXFP4 call, pure decode at H 32, H_kv 8,
D 128 and 256: the data behind its split rule.

usage: tools/ragged_fp4_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl] [--sweep]"""
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
import ragged_kvcache as RG  # noqa: E402
from decode_bench import COPY_BW, set_splits, time_ms  # noqa: E402

PAGE = 128
L = 16384
SWEEP = [(B, 32, 8, D, Ls) for D in (128, 256) for (B, Ls) in ((1, 4096), (1, 32768), (8, 16384), (32, 4096))]


def splits_of(T, B, H, Hkv, MP, D):
    ws = fa.lib.fa_fwd_kvcache_fp4_ragged_workspace_bytes(T, B, H, Hkv, MP, PAGE, D)
    plan = (16 + 8 * ((H // Hkv * T + 31 * B) // 32) + 15) // 16 * 16
    return max(1, (ws - plan) // (H * T * (D + 2) * 4))


def pools(B, Hkv, D, Ls, seed, fp8=False):
    """MXFP4 pools (and an e4m3 pool with its descales) of B sequences of Ls keys under one permuted table"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = B * (Ls // PAGE)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
    table = perm.view(B, Ls // PAGE).to(torch.int32)

    def to_pages(t):
        w = t.shape[-1]
        pool = t.view(B, Hkv, Ls // PAGE, PAGE, w).permute(0, 2, 1, 3, 4).reshape(n, Hkv, PAGE, w)
        return torch.empty_like(pool).index_copy_(0, perm, pool)
    out4, out8 = [], []
    for _ in range(2):                                                          # K, then V
        x = torch.randn(B, Hkv, Ls, D, device="cuda", dtype=torch.bfloat16, generator=g)
        nib, sc = F4.quantize_kv_mxfp4(x)
        out4 += [to_pages(nib), to_pages(sc)]
        if fp8:
            x8, d8 = M.quantize_kv_fp8(x)
            out8 += [to_pages(x8.view(torch.uint8)).view(torch.float8_e4m3fn), d8]
        del x
    k4, ks, v4, vs = out4
    return (k4, v4, ks, vs), (tuple(out8) if fp8 else None), table


def timed(calls, a):
    for _ in range(a.warmup):
        for f in calls.values():
            f()
    t = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, f in calls.items():
            t[k].append(time_ms(f, a.iters))
    return {k: min(v) for k, v in t.items()}, {k: (max(v) - min(v)) / min(v) for k, v in t.items()}


def bench(name, B, H, Hkv, D, S, a, fp8=False, padded_paged=False, twin=None):
    T = sum(S)
    g = torch.Generator(device="cuda").manual_seed(T + D)
    q = torch.randn(T, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
    cu = torch.tensor([0] + [sum(S[:i + 1]) for i in range(B)], dtype=torch.int32, device="cuda")
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    p4, p8, table = pools(B, Hkv, D, L, seed=D + B, fp8=fp8)
    calls = {"fp4_ragged": lambda: R4.flash_attention_kvcache_fp4_ragged(q, *p4, cu, sl, table, is_causal=True)}
    if padded_paged:                                                            # q left-padded to max(S): [B, H, max(S), D]
        Sq = max(S)
        qp = torch.zeros(B, H, Sq, D, device="cuda", dtype=torch.bfloat16)
        for b, s in enumerate(S):
            qp[b, :, Sq - s:] = q[int(cu[b]):int(cu[b]) + s].transpose(0, 1)
        calls["fp4_paged"] = lambda: F4.flash_attention_kvcache_fp4_paged(qp, *p4, sl, table, is_causal=True)
    if fp8:
        k8, kd, v8, vd = p8
        calls["fp8_ragged"] = lambda: RG.flash_attention_kvcache_ragged(q, k8, v8, cu, sl, table, is_causal=True, k_descale=kd,
                                                                        v_descale=vd)
    if twin:                                                                    # the same cache bytes at another head geometry
        tH, tHkv, tD = twin
        tq = torch.randn(T, tH, tD, device="cuda", dtype=torch.bfloat16, generator=g)
        tp4, _, ttable = pools(B, tHkv, tD, L, seed=tD + B + 1)
        calls["fp4_ragged_twin"] = lambda: R4.flash_attention_kvcache_fp4_ragged(tq, *tp4, cu, sl, ttable, is_causal=True)
    o = calls["fp4_ragged"]()
    ms, sp = timed(calls, a)
    nbytes = B * L * Hkv * 2 * (D // 2 + D // 32) + 2 * T * H * D * 2
    bw = nbytes / (ms["fp4_ragged"] * 1e-3)
    line = {"point": name, "B": B, "H": H, "H_kv": Hkv, "D": D, "dtype": "bf16", "kv_dtype": "mxfp4", "L": L, "page_size": PAGE,
            "total_q": T, "queries": "1" if max(S) == 1 else "%d-%d" % (min(S), max(S)),
            "splits": splits_of(T, B, H, Hkv, L // PAGE, D), "finite": bool(torch.isfinite(o).all())}
    for k in calls:
        line[k + "_ms"] = round(ms[k], 4)
        line[k + "_spread"] = round(sp[k], 4)
        if k != "fp4_ragged":
            line["ratio_to_" + k] = round(ms["fp4_ragged"] / ms[k], 4)
    if twin:
        line["twin"] = {"H": twin[0], "H_kv": twin[1], "D": twin[2]}
    line.update({"bytes": nbytes, "TBps": round(bw / 1e12, 3), "share_of_copy_6p3": round(bw / COPY_BW, 3), "iters": a.iters,
                 "rounds": a.rounds, "device": torch.cuda.get_device_name(0)})
    return line


def sweep(a):
    out = []
    for B, H, Hkv, D, Ls in SWEEP:
        g = torch.Generator(device="cuda").manual_seed(B + D + Ls)
        q = torch.randn(B, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
        cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
        sl = torch.full((B,), Ls, dtype=torch.int32, device="cuda")
        p4, _, table = pools(B, Hkv, D, Ls, seed=Ls + D)
        res = {"B": B, "H": H, "H_kv": Hkv, "total_q": B, "D": D, "L": Ls, "page_size": PAGE, "kv_dtype": "mxfp4", "packed": True,
               "formula": splits_of(B, B, H, Hkv, Ls // PAGE, D)}
        for n in sorted({1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, res["formula"]}):   # (the rule's own count is timed too)
            if n > 1 and Ls // n < 64:
                continue
            set_splits(n)
            f = lambda: R4.flash_attention_kvcache_fp4_ragged(q, *p4, cu, sl, table)
            for _ in range(a.warmup):
                f()
            res["ms_n%d" % n] = round(min(time_ms(f, a.iters) for _ in range(a.rounds)), 4)
        set_splits(0)
        print(json.dumps(res), flush=True)
        out.append(res)
        del q, p4
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
        verify = [1 + (5 * b + 3) % 8 for b in range(32)]                       # 1-8 queries, every count four times
        for kw in (dict(name="decode", B=8, H=32, Hkv=8, D=128, S=[1] * 8, fp8=True, padded_paged=True),
                   dict(name="verify", B=32, H=32, Hkv=8, D=128, S=verify, padded_paged=True),
                   dict(name="decode_d256", B=8, H=16, Hkv=8, D=256, S=[1] * 8, fp8=True, twin=(32, 16, 128))):
            line = bench(a=a, **kw)
            print(json.dumps(line), flush=True)
            lines.append(line)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x.get("finite", True) for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
