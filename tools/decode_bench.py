#!/usr/bin/env python3
"""Decoding attention over a padded KV cache (flash_attention_kvcache) against the existing path, in ONE process: for
each point the split-KV kernels and -- at uniform fill levels -- flash_attention_gqa on the cache sliced to the visible
rows (what a caller of the training kernels does today; a bottom-right causal mask there is the top-left window
(-1, L - S_q)).  Timed with HIP events over --iters back-to-back calls after warm-up, interleaved, best of --rounds.

Per point: time, split count, algorithmic bytes (the K/V rows some query can see + Q + O), bytes/s and its share of the
6.3 TB/s a copy reaches and of the 8 TB/s spec, and for the uniform points the GQA time and ratio (kvcache / gqa; below
1: the new path is faster).  One JSON line per point.

--sweep instead times forced split counts (fa_debug_kvcache_splits) at a few points: the data behind the split formula.

usage: tools/decode_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl] [--sweep]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))

import torch  # noqa: E402

import _mi355fa as fa  # noqa: E402
import My_FlashAttention_optimized as M  # noqa: E402

COPY_BW, SPEC_BW = 6.3e12, 8.0e12
RAGGED = [512, 1024, 2048, 4096, 6144, 8192, 12288, 16384]
# (B, H, H_kv, S_q, D, lengths (one int: uniform), causal, window)
POINTS = ([(1, 32, 8, 1, 128, L, False, (-1, -1)) for L in (4096, 32768, 131072)] +
          [(8, 32, 8, 1, 128, L, False, (-1, -1)) for L in (1024, 4096, 16384)] +
          [(8, 32, 8, 1, 64, 16384, False, (-1, -1)),
           (32, 32, 8, 1, 128, 4096, False, (-1, -1)),
           (8, 32, 1, 1, 128, 16384, False, (-1, -1)),
           (8, 32, 32, 1, 128, 16384, False, (-1, -1)),
           (8, 32, 8, 4, 128, 16384, True, (-1, -1)),
           (8, 32, 8, 1, 128, RAGGED, False, (-1, -1)),
           (8, 32, 8, 1, 128, 32768, False, (4095, 0))])
SWEEP = [(1, 32, 8, 1, 128, 4096), (1, 32, 8, 1, 128, 32768), (1, 32, 8, 1, 128, 131072), (8, 32, 8, 1, 128, 1024),
         (8, 32, 8, 1, 128, 4096), (8, 32, 8, 1, 128, 16384), (8, 32, 8, 1, 64, 16384), (32, 32, 8, 1, 128, 4096),
         (8, 32, 1, 1, 128, 16384), (8, 32, 32, 1, 128, 16384)]


def set_splits(n):
    fn = fa.lib.fa_debug_kvcache_splits
    fn.argtypes = [ctypes.c_int]
    fn.restype = None
    fn(n)


def splits_of(B, H, Hkv, Sq, Sc, D):
    """The split count a launch takes (from the workspace formula n * B * H * S_q * (D + 2) * 4; 0 bytes = 1 split)."""
    ws = fa.lib.fa_fwd_kvcache_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D)
    return max(1, ws // (B * H * Sq * (D + 2) * 4))


def time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def visible_rows(L, Sq, wl, wr):
    lo = 0 if wl < 0 else max(0, L - Sq - wl)
    hi = L if wr < 0 else min(L, L - 1 + wr + 1)
    return max(0, hi - lo), lo


def setup(B, H, Hkv, Sq, D, lens):
    Sc = max(lens)
    g = torch.Generator(device="cuda").manual_seed(Sc + D + Hkv + Sq)
    mk = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16, generator=g)
    return mk(B, H, Sq, D), mk(B, Hkv, Sc, D), mk(B, Hkv, Sc, D), torch.tensor(lens, dtype=torch.int32, device="cuda")


def bench_point(B, H, Hkv, Sq, D, lens, causal, window, a):
    uniform = isinstance(lens, int)
    lens = [lens] * B if uniform else list(lens)
    q, kc, vc, sl = setup(B, H, Hkv, Sq, D, lens)
    wl, wr = (window[0], 0) if causal else window
    fk = lambda: M.flash_attention_kvcache(q, kc, vc, sl, is_causal=causal, window_size=window)
    rows = [visible_rows(L, Sq, wl, wr) for L in lens]
    nbytes = sum(n for n, _ in rows) * Hkv * 2 * D * 2 + 2 * B * H * Sq * D * 2
    line = {"B": B, "H": H, "H_kv": Hkv, "S_q": Sq, "D": D, "dtype": "bf16",
            "L": lens[0] if uniform else lens, "causal": causal, "window": list(window),
            "splits": splits_of(B, H, Hkv, Sq, max(lens), D)}
    o = fk()
    fg = None
    if uniform:
        n, lo = rows[0]
        L = lens[0]
        ks, vs = kc[:, :, lo:lo + n], vc[:, :, lo:lo + n]
        gwin = (-1, n - Sq) if (causal or wr >= 0) else (-1, -1)   # bottom-right causal = top-left window (-1, n - S_q)
        fg = lambda: M.flash_attention_gqa(q, ks, vs, window_size=gwin)
        og = fg()
        line["rel_diff_vs_gqa"] = round(float((o.float() - og.float()).norm() / og.float().norm()), 5)
    line["finite"] = bool(torch.isfinite(o).all())
    for _ in range(a.warmup):
        fk()
        if fg:
            fg()
    tk, tg = [], []
    for _ in range(a.rounds):
        tk.append(time_ms(fk, a.iters))
        if fg:
            tg.append(time_ms(fg, a.iters))
    ms = min(tk)
    bw = nbytes / (ms * 1e-3)
    line.update({"kvcache_ms": round(ms, 4), "bytes": nbytes, "TBps": round(bw / 1e12, 3),
                 "share_of_copy_6p3": round(bw / COPY_BW, 3), "share_of_spec_8": round(bw / SPEC_BW, 3)})
    if fg:
        line.update({"gqa_ms": round(min(tg), 4), "ratio": round(ms / min(tg), 4)})
    line["device"] = torch.cuda.get_device_name(0)
    return line


def sweep(a):
    out = []
    for B, H, Hkv, Sq, D, L in SWEEP:
        q, kc, vc, sl = setup(B, H, Hkv, Sq, D, [L] * B)
        res = {"B": B, "H": H, "H_kv": Hkv, "S_q": Sq, "D": D, "L": L, "formula": splits_of(B, H, Hkv, Sq, L, D)}
        for n in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 128):
            if n > 1 and L // n < 64:
                continue
            set_splits(n)
            fk = lambda: M.flash_attention_kvcache(q, kc, vc, sl)
            for _ in range(a.warmup):
                fk()
            res["ms_n%d" % n] = round(min(time_ms(fk, a.iters) for _ in range(a.rounds)), 4)
        set_splits(0)
        print(json.dumps(res), flush=True)
        out.append(res)
        del q, kc, vc
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
