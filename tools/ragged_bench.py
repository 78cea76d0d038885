#!/usr/bin/env python3
"""Paged-cache decoding with packed variable-length queries (ragged_kvcache.flash_attention_kvcache_ragged) against what
covers the same step without it, in ONE process: HIP events over --iters back-to-back calls after a pre-roll, the sides
interleaved round by round, best of --rounds, and the per-round ratios beside it (their spread is the noise a ratio has to
be read against).  bf16, D 128, H 32, H_kv 8, pages of 128 keys, a randomly permuted table.

  pure_decode   B 8, every S_b = 1, L 16384, against flash_attention_kvcache_paged on the same keys: the cost of the plan
                kernel and of the lookup.  plan_ms is the plan kernel alone (fa_debug_ragged_plan, HIP events); `within` says
                whether ragged <= paged + plan + the round-to-round spread of the ragged times.  Also on an e4m3 pool.
  spec_verify   B 32, S_b uniform in 1..8 (seeded), L 16384, causal, against the paged call on q left-padded to S_q = 8.
  mixed_step    one 512-token chunk over L 4096 plus 63 decode rows over L 16384, causal, against the two paged calls that
                cover it (B 1 S_q 512 and B 63 S_q 1), timed together; gqa_ms is flash_attention_gqa on the chunk's gathered
                keys alone (the mask bottom-right aligned through its window), chunk_ms the ragged call on the chunk alone.
  --sweep       forced split counts (fa_debug_kvcache_splits) at the three points and on the e4m3 pool at the first: the
                formula's count, the best forced count and how far the formula is off it.

One JSON line per point.  usage: tools/ragged_bench.py [--iters N] [--warmup W] [--rounds R] [--sweep] [--out file.jsonl]"""
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
from paged_kvcache import flash_attention_kvcache_paged as paged  # noqa: E402
from ragged_kvcache import flash_attention_kvcache_ragged as ragged  # noqa: E402

H, HKV, D, PAGE, LMAX = 32, 8, 128, 128, 16384
BF16 = torch.bfloat16
SWEEP = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 64)


def force(n):
    fn = fa.lib.fa_debug_kvcache_splits
    fn.argtypes, fn.restype = [ctypes.c_int], None
    fn(n)


def time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def rounds_of(fns, a):
    """[[ms per round] per function], the functions interleaved round by round after the pre-roll"""
    for _ in range(a.warmup):
        for f in fns:
            f()
    t = [[] for _ in fns]
    for _ in range(a.rounds):
        for i, f in enumerate(fns):
            t[i].append(time_ms(f, a.iters))
    return t


class Pool:
    """B sequences with room for LMAX keys each in pages of PAGE keys, stored in a random order"""

    def __init__(self, B, fp8, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        n = B * (LMAX // PAGE)
        mk = lambda: torch.randn(n, HKV, PAGE, D, device="cuda", dtype=BF16, generator=g)
        self.kp, self.vp = mk(), mk()
        self.kw = {}
        if fp8:
            self.kp, self.vp = self.kp.to(torch.float8_e4m3fn), self.vp.to(torch.float8_e4m3fn)
            self.kw = dict(k_descale=torch.full((HKV,), 0.5, device="cuda"), v_descale=torch.full((HKV,), 0.5, device="cuda"))
        self.table = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).view(B, LMAX // PAGE).to(torch.int32).cuda()
        self.g = g

    def q(self, *shape):
        return torch.randn(*shape, device="cuda", dtype=BF16, generator=self.g)


def formula_splits(T, B, fp8):
    force(0)
    ws = fa.lib.fa_fwd_kvcache_ragged_workspace_bytes(T, B, H, HKV, LMAX // PAGE, PAGE, D, int(fp8))
    plan = (16 + 8 * ((H // HKV * T + 31 * B) // 32) + 15) // 16 * 16
    return max(1, (ws - plan) // (H * T * (D + 2) * 4))


def base_line(point, S, lens, fp8, n):
    return {"point": point, "B": len(S), "total_q": sum(S), "max_S": max(S), "H": H, "H_kv": HKV, "D": D, "page_size": PAGE,
            "L": sorted(set(lens)), "cache": "e4m3" if fp8 else "bf16", "splits": n, "device": torch.cuda.get_device_name(0)}


def ratios(x, y):
    return [round(p / q, 4) for p, q in zip(x, y)]


def cu_of(S):
    return torch.tensor([0] + torch.tensor(S).cumsum(0).tolist(), dtype=torch.int32, device="cuda")


def plan_ms(cu, T, B, a):
    ws = torch.empty(fa.lib.fa_fwd_kvcache_ragged_workspace_bytes(T, B, H, HKV, LMAX // PAGE, PAGE, D, 0), dtype=torch.uint8,
                     device="cuda")
    fn = fa.lib.fa_debug_ragged_plan
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p], ctypes.c_int
    s = torch.cuda.current_stream().cuda_stream
    f = lambda: fa.check(fn(cu.data_ptr(), ws.data_ptr(), T, B, H, HKV, s), "fa_debug_ragged_plan")
    return min(rounds_of([f], a)[0])


def sweep(point, f, S, lens, fp8, a):
    n0 = formula_splits(sum(S), len(S), fp8)
    times = {}
    for n in sorted(set(SWEEP) | {n0}):
        force(n)
        times[n] = min(rounds_of([f], a)[0])
    force(0)
    best = min(times, key=times.get)
    line = base_line(point + "_sweep", S, lens, fp8, n0)
    line.update(ms={str(n): round(t, 4) for n, t in times.items()}, best_splits=best,
                formula_off_best_pct=round(100.0 * (times[n0] / times[best] - 1.0), 2))
    return line


def pure_decode(fp8, a):
    B = 8
    S, lens = [1] * B, [LMAX] * B
    pool = Pool(B, fp8, 1 + fp8)
    q = pool.q(B, H, D)
    cu, sl = cu_of(S), torch.tensor(lens, dtype=torch.int32, device="cuda")
    f_rg = lambda: ragged(q, pool.kp, pool.vp, cu, sl, pool.table, **pool.kw)
    f_pg = lambda: paged(q.view(B, H, 1, D), pool.kp, pool.vp, sl, pool.table, **pool.kw)
    same = torch.equal(f_rg().view(torch.int16), f_pg().view(B, H, D).view(torch.int16))
    t_rg, t_pg = rounds_of([f_rg, f_pg], a)
    p_ms = plan_ms(cu, B, B, a)
    spread = max(t_rg) - min(t_rg)
    line = base_line("pure_decode", S, lens, fp8, formula_splits(B, B, fp8))
    line.update(paged_ms=round(min(t_pg), 4), ragged_ms=round(min(t_rg), 4), plan_ms=round(p_ms, 4),
                ragged_spread_ms=round(spread, 4), ratio=round(min(t_rg) / min(t_pg), 4), round_ratios=ratios(t_rg, t_pg),
                within=bool(min(t_rg) <= min(t_pg) + p_ms + spread), same_bits=bool(same))
    yield line
    if a.sweep:
        yield sweep("pure_decode", f_rg, S, lens, fp8, a)


def spec_verify(a):
    B, SMAX = 32, 8
    S = torch.randint(1, SMAX + 1, (B,), generator=torch.Generator().manual_seed(7)).tolist()
    lens = [LMAX] * B
    pool = Pool(B, False, 3)
    T = sum(S)
    q = pool.q(T, H, D)
    cu, sl = cu_of(S), torch.tensor(lens, dtype=torch.int32, device="cuda")
    qpad = torch.zeros(B, H, SMAX, D, device="cuda", dtype=BF16)           # left-padded: the real queries are the last S_b
    at = 0
    for b, s in enumerate(S):
        qpad[b, :, SMAX - s:] = q[at:at + s].transpose(0, 1)
        at += s
    f_rg = lambda: ragged(q, pool.kp, pool.vp, cu, sl, pool.table, is_causal=True)
    f_pg = lambda: paged(qpad, pool.kp, pool.vp, sl, pool.table, is_causal=True)
    o, op = f_rg(), f_pg()
    at, err = 0, 0.0
    for b, s in enumerate(S):                                                # the same rows up to the split count's rounding
        err = max(err, float((o[at:at + s].transpose(0, 1).float() - op[b, :, SMAX - s:].float()).abs().max()))
        at += s
    t_rg, t_pg = rounds_of([f_rg, f_pg], a)
    force(0)
    line = base_line("spec_verify", S, lens, False, formula_splits(T, B, False))
    line.update(padded_rows=B * SMAX, paged_padded_ms=round(min(t_pg), 4), ragged_ms=round(min(t_rg), 4),
                ratio=round(min(t_rg) / min(t_pg), 4), round_ratios=ratios(t_rg, t_pg), max_abs_diff=round(err, 5))
    yield line
    if a.sweep:
        yield sweep("spec_verify", f_rg, S, lens, False, a)


def mixed_step(a):
    B, CH, LCH = 64, 512, 4096
    S, lens = [CH] + [1] * (B - 1), [LCH] + [LMAX] * (B - 1)
    pool = Pool(B, False, 5)
    T = sum(S)
    q = pool.q(T, H, D)
    cu, sl = cu_of(S), torch.tensor(lens, dtype=torch.int32, device="cuda")
    q_ch = q[:CH].transpose(0, 1)[None].contiguous()                          # [1, H, 512, D]
    q_dec = q[CH:].view(B - 1, H, 1, D)
    sl_ch, sl_dec = sl[:1].contiguous(), sl[1:].contiguous()
    tb_ch, tb_dec = pool.table[:1].contiguous(), pool.table[1:].contiguous()
    cu_ch = cu_of([CH])
    kg = pool.kp[tb_ch[0, :LCH // PAGE].long()].transpose(0, 1).reshape(1, HKV, LCH, D).contiguous()   # the chunk's keys, gathered
    vg = pool.vp[tb_ch[0, :LCH // PAGE].long()].transpose(0, 1).reshape(1, HKV, LCH, D).contiguous()
    f_rg = lambda: ragged(q, pool.kp, pool.vp, cu, sl, pool.table, is_causal=True)

    def f_two():
        paged(q_ch, pool.kp, pool.vp, sl_ch, tb_ch, is_causal=True)
        paged(q_dec, pool.kp, pool.vp, sl_dec, tb_dec, is_causal=True)

    f_chunk = lambda: ragged(q[:CH], pool.kp, pool.vp, cu_ch, sl_ch, tb_ch, is_causal=True)
    f_gqa = lambda: M.flash_attention_gqa(q_ch, kg, vg, window_size=(-1, LCH - CH))     # key j visible up to i + L - S_q
    o = f_rg()
    err_gqa = float((o[:CH].transpose(0, 1).float() - f_gqa()[0].float()).abs().max())
    t_rg, t_two, t_ch, t_gqa = rounds_of([f_rg, f_two, f_chunk, f_gqa], a)
    line = base_line("mixed_step", S, lens, False, formula_splits(T, B, False))
    line.update(two_paged_calls_ms=round(min(t_two), 4), ragged_ms=round(min(t_rg), 4), ratio=round(min(t_rg) / min(t_two), 4),
                round_ratios=ratios(t_rg, t_two), chunk_ms=round(min(t_ch), 4), gqa_ms=round(min(t_gqa), 4),
                chunk_over_gqa=round(min(t_ch) / min(t_gqa), 4), chunk_round_ratios=ratios(t_ch, t_gqa),
                max_abs_diff_gqa=round(err_gqa, 5))
    yield line
    if a.sweep:
        yield sweep("mixed_step", f_rg, S, lens, False, a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for gen in (pure_decode(False, a), pure_decode(True, a), spec_verify(a), mixed_step(a)):
        for line in gen:
            print(json.dumps(line), flush=True)
            lines.append(line)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x.get("same_bits", True) for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
