#!/usr/bin/env python3
"""What the ALiBi bias costs, in ONE process, interleaved, best of --rounds (HIP events), every path output-checked:

  (a) fwd+bwd of flash_attention_alibi against flash_attention_gqa at the same shape without a bias (the same kernel
      family, so the ratio is the price of the bias): an MPT-7B-like point B4 H32 S4096 D128 bf16 (H_kv = H), causal and
      window (4095, 0), and B4 H32 S4096 D64 causal;
  (b) the same calls against torch SDPA with a materialised bf16 ALiBi attn_mask [1, H, S, S] (what an HF BLOOM / MPT
      user runs today; autograd).  The line records which SDPA backend accepted the call;
  (c) a decode step of flash_attention_kvcache_alibi against flash_attention_kvcache at B8 H32 H_kv8 S_q1 L16384 D128.

Output checks: (a) / (b) the ALiBi O and dQ / dK / dV, and those of the timed SDPA path, against eager attention with
the same bias run once in fp32 on the same inputs (relFro); (c) the decode O against an fp32 eager biased reference.
One JSON line per comparison; ratio = alibi_ms / other_ms.  Slopes: alibi_slopes(H), the paper's.

usage: tools/alibi_bench.py [--iters N] [--warmup W] [--rounds R] [--train-points 0,1,2] [--no-decode]
                            [--out profiles/alibi_bench_lines.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch.nn.attention import SDPBackend, sdpa_kernel  # noqa: E402

import My_FlashAttention_optimized as M  # noqa: E402

# (B, H, H_kv, S, D, window)
TRAIN = [(4, 32, 32, 4096, 128, (-1, 0)), (4, 32, 32, 4096, 128, (4095, 0)), (4, 32, 32, 4096, 64, (-1, 0))]
DECODE = (8, 32, 8, 1, 16384, 128)


def time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def alibi_mask(slopes, Sq, Sk, window, dtype, offset=0):
    """[1, H, S_q, S_k] additive mask: -slope |i + offset - j| where visible (window (left, right), query i at position
    i + offset), -inf elsewhere"""
    i = torch.arange(Sq, device=slopes.device)[:, None] + offset
    j = torch.arange(Sk, device=slopes.device)[None, :]
    dead = (j > i + window[1]) if window[1] >= 0 else torch.zeros_like(j > i)
    if window[0] >= 0:
        dead = dead | (j < i - window[0])
    m = -slopes.float()[:, None, None] * (i - j).abs().float()
    return m.masked_fill(dead, -torch.inf)[None].to(dtype)


def rel(x, y):
    return float((x.float() - y.float()).norm() / y.float().norm())


def interleaved(fns, a):
    for _ in range(a.warmup):
        for f in fns:
            f()
    best = [float("inf")] * len(fns)
    for _ in range(a.rounds):
        for n, f in enumerate(fns):
            best[n] = min(best[n], time_ms(f, a.iters))
    return best


def sdpa_backend(q, k, v, mask):
    """The first backend, in PyTorch's priority order, that accepts the masked call (the one the default dispatch runs)"""
    for b in (SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION, SDPBackend.MATH):
        try:
            with sdpa_kernel([b]):
                F.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=k.shape[1] != q.shape[1])
            return b.name
        except RuntimeError:
            continue
    return "none"


def train_point(B, H, Hkv, S, D, w, a):
    g = torch.Generator(device="cuda").manual_seed(S + D + Hkv)
    mk = lambda h: torch.randn(B, h, S, D, device="cuda", generator=g).to(torch.bfloat16)
    q, k, v = mk(H).requires_grad_(True), mk(Hkv).requires_grad_(True), mk(Hkv).requires_grad_(True)
    do = mk(H)
    slopes = M.alibi_slopes(H, device="cuda")
    mask = alibi_mask(slopes, S, S, w, torch.bfloat16)
    causal = w == (-1, 0)
    with torch.no_grad():
        backend = sdpa_backend(q[:, :, :256], k[:, :, :256], v[:, :, :256], mask[:, :, :256, :256])

    def run(kind):
        def f():
            if kind == "alibi":
                o = M.flash_attention_alibi(q, k, v, slopes, window_size=w)
            elif kind == "gqa":
                o = M.flash_attention_gqa(q, k, v, window_size=w)
            else:
                o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=Hkv != H)
            o.backward(do)
            return o
        return f

    fa_, fg, fs = run("alibi"), run("gqa"), run("sdpa")
    outs = {}
    for name, f in (("alibi", fa_), ("sdpa", fs)):
        for t in (q, k, v):
            t.grad = None
        o = f()
        torch.cuda.synchronize()
        outs[name] = [o.detach()] + [t.grad.clone() for t in (q, k, v)]
    q32, k32, v32 = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    m32 = alibi_mask(slopes, S, S, w, torch.float32)
    r = H // Hkv
    s32 = (q32 @ k32.repeat_interleave(r, 1).transpose(-1, -2)) * D ** -0.5 + m32
    o32 = torch.softmax(s32, -1) @ v32.repeat_interleave(r, 1)
    o32.backward(do.float())
    ref = [o32.detach()] + [t.grad for t in (q32, k32, v32)]
    del o32, s32, m32, q32, k32, v32
    errs = [rel(x, y) for x, y in zip(outs["alibi"], ref)]
    errs_sdpa = [rel(x, y) for x, y in zip(outs["sdpa"], ref)]
    finite = all(bool(torch.isfinite(x).all()) for x in outs["alibi"])
    del outs, ref
    torch.cuda.empty_cache()
    ms_a, ms_g, ms_s = interleaved((fa_, fg, fs), a)
    fl = M.local_attention_flops(B, H, S, S, D, w[0], w[1], "fwd_bwd")
    base = {"B": B, "H": H, "H_kv": Hkv, "S": S, "D": D, "dtype": "bf16", "window": list(w), "causal": causal,
            "slopes": "alibi_slopes(H)", "alibi_ms": round(ms_a, 4), "alibi_tflops": round(fl / (ms_a * 1e-3) / 1e12, 1),
            "check_vs_fp32_eager_relfro": {n: round(e, 5) for n, e in zip(("O", "dQ", "dK", "dV"), errs)},
            "finite": finite, "device": torch.cuda.get_device_name(0)}
    yield dict(base, comparison="a: fwd+bwd alibi vs flash_attention_gqa (no bias)", other_ms=round(ms_g, 4),
               ratio=round(ms_a / ms_g, 4))
    yield dict(base, comparison="b: fwd+bwd alibi vs SDPA with a materialised bf16 ALiBi mask", other_ms=round(ms_s, 4),
               ratio=round(ms_a / ms_s, 4), sdpa_backend=backend, sdpa_mask_GiB=round(mask.numel() * 2 / 2 ** 30, 3),
               sdpa_vs_fp32_eager_relfro={n: round(e, 5) for n, e in zip(("O", "dQ", "dK", "dV"), errs_sdpa)})


def decode_point(a):
    B, H, Hkv, Sq, L, D = DECODE
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(B, H, Sq, D, device="cuda", generator=g).to(torch.bfloat16)
    kc, vc = (torch.randn(B, Hkv, L, D, device="cuda", generator=g).to(torch.bfloat16) for _ in range(2))
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    slopes = M.alibi_slopes(H, device="cuda")
    fa_ = lambda: M.flash_attention_kvcache_alibi(q, kc, vc, sl, slopes)
    fk = lambda: M.flash_attention_kvcache(q, kc, vc, sl)
    o = fa_()
    kf, vf = kc.float().repeat_interleave(H // Hkv, 1), vc.float().repeat_interleave(H // Hkv, 1)
    m = alibi_mask(slopes, Sq, L, (-1, -1), torch.float32, offset=L - Sq)
    ref = torch.softmax((q.float() @ kf.transpose(-1, -2)) * D ** -0.5 + m, -1) @ vf
    err = rel(o, ref)
    ms_a, ms_k = interleaved((fa_, fk), a)
    gb = 2 * B * Hkv * L * D * 2 / 1e9
    yield {"comparison": "c: decode step alibi vs flash_attention_kvcache", "B": B, "H": H, "H_kv": Hkv, "S_q": Sq, "L": L,
           "D": D, "dtype": "bf16", "slopes": "alibi_slopes(H)", "alibi_ms": round(ms_a, 4), "other_ms": round(ms_k, 4),
           "ratio": round(ms_a / ms_k, 4), "alibi_kv_GBps": round(gb / (ms_a * 1e-3), 1),
           "check_vs_fp32_eager_relfro": {"O": round(err, 5)}, "finite": bool(torch.isfinite(o).all()),
           "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds; the best of each path is kept")
    ap.add_argument("--train-points", default=",".join(str(i) for i in range(len(TRAIN))), help="indices into TRAIN")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for i in (int(x) for x in a.train_points.split(",") if x):
        for line in train_point(*TRAIN[i], a):
            print(json.dumps(line), flush=True)
            lines.append(line)
        torch.cuda.empty_cache()
    for line in ([] if a.no_decode else decode_point(a)):
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x["finite"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
