#!/usr/bin/env python3
"""What logit soft-capping costs, in ONE process, interleaved, best of --rounds (HIP events), every path output-checked:

  (a) fwd+bwd of flash_attention_softcap against flash_attention_gqa at the same shape without a cap (the same kernel
      family, so the ratio is the price of the cap): a Gemma-2-27B-like point B4 H32 H_kv16 S4096 D128 bf16, causal and
      window (4095, 0), and B4 H32 S4096 D64 causal (H_kv = H);
  (b) the same calls against eager PyTorch soft-capped attention (matmul, tanh, mask, softmax, matmul; autograd) -- what a
      Gemma 2 / Grok-1 user runs without this library;
  (c) a decode step of flash_attention_kvcache_softcap against flash_attention_kvcache at B8 H32 H_kv8 S_q1 L16384 D128.

Output checks: (a) / (b) the soft-capped O and dQ / dK / dV, and those of the timed bf16 eager path, against the eager path
run once in fp32 on the same inputs (relFro); (c) the decode O against an fp32 eager soft-capped reference.  One JSON line
per comparison; ratio = softcap_ms / other_ms.

usage: tools/softcap_bench.py [--iters N] [--warmup W] [--rounds R] [--train-points 0,1,2] [--no-decode]
                              [--out profiles/softcap_bench_lines.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))

import torch  # noqa: E402

import My_FlashAttention_optimized as M  # noqa: E402

CAP = 50.0
# (B, H, H_kv, S, D, window, scale)
TRAIN = [(4, 32, 16, 4096, 128, (-1, 0), 144 ** -0.5), (4, 32, 16, 4096, 128, (4095, 0), 144 ** -0.5),
         (4, 32, 32, 4096, 64, (-1, 0), 64 ** -0.5)]
DECODE = (8, 32, 8, 1, 16384, 128)


def time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def eager_softcap(q, k, v, cap, scale, window):
    """Soft-capped attention as eager ops; the mask is top-left aligned (training) with window = (left, right)."""
    g = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    u = cap * torch.tanh((q @ k.transpose(-1, -2)) * (scale / cap))
    i = torch.arange(q.shape[2], device=q.device)[:, None]
    j = torch.arange(k.shape[2], device=q.device)[None, :]
    dead = (j > i + window[1]) if window[1] >= 0 else torch.zeros_like(j > i)
    if window[0] >= 0:
        dead = dead | (j < i - window[0])
    return torch.softmax(u.masked_fill(dead, -torch.inf), dim=-1) @ v


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


def train_point(B, H, Hkv, S, D, w, scale, a):
    g = torch.Generator(device="cuda").manual_seed(S + D + Hkv)
    mk = lambda h, amp=1.0: (torch.randn(B, h, S, D, device="cuda", generator=g) * amp).to(torch.bfloat16)
    q = mk(H, 0.6 * CAP / (scale * D ** 0.5)).requires_grad_(True)   # scores at about 0.6 x the cap
    k, v = mk(Hkv).requires_grad_(True), mk(Hkv).requires_grad_(True)
    do = mk(H)
    causal = w == (-1, 0)

    def run(kind):
        def f():
            if kind == "softcap":
                o = M.flash_attention_softcap(q, k, v, CAP, window_size=w, softmax_scale=scale)
            elif kind == "gqa":
                o = M.flash_attention_gqa(q, k, v, window_size=w)
            else:
                o = eager_softcap(q, k, v, CAP, scale, w)
            o.backward(do)
            return o
        return f

    fs, fg, fe = run("softcap"), run("gqa"), run("eager")
    outs = {}
    for name, f in (("softcap", fs), ("eager", fe)):
        for t in (q, k, v):
            t.grad = None
        o = f()
        torch.cuda.synchronize()
        outs[name] = [o.detach()] + [t.grad.clone() for t in (q, k, v)]
    q32, k32, v32 = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    o32 = eager_softcap(q32, k32, v32, CAP, scale, w)
    o32.backward(do.float())
    ref = [o32.detach()] + [t.grad for t in (q32, k32, v32)]
    del o32, q32, k32, v32
    errs = [rel(x, y) for x, y in zip(outs["softcap"], ref)]
    errs_eager = [rel(x, y) for x, y in zip(outs["eager"], ref)]
    finite = all(bool(torch.isfinite(x).all()) for x in outs["softcap"])
    del outs, ref
    torch.cuda.empty_cache()
    ms_s, ms_g, ms_e = interleaved((fs, fg, fe), a)
    fl = M.local_attention_flops(B, H, S, S, D, w[0], w[1], "fwd_bwd")
    base = {"B": B, "H": H, "H_kv": Hkv, "S": S, "D": D, "dtype": "bf16", "window": list(w), "causal": causal, "softcap": CAP,
            "scale": round(scale, 6), "softcap_ms": round(ms_s, 4), "softcap_tflops": round(fl / (ms_s * 1e-3) / 1e12, 1),
            "check_vs_fp32_eager_relfro": {n: round(e, 5) for n, e in zip(("O", "dQ", "dK", "dV"), errs)},
            "bf16_eager_vs_fp32_eager_relfro": {n: round(e, 5) for n, e in zip(("O", "dQ", "dK", "dV"), errs_eager)},
            "finite": finite,
            "device": torch.cuda.get_device_name(0)}
    yield dict(base, comparison="a: fwd+bwd softcap vs flash_attention_gqa (no cap)", other_ms=round(ms_g, 4),
               ratio=round(ms_s / ms_g, 4))
    yield dict(base, comparison="b: fwd+bwd softcap vs eager soft-capped attention", other_ms=round(ms_e, 4),
               ratio=round(ms_s / ms_e, 4))


def decode_point(a):
    B, H, Hkv, Sq, L, D = DECODE
    g = torch.Generator(device="cuda").manual_seed(1)
    scale = D ** -0.5
    q = (torch.randn(B, H, Sq, D, device="cuda", generator=g) * (0.6 * CAP / (scale * D ** 0.5))).to(torch.bfloat16)
    kc, vc = (torch.randn(B, Hkv, L, D, device="cuda", generator=g).to(torch.bfloat16) for _ in range(2))
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    fs = lambda: M.flash_attention_kvcache_softcap(q, kc, vc, sl, CAP)
    fk = lambda: M.flash_attention_kvcache(q, kc, vc, sl)
    o = fs()
    kf, vf = kc.float().repeat_interleave(H // Hkv, 1), vc.float().repeat_interleave(H // Hkv, 1)
    ref = torch.softmax(CAP * torch.tanh((q.float() @ kf.transpose(-1, -2)) * (scale / CAP)), -1) @ vf
    err = rel(o, ref)
    ms_s, ms_k = interleaved((fs, fk), a)
    gb = 2 * B * Hkv * L * D * 2 / 1e9
    yield {"comparison": "c: decode step softcap vs flash_attention_kvcache", "B": B, "H": H, "H_kv": Hkv, "S_q": Sq, "L": L,
           "D": D, "dtype": "bf16", "softcap": CAP, "softcap_ms": round(ms_s, 4), "other_ms": round(ms_k, 4),
           "ratio": round(ms_s / ms_k, 4), "softcap_kv_GBps": round(gb / (ms_s * 1e-3), 1),
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
