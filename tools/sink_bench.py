#!/usr/bin/env python3
"""What attention sinks cost, in ONE process, interleaved, best of --rounds (HIP events), every path output-checked:

  (a) fwd+bwd of flash_attention_sink (sinks requiring grad, so the sink-gradient kernel runs) against flash_attention_gqa
      at the same shape (the same tile loops and the same backward binaries: the ratio is the price of the sink epilogue
      plus fa_bwd_dsink_kernel): gpt-oss-like B4 H64 H_kv8 S4096 D64 bf16, causal and window (127, 0), and one D128 point;
  (b) the same call against eager attention that concatenates the sink column (what a user without the kernel runs;
      bf16, autograd);
  (c) a decode step of flash_attention_kvcache_sink against flash_attention_kvcache, and of
      flash_attention_kvcache_fp8_sink against flash_attention_kvcache_fp8: B8 H64 H_kv8 S_q1 L16384 D64 and
      B8 H32 H_kv8 S_q1 L16384 D128.

Output checks: (a) / (b) O, dQ, dK, dV and dz of the sink call, and those of the timed eager path, against the same eager
attention run once in fp32 (relFro; on the first batch element, whose fp32 scores fit comfortably); (c) the decode O
against an fp32 eager reference on the (dequantised) cache.  One JSON line per comparison; ratio = sink_ms / other_ms;
spread = (median - best) / best over the rounds, per path, so a ratio can be read against the noise.
Sinks: linspace(0, 8, H) for training, linspace(2, 10, H) for decoding.

usage: tools/sink_bench.py [--iters N] [--warmup W] [--rounds R] [--train-points 0,1,2] [--no-eager] [--no-decode]
                           [--out profiles/sink_bench_lines.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))

import torch  # noqa: E402

import My_FlashAttention_optimized as M  # noqa: E402

# (B, H, H_kv, S, D, window)
TRAIN = [(4, 64, 8, 4096, 64, (-1, 0)), (4, 64, 8, 4096, 64, (127, 0)), (4, 32, 8, 4096, 128, (-1, 0))]
# (B, H, H_kv, S_q, L, D)
DECODE = [(8, 64, 8, 1, 16384, 64), (8, 32, 8, 1, 16384, 128)]


def time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def rel(x, y):
    return float((x.float() - y.float()).norm() / y.float().norm())


def interleaved(fns, a):
    """[(best ms, spread)] per function: rounds interleaved, spread = (median - best) / best"""
    for _ in range(a.warmup):
        for f in fns:
            f()
    t = [[] for _ in fns]
    for _ in range(a.rounds):
        for n, f in enumerate(fns):
            t[n].append(time_ms(f, a.iters))
    return [(min(x), (statistics.median(x) - min(x)) / min(x)) for x in t]


def visible(Sq, Sk, w, device, offset=0):
    i = torch.arange(Sq, device=device)[:, None] + offset
    j = torch.arange(Sk, device=device)[None, :]
    vis = torch.ones(Sq, Sk, dtype=torch.bool, device=device)
    if w[0] >= 0:
        vis &= j >= i - w[0]
    if w[1] >= 0:
        vis &= j <= i + w[1]
    return vis


def eager_sink(q, k, v, sinks, vis):
    """Eager attention with the sink concatenated as one more score column (dropped again before P @ V), in q's dtype"""
    B, H, S, D = q.shape
    r = H // k.shape[1]
    s = (q @ k.repeat_interleave(r, 1).transpose(-1, -2)) * D ** -0.5
    s = s.masked_fill(~vis, -torch.inf)
    p = torch.softmax(torch.cat([s, sinks.to(q.dtype).view(1, H, 1, 1).expand(B, H, S, 1)], -1), -1)
    return p[..., :-1] @ v.repeat_interleave(r, 1)


def train_point(B, H, Hkv, S, D, w, a):
    g = torch.Generator(device="cuda").manual_seed(S + D + Hkv)
    mk = lambda h: torch.randn(B, h, S, D, device="cuda", generator=g).to(torch.bfloat16)
    q, k, v = mk(H).requires_grad_(True), mk(Hkv).requires_grad_(True), mk(Hkv).requires_grad_(True)
    do = mk(H)
    sinks = torch.linspace(0, 8, H, device="cuda").requires_grad_(True)
    vis = visible(S, S, w, "cuda")
    leaves = (q, k, v, sinks)

    def run(kind):
        def f():
            if kind == "sink":
                o = M.flash_attention_sink(q, k, v, sinks, window_size=w)
            elif kind == "gqa":
                o = M.flash_attention_gqa(q, k, v, window_size=w)
            else:
                o = eager_sink(q, k, v, sinks, vis)
            o.backward(do)
            return o
        return f

    fs, fg, fe = run("sink"), run("gqa"), run("eager")
    fns = (fs, fg) if a.no_eager else (fs, fg, fe)
    # ---- output check on the first batch element: the timed functions' O, and the gradients of a call on that element ----
    sl = lambda t: t.detach()[:1]
    q32, k32, v32, z32 = (x.float().requires_grad_(True) for x in (sl(q), sl(k), sl(v), sinks.detach()))
    o32 = eager_sink(q32, k32, v32, z32, vis)
    o32.backward(do[:1].float())
    ref = [o32.detach()] + [t.grad for t in (q32, k32, v32, z32)]
    del o32
    errs = {}
    for name, f in (("sink", fs),) + ((("eager", fe),) if not a.no_eager else ()):
        full = f().detach()
        q1, k1, v1, z1 = (x.clone().requires_grad_(True) for x in (sl(q), sl(k), sl(v), sinks.detach()))
        o1 = M.flash_attention_sink(q1, k1, v1, z1, window_size=w) if name == "sink" else eager_sink(q1, k1, v1, z1, vis)
        o1.backward(do[:1])
        torch.cuda.synchronize()
        got = [full[:1], q1.grad, k1.grad, v1.grad, z1.grad]
        errs[name] = {n: round(rel(x, y), 5) for n, x, y in zip(("O", "dQ", "dK", "dV", "dz"), got, ref)}
        errs[name]["finite"] = all(bool(torch.isfinite(x).all()) for x in got)
    for t in leaves:
        t.grad = None
    del ref, q32, k32, v32
    torch.cuda.empty_cache()
    res = interleaved(fns, a)
    (ms_s, sp_s), (ms_g, sp_g) = res[0], res[1]
    fl = M.local_attention_flops(B, H, S, S, D, w[0], w[1], "fwd_bwd")
    base = {"B": B, "H": H, "H_kv": Hkv, "S": S, "D": D, "dtype": "bf16", "window": list(w), "sinks": "linspace(0, 8, H), requires_grad",
            "sink_ms": round(ms_s, 4), "sink_spread": round(sp_s, 4), "sink_tflops": round(fl / (ms_s * 1e-3) / 1e12, 1),
            "check_vs_fp32_eager_relfro": errs["sink"], "finite": errs["sink"]["finite"], "rounds": a.rounds, "iters": a.iters,
            "device": torch.cuda.get_device_name(0)}
    yield dict(base, comparison="a: fwd+bwd sink vs flash_attention_gqa (no sink)", other_ms=round(ms_g, 4),
               other_spread=round(sp_g, 4), ratio=round(ms_s / ms_g, 4), extra_us=round((ms_s - ms_g) * 1e3, 1))
    if not a.no_eager:
        ms_e, sp_e = res[2]
        yield dict(base, comparison="b: fwd+bwd sink vs eager attention with a concatenated sink column (bf16)",
                   other_ms=round(ms_e, 4), other_spread=round(sp_e, 4), ratio=round(ms_s / ms_e, 4),
                   eager_vs_fp32_eager_relfro=errs["eager"])


def decode_point(B, H, Hkv, Sq, L, D, a):
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(B, H, Sq, D, device="cuda", generator=g).to(torch.bfloat16)
    kf, vf = (torch.randn(B, Hkv, L, D, device="cuda", generator=g) for _ in range(2))
    kc, vc = kf.to(torch.bfloat16), vf.to(torch.bfloat16)
    k8, kd = M.quantize_kv_fp8(kf)
    v8, vd = M.quantize_kv_fp8(vf)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    sinks = torch.linspace(2, 10, H, device="cuda")
    f16s = lambda: M.flash_attention_kvcache_sink(q, kc, vc, sl, sinks)
    f16 = lambda: M.flash_attention_kvcache(q, kc, vc, sl)
    f8s = lambda: M.flash_attention_kvcache_fp8_sink(q, k8, v8, sl, sinks, kd, vd)
    f8 = lambda: M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd)
    vis = torch.ones(Sq, L, dtype=torch.bool, device="cuda")
    with torch.no_grad():
        e16 = rel(f16s(), eager_sink(q.float(), kc.float(), vc.float(), sinks, vis))
        e8 = rel(f8s(), eager_sink(q.float(), k8.float() * kd[..., None, None], v8.float() * vd[..., None, None], sinks, vis))
        moved = rel(f16s(), f16())
    (ms16s, sp16s), (ms16, sp16), (ms8s, sp8s), (ms8, sp8) = interleaved((f16s, f16, f8s, f8), a)
    base = {"B": B, "H": H, "H_kv": Hkv, "S_q": Sq, "L": L, "D": D, "dtype": "bf16", "sinks": "linspace(2, 10, H)",
            "sink_moves_O_relfro": round(moved, 4), "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    yield dict(base, comparison="c: decode step kvcache_sink vs flash_attention_kvcache", sink_ms=round(ms16s, 4),
               sink_spread=round(sp16s, 4), other_ms=round(ms16, 4), other_spread=round(sp16, 4), ratio=round(ms16s / ms16, 4),
               sink_kv_GBps=round(2 * B * Hkv * L * D * 2 / 1e9 / (ms16s * 1e-3), 1),
               check_vs_fp32_eager_relfro={"O": round(e16, 5)}, finite=e16 == e16)
    yield dict(base, comparison="c: decode step kvcache_fp8_sink vs flash_attention_kvcache_fp8", sink_ms=round(ms8s, 4),
               sink_spread=round(sp8s, 4), other_ms=round(ms8, 4), other_spread=round(sp8, 4), ratio=round(ms8s / ms8, 4),
               sink_kv_GBps=round(2 * B * Hkv * L * D / 1e9 / (ms8s * 1e-3), 1),
               check_vs_fp32_eager_relfro={"O": round(e8, 5)}, finite=e8 == e8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds; the best of each path is kept")
    ap.add_argument("--train-points", default=",".join(str(i) for i in range(len(TRAIN))), help="indices into TRAIN")
    ap.add_argument("--no-eager", action="store_true", help="skip the eager baseline (the kernel-trace run)")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for i in (int(x) for x in a.train_points.split(",") if x):
        for line in train_point(*TRAIN[i], a):
            print(json.dumps(line), flush=True)
            lines.append(line)
        torch.cuda.empty_cache()
    for pt in ([] if a.no_decode else DECODE):
        for line in decode_point(*pt, a):
            print(json.dumps(line), flush=True)
            lines.append(line)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x["finite"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
