#!/usr/bin/env python3
"""Sparse MLA prefill (mla_sparse_prefill.flash_attention_mla_sparse_prefill) against the only thing a user could do without
it: push the step through the decode call (mla_sparse_kvcache.flash_attention_mla_kvcache_sparse) as ONE sequence of S_q = M
rows over the same rows laid into 64-key pages, with the same lists.  Both calls in ONE process, alternating round by round,
timed with HIP events over --iters back-to-back calls after a warm-up of both, best of --rounds; the spread of each call's own
rounds ((max - min) / min) is reported.  There is no pass mark: nobody had measured either call at these sizes, and each point is
written down whichever way it falls.

Settings: bf16, topk 2048, lists uniform random without replacement among the keys a row may see, ascending, -1 padded -- what
mla_indexer_select returns.  Points: M = N = 4096 causal at H 128 and at H 16; M 512 behind 15872 cached keys (N 16384) at H 128.
Achieved TFLOP/s counts the visible products only: 2 * (576 + 512) per (head, visible entry).

--pkg DIR measures the package in DIR instead of the tree's (a variant build of the library with its bindings beside it): how the
placement claim of csrc/fa_mla_sparse_prefill.hip was measured against the plain order token = id / HB.

usage: tools/mla_sparse_prefill_bench.py [--iters N] [--warmup W] [--rounds R] [--out file.jsonl] [--pkg DIR] [--tag TEXT]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPK, PAGE = 2048, 64
# (name, M, N, H)
POINTS = [("causal-prompt", 4096, 4096, 128), ("causal-prompt-h16", 4096, 4096, 16), ("chunk-with-context", 512, 16384, 128)]


def lists(M, N, seed):
    """int32 [M, TOPK] on the device: row i sees keys [0, N - M + i + 1)"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.rand(M, N, generator=g, device="cuda")
    r[torch.arange(N, device="cuda")[None] > (N - M + torch.arange(M, device="cuda"))[:, None]] = -1.0
    val, idx = r.topk(TOPK, dim=1)
    idx = torch.where(val < 0, torch.full_like(idx, N), idx).sort(1).values
    return torch.where(idx >= N, torch.full_like(idx, -1), idx).to(torch.int32)


def bench_point(name, M, N, H, a, PRE, DEC, time_ms):
    import torch
    g = torch.Generator(device="cuda").manual_seed(M + N + H)
    q = torch.randn(M, H, 576, generator=g, device="cuda").to(torch.bfloat16)
    kv = torch.randn(N, 576, generator=g, device="cuda").to(torch.bfloat16)
    idx = lists(M, N, H)
    visible = int((idx >= 0).sum())
    q4, pool, idx3 = q.transpose(0, 1)[None], kv.view(N // PAGE, PAGE, 576), idx[None]
    sl = torch.tensor([N], dtype=torch.int32, device="cuda")
    table = torch.arange(N // PAGE, dtype=torch.int32, device="cuda")[None]
    out, out4 = torch.empty(M, H, 512, dtype=q.dtype, device="cuda"), torch.empty(1, H, M, 512, dtype=q.dtype, device="cuda")
    pre = lambda: PRE.flash_attention_mla_sparse_prefill(q, kv, idx, out=out)
    dec = lambda: DEC.flash_attention_mla_kvcache_sparse(q4, pool, idx3, sl, table, out=out4)
    o, ref = pre().float(), dec()[0].transpose(0, 1).float()
    line = {"point": name, "M": M, "N": N, "H": H, "topk": TOPK, "dtype": "bf16", "visible": visible, "tag": a.tag,
            "finite": bool(torch.isfinite(o).all()), "rel_diff_vs_decode_call": round(float((o - ref).norm() / ref.norm()), 5)}
    fns = (pre, dec)
    for _ in range(a.warmup):
        for f in fns:
            f()
    t = [[], []]
    for _ in range(a.rounds):
        for k, f in enumerate(fns):
            t[k].append(time_ms(f, a.iters))
    ms, ms_d = (min(x) for x in t)
    sp = lambda x: round((max(x) - min(x)) / min(x), 4)
    line.update({"prefill_ms": round(ms, 4), "decode_call_ms": round(ms_d, 4), "ratio_to_decode_call": round(ms / ms_d, 4),
                 "spread": sp(t[0]), "spread_decode_call": sp(t[1]),
                 "faster_than_decode_call_beyond_spread": bool(max(t[0]) < min(t[1])),
                 "tflops_visible": round(2.0 * (576 + 512) * H * visible / (ms * 1e-3) / 1e12, 1),
                 "tflops_visible_decode_call": round(2.0 * (576 + 512) * H * visible / (ms_d * 1e-3) / 1e12, 1),
                 "TBps_gathered_per_head_block": round(-(-H // 32) * visible * 1152 / (ms * 1e-3) / 1e12, 3),
                 "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)})
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))
    ap.add_argument("--tag", default="tree", help="written into every line: which build was measured")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    import mla_sparse_kvcache as DEC
    import mla_sparse_prefill as PRE
    from decode_bench import time_ms
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no fallback"
    assert os.path.dirname(os.path.abspath(PRE.__file__)) == os.path.abspath(a.pkg), PRE.__file__
    lines = []
    for pt in POINTS:
        line = bench_point(*pt, a, PRE, DEC, time_ms)
        print(json.dumps(line), flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as fh:
            fh.writelines(json.dumps(x) + "\n" for x in lines)
    return 0 if all(x["finite"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
