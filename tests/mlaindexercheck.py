"""What the indexer-logits tests share (not a test module): a paged FP8 key pool under a permuted table with poison everywhere
nothing may read, the fp64 truth on the cache's own bytes and scales (products of two e4m3 values are exact in fp32: there is no
quantisation error to allow for), and the check.  Bound, per element: |got - truth| <= BOUND * M, M = k_scale[t] * sum_h |w_h| *
sum_d |q_hd * k_td|: 200 * 2^-24, the worst case of any fp32 summation order over 128 + 64 terms plus the final multiplies, plus
4 * 6.42e-6 for the instruction itself -- v_mfma_f32_16x16x128_f8f6f4 sums its 128 exact products below fp32; measured with one
instruction per logit against fp64 (the one-hot-head test: a logit is one accumulator element times the key's scale): up to
6.42e-6 of sum_d |q_d * k_d|, where an fp32 sum stays near 1e-7 (README).  A missing dim or head moves a logit by about 1e-2 * M.
Hidden columns are -inf bit for bit, visible ones finite.  MI355FA_MLA_INDEXER_ERRORS_JSONL=path records every check's maximum of
|got - truth| / M (profiles/mla_indexer_errors.jsonl)."""
import json
import os

import torch

F8 = torch.float8_e4m3fn
BOUND = 200 * 2.0 ** -24 + 4 * 6.42e-6


class Problem:
    """B = len(fills) sequences of fills[b] cached keys in pages of `page` keys, `mp` table entries each.  Host: q8, w, keys and
    scales (the logical caches [B, mp * page, ...]).  Device: q, wd, pool, scale, table, sl; 0x7F bytes and NaN scales wherever no
    row below fills[b] lives, table entries of 2^30 past `reach` keys.  row_stride pads rows; joined: one bytes-then-scales buffer."""

    def __init__(self, fills, Hi, Sq, page, mp, seed, row_stride=128, joined=False, reach=None):
        g = torch.Generator().manual_seed(seed)
        B, S = len(fills), mp * page
        self.fills, self.Hi, self.Sq, self.page, self.mp = list(fills), Hi, Sq, page, mp
        self.q8 = torch.randn(B, Sq, Hi, 128, generator=g).to(F8)
        self.w = torch.randn(B, Sq, Hi, generator=g) * Hi ** -0.5                       # both signs
        self.keys = torch.randn(B, S, 128, generator=g).to(F8)
        self.scales = torch.exp2(torch.rand(B, S, generator=g) * 12 - 6)                # 2^-6 ... 2^6
        n = B * mp + 3
        slots = torch.randperm(n, generator=g)[:B * mp].view(B, mp)
        if joined:
            buf, views = torch.full((n, page * 132), 0x7F, dtype=torch.uint8), \
                lambda x: (x[:, :page * 128].view(n, page, 128), x[:, page * 128:].view(torch.float32))
        else:
            buf, views = torch.full((n, page, row_stride), 0x7F, dtype=torch.uint8), lambda x: (x[..., :128], None)
        pool, scale = views(buf)
        scale = torch.empty(n, page) if scale is None else scale
        scale.fill_(float("nan"))
        table = torch.full((B, mp), 1 << 30, dtype=torch.int32)
        reach = self.fills if reach is None else reach                                   # keys the table must reach (appends)
        for b in range(B):
            used = -(-reach[b] // page)
            table[b, :used] = slots[b, :used]
            for t in range(fills[b]):
                pool[slots[b, t // page], t % page] = self.keys[b, t].view(torch.uint8)
                scale[slots[b, t // page], t % page] = self.scales[b, t]
        self.q, self.wd, self.table = self.q8.cuda(), self.w.cuda(), table.cuda()
        self.pool, dscale = views(buf.cuda())
        self.scale = scale.cuda() if dscale is None else dscale
        self.sl = torch.tensor(self.fills, dtype=torch.int32).cuda()

    def args(self):
        return self.q, self.wd, self.pool, self.scale, self.sl, self.table


def truth(q8, w, keys, scales, Ls, causal, W):
    """(fp64 logits [B, Sq, W] with -inf where hidden, M, the visibility mask); columns past the caches' length are hidden"""
    B, Sq = q8.shape[:2]
    S = keys.shape[1]
    qd, kd, wd, sd = q8.double(), keys.double(), w.double(), scales.double()
    s = torch.einsum("bihd,btd->biht", qd, kd)
    ref = (wd[..., None] * s.clamp_min(0)).sum(2) * sd[:, None]
    M = (wd.abs()[..., None] * torch.einsum("bihd,btd->biht", qd.abs(), kd.abs())).sum(2) * sd[:, None]
    t = torch.arange(W)
    L = torch.tensor(Ls)[:, None, None]
    vis = (t < L) & ((t <= L - Sq + torch.arange(Sq)[None, :, None]) | (not causal))
    out = torch.full((B, Sq, W), float("-inf"), dtype=torch.float64)
    m = torch.zeros(B, Sq, W, dtype=torch.float64)
    n = min(S, W)
    out[..., :n], m[..., :n] = ref[..., :n], M[..., :n]
    return torch.where(vis, out, torch.full_like(out, float("-inf"))), m, vis


def held(tag, got, ref, M, vis):
    """hidden columns -inf bit for bit, visible ones finite and within BOUND * M of the truth; returns max |err| / M"""
    got = got.detach().cpu()
    assert (got[~vis].view(torch.int32) == -8388608).all(), (tag, "a hidden column is not -inf")
    assert torch.isfinite(got[vis]).all(), (tag, "a visible column is not finite")
    err = (got[vis].double() - ref[vis]).abs()
    rel = float((err / M[vis].clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: max |err| / M = %.3e (bound %.3e)" % (tag, rel, BOUND))
    path = os.environ.get("MI355FA_MLA_INDEXER_ERRORS_JSONL")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": tag, "max_err_over_M": rel, "bound": BOUND, "visible": int(vis.sum())}) + "\n")
    assert (err <= BOUND * M[vis]).all(), (tag, rel)
    return rel
