"""Helpers of the MLA decode tests (tests/test_gpu_mla.py, tests/test_gpu_race_mla.py, tests/test_host_mla.py; not a test
module): the problem, its pool under a permuted table, the fp64 truth and the check with the project's own bounds.

Truth: attn_ref.attention_fp64(q, kv[:, None], kv[:, None, :, :512], None, scale, visible(..., L=L)) per sequence on its first
L rows -- one latent head, the value of a key = the first 512 values of its row.  Bounds, per sequence (each fill level is a
problem of its own): fp16 relFro < 1e-3; bf16 < max(2 x PyTorch's bf16 SDPA on the same (q, K, V = K[..., :512]) problem,
4e-3); LSE rtol 1e-3 / atol 2e-3 with -inf exact on the keyless rows.  With MI355FA_MLA_ERRORS_JSONL=path in the environment
every check appends its measured maxima to that file (profiles/mla_errors.jsonl is such a record)."""
import json
import os

import torch
import torch.nn.functional as F

import fa_oracle as fo
from attn_ref import attention_fp64, visible

F16, BF16 = torch.float16, torch.bfloat16
DT, IDS = [F16, BF16], ["fp16", "bf16"]
D, DV = 576, 512
DEFAULT_SCALE = D ** -0.5
FP16_BOUND, BF16_FLOOR = 1e-3, 4e-3
FAR = 0.1                          # tests/test_gpu_scale.py FAR: relFro of the truth against the default-scale truth, at least


def M():
    import mla_kvcache
    return mla_kvcache.flash_attention_mla_kvcache


def make(B, H, Sq, S, dtype, seed=0, device="cuda"):
    """q [B, H, S_q, 576] and the padded latent cache [B, S, 576]"""
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=device, dtype=torch.float32).to(dtype)
    return r(B, H, Sq, D), r(B, S, D)


def pages_of(L, page):
    return -(-L // page)


def scatter(kv, lens, page, max_pages, seed, alloc=None, row_stride=D, identity=False):
    """The pool [num_pages, page, 576] (rows row_stride elements apart) and the int32 table [B, max_pages] of the padded cache
    kv [B, S, 576], sequence b on its first lens[b] rows (alloc[b] >= lens[b]: the rows it gets pages for).  Every row at or
    past lens[b], every unused page and the padding between rows are NaN; table entries past a sequence's pages are out of
    range.  identity: pages in order, sequence after sequence, instead of a random permutation."""
    B = len(lens)
    used = [pages_of(L, page) for L in (alloc or lens)]
    assert all(n <= max_pages for n in used)
    num_pages = sum(used) + 3
    g = torch.Generator().manual_seed(seed)
    perm = list(range(num_pages)) if identity else torch.randperm(num_pages, generator=g).tolist()
    bad = (-1, num_pages, num_pages + 12345, -(1 << 30), (1 << 31) - 1)
    table = torch.empty(B, max_pages, dtype=torch.int32)
    wide = torch.full((num_pages, page, row_stride), float("nan"), dtype=kv.dtype, device=kv.device)
    pool = wide[..., :D]
    at = 0
    for b in range(B):
        for i in range(max_pages):
            table[b, i] = perm[at + i] if i < used[b] else bad[(b + i) % len(bad)]
        for i in range(pages_of(lens[b], page)):
            n = min(page, lens[b] - i * page)
            pool[perm[at + i], :n] = kv[b, i * page:i * page + n]
        at += used[b]
    return pool, table.to(kv.device)


def truth(q, kv, lens, causal, scale=None):
    """fp64 O [B, H, S_q, 512] and LSE [B, H, S_q]; a sequence without keys, and a row without a visible key: O = 0, LSE = -inf"""
    B, H, Sq, _ = q.shape
    scale = DEFAULT_SCALE if scale is None else scale
    O = torch.zeros(B, H, Sq, DV, dtype=torch.float64, device=q.device)
    LSE = torch.full((B, H, Sq), float("-inf"), dtype=torch.float64, device=q.device)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        k = kv[b:b + 1, None, :L]
        r = attention_fp64(q[b:b + 1], k, k[..., :DV], None, scale, visible(Sq, L, -1, 0 if causal else -1, q.device, L=L))
        O[b], LSE[b] = r["O"][0], r["LSE"][0]
    return O, LSE


def sdpa_level(q, kv, lens, causal, scale, O_ref):
    """per sequence: relFro of PyTorch's own SDPA in q's dtype on the same (q, K, V = K[..., :512]) problem (keyless rows 0)"""
    B, H, Sq, _ = q.shape
    lv = []
    for b, L in enumerate(lens):
        if L == 0:
            lv.append(0.0)
            continue
        k = kv[b, :L][None, None].expand(1, H, L, D)
        o = F.scaled_dot_product_attention(q[b:b + 1], k, k[..., :DV], attn_mask=visible(Sq, L, -1, 0 if causal else -1, q.device, L=L),
                                           scale=DEFAULT_SCALE if scale is None else scale)
        e = fo.rel_fro(O_ref[b:b + 1], torch.nan_to_num(o.float(), nan=0.0))
        lv.append(e if e == e else 0.0)
    return lv


def record(line):
    path = os.environ.get("MI355FA_MLA_ERRORS_JSONL")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def held(tag, q, o, lse, O, LSE, lens, level=None):
    """(o, lse) of a call against a truth() worked out before; level: sdpa_level() of the problem (bf16).  Every output finite
    but LSE = -inf where the truth's is."""
    B, H, Sq, _ = q.shape
    assert o.shape == (B, H, Sq, DV) and o.dtype == q.dtype and lse.shape == (B, H, Sq) and lse.dtype == torch.float32, tag
    assert torch.isfinite(o.float()).all(), (tag, "O is not finite")
    err = [fo.rel_fro(O[b], o[b]) if O[b].abs().max() > 0 else float(o[b].float().abs().max()) for b in range(B)]
    bound = [FP16_BOUND if q.dtype == F16 else max(2 * (level[b] if level else 0.0), BF16_FLOOR) for b in range(B)]
    inf = torch.isinf(LSE)
    lerr = float((lse[~inf].double() - LSE[~inf]).abs().max()) if (~inf).any() else 0.0
    worst = max(range(B), key=lambda b: err[b] / bound[b])
    print("%s: worst sequence %d (L %d) relFro %.3e bound %.3e, LSE max abs err %.3e" % (tag, worst, lens[worst], err[worst], bound[worst], lerr))
    record(dict(id=tag, dtype=IDS[DT.index(q.dtype)], o_relfro_max=max(err), worst_L=lens[worst], worst_relfro=err[worst],
                worst_bound=bound[worst], lse_abs_err_max=lerr))
    assert all(e < bd for e, bd in zip(err, bound)), (tag, "sequence", worst, "L", lens[worst], err[worst], bound[worst])
    assert torch.equal(torch.isneginf(lse), inf), (tag, "LSE = -inf exactly on the rows with no visible key")
    assert not torch.isnan(lse).any() and not torch.isposinf(lse).any(), (tag, "LSE")
    assert torch.allclose(lse[~inf].double(), LSE[~inf], rtol=1e-3, atol=2e-3), (tag, "LSE", lerr)


def same(a, b):
    """(O, LSE) pairs with the same bits"""
    return a[0].shape == b[0].shape and torch.equal(a[0].contiguous().view(torch.int16), b[0].contiguous().view(torch.int16)) and \
        torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
