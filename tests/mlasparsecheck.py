"""Helpers of the sparse MLA decode tests (not a test module).  Sparse attention of query (b, i) is dense attention of ONE query
over its visible selected rows, so truth, level and bounds are tests/mlacheck.py's on the gathered problem: q seen as
[B * S_q, H, 1, 576], the visible entries of indices[b, i] (duplicates kept, in list order) gathered from the padded cache into
[B * S_q, n_visible_max, 576], lens = the visible counts, non-causal."""
import torch

import mlacheck as mc


def S():
    import mla_sparse_kvcache
    return mla_sparse_kvcache.flash_attention_mla_kvcache_sparse


def visible(indices, lens, causal):
    """bool [B, S_q, topk]: 0 <= idx < L_b and, under causal, idx <= L_b - S_q + i"""
    Sq = indices.shape[1]
    L = torch.as_tensor(lens, device=indices.device)[:, None, None]
    pos = L - Sq + torch.arange(Sq, device=indices.device)[None, :, None]
    v = (indices >= 0) & (indices < L)
    return v & (indices <= pos) if causal else v


def gather(q, kv, indices, lens, causal):
    """(q as [B * S_q, H, 1, 576], the gathered rows [B * S_q, n_visible_max, 576], the visible counts)"""
    B, H, Sq, _ = q.shape
    vis, idx = visible(indices, lens, causal).reshape(B * Sq, -1), indices.reshape(B * Sq, -1)
    counts = vis.sum(1).tolist()
    rows = torch.zeros(B * Sq, max(max(counts), 1), mc.D, dtype=kv.dtype, device=kv.device)
    for n, c in enumerate(counts):
        rows[n, :c] = kv[n // Sq, idx[n][vis[n]].long()]
    return q.transpose(1, 2).reshape(B * Sq, H, 1, mc.D), rows, counts


def flat(x, B, Sq):
    """O [B, H, S_q, 512] / LSE [B, H, S_q] of a call as the gathered problem's [B * S_q, H, 1, ...]"""
    return x.transpose(1, 2).reshape(B * Sq, x.shape[1], 1, *x.shape[3:])


def reference(q, kv, indices, lens, causal, scale=None):
    """what held() needs beside a call's result, worked out once per problem"""
    qf, rows, counts = gather(q, kv, indices, lens, causal)
    O, LSE = mc.truth(qf, rows, counts, False, scale)
    level = mc.sdpa_level(qf, rows, counts, False, scale, O) if q.dtype == mc.BF16 else None
    return qf, O, LSE, counts, level


def held(tag, ref, got):
    qf, O, LSE, counts, level = ref
    B, Sq = got[0].shape[0], got[0].shape[2]
    mc.held(tag, qf, flat(got[0], B, Sq), flat(got[1], B, Sq), O, LSE, counts, level)


def draw(lens, Sq, topk, seed, lead=()):
    """int32 [B, S_q, topk] on the CPU: per (b, i) the entries `lead`, then a random permutation of [0, L_b) (under causal some
    of it lies behind the query) with a few duplicates, interleaved with and followed by -1, L, L + 7 and 1 << 30; cut or
    -1-padded to topk.  Entry 0 is a position whenever L_b > 0: lists of one entry are single-key rows."""
    g = torch.Generator().manual_seed(seed)
    out = torch.full((len(lens), Sq, topk), -1, dtype=torch.int32)
    for b, L in enumerate(lens):
        junk = (-1, L, L + 7, 1 << 30)
        for i in range(Sq):
            perm = torch.randperm(L, generator=g).tolist()
            lst = list(lead)
            for n, x in enumerate(perm):
                lst.append(x)
                if n % 5 == 0:
                    lst.append(junk[(n // 5 + b + i) % 4])
                if n % 11 == 3:
                    lst.append(perm[n // 2])
            lst = (lst + list(junk))[:topk]
            out[b, i, :len(lst)] = torch.tensor(lst, dtype=torch.int32)
    return out


# ---- tests/test_gpu_mla_sparse_deep.py: one column group at a time -------------------------------------------------------------
COL_LENS, COL_H, COL_SQ, COL_PAGE, COL_S, COL_TOPK = [65, 300], 16, 2, 64, 320, 70


def column_problem(kind, w, dtype, device="cuda"):
    """(q, kv, indices) of the column test `kind` at column group w, section 2 of tests/test_gpu_mla.py under draw()'s lists of
    70 entries: 'latent' q (x 2) and the cache zero outside latent columns [128 w, + 128); 'rope' q (x 8) and the cache zero
    outside RoPE columns [512 + 16 w, + 16); 'zero' quarter w of the cache zero; 'ropev' q zero on the RoPE columns"""
    seed = {"latent": 140, "rope": 150, "zero": 160, "ropev": 170}[kind] + w
    q0, kv0 = mc.make(len(COL_LENS), COL_H, COL_SQ, COL_S, dtype, seed=seed, device=device)
    idx = draw(COL_LENS, COL_SQ, COL_TOPK, seed=seed + 1).to(device)
    if kind in ("latent", "rope"):
        cols = slice(128 * w, 128 * w + 128) if kind == "latent" else slice(mc.DV + 16 * w, mc.DV + 16 * w + 16)
        q, kv = torch.zeros_like(q0), torch.zeros_like(kv0)
        q[..., cols], kv[..., cols] = q0[..., cols] * (2 if kind == "latent" else 8), kv0[..., cols]
        return q, kv, idx
    if kind == "zero":
        kv0[..., 128 * w:128 * w + 128] = 0
    else:
        q0[..., mc.DV:] = 0
    return q0, kv0, idx


# ---- tests/test_gpu_mla_sparse_deep.py: lists by a per-tile pattern of live and dead tiles ---------------------------------
PATTERNS = ["LDL", "LDDL", "DLL", "DDDL", "LDDDDL", "DLDLDLD", "LDDD"]
DEAD = ["minus-one", "L", "huge", "int-min", "behind", "past-L"]
PAT_L, PAT_PAGE, PAT_MP = 300, 64, 6         # the table reaches 384 rows: 84 positions at or past L and below its reach


def split_range(nt, split, nsplit):
    """csrc/fa_decode_mla_sparse.hip: the tiles [s_beg, s_end) of a split"""
    return nt * split // nsplit, nt * (split + 1) // nsplit


def dead_tile(kind, L, pos, t, reach):
    """32 invisible entries of one kind for a query at position `pos` (tile t of its list).  'behind': the positions in
    (pos, L), repeated; the last query of a sequence has none behind it and gets L.  'past-L': a duplicate-free run of
    positions >= L and below the table's reach (rows the pool holds NaN for, or pages the table has no entry for)."""
    k = torch.arange(32)
    if kind == "minus-one":
        return torch.full((32,), -1)
    if kind == "L":
        return torch.full((32,), L)
    if kind == "huge":
        return torch.full((32,), 1 << 30)
    if kind == "int-min":
        return torch.full((32,), -(1 << 31))
    if kind == "behind":
        return pos + 1 + k % (L - 1 - pos) if pos < L - 1 else torch.full((32,), L)
    assert kind == "past-L" and reach - L >= 32
    return L + (5 * t) % (reach - L - 31) + k


def pattern_lists(L, Sq, pattern, kind, seed, reach):
    """int32 [1, S_q, 32 * len(pattern)] on the CPU, for one sequence of L keys under the causal mask: tile t of every query's
    list is live ('L': random positions of [0, L) -- some behind the query --, every fifth entry one of draw()'s junk values, and
    one position every query sees at a random place) or dead ('D': dead_tile(kind))."""
    g = torch.Generator().manual_seed(seed)
    junk = (-1, L, L + 7, 1 << 30)
    out = torch.empty(1, Sq, 32 * len(pattern), dtype=torch.int64)
    for i in range(Sq):
        for t, c in enumerate(pattern):
            if c == "D":
                e = dead_tile(kind, L, L - Sq + i, t, reach)
            else:
                e = torch.randint(0, L, (32,), generator=g)
                e[::5] = torch.tensor([junk[(n + t + i) % 4] for n in range(7)])
                e[int(torch.randint(0, 32, (1,), generator=g))] = int(torch.randint(0, L - Sq + 1, (1,), generator=g))
            out[0, i, 32 * t:32 * t + 32] = e
    return out.to(torch.int32)
