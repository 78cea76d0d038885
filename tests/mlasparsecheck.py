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


def reference(q, kv, indices, lens, causal):
    """what held() needs beside a call's result, worked out once per problem"""
    qf, rows, counts = gather(q, kv, indices, lens, causal)
    O, LSE = mc.truth(qf, rows, counts, False)
    level = mc.sdpa_level(qf, rows, counts, False, None, O) if q.dtype == mc.BF16 else None
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
