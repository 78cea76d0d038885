"""Helpers of the packed MLA decode tests (tests/test_gpu_mla_ragged.py, tests/test_gpu_race_mla_ragged.py,
tests/test_host_mla_ragged.py; not a test module), over tests/mlacheck.py: a step of sequences with their own query counts is
packed into the call's tensors, and the call's results are unpacked into per-sequence problems of mlacheck's shape.

Truth: mc.truth per sequence on (the q rows of b, its first L_b cache rows), L_b = the fill before the step, plus S_b with an
append.  Bounds: mlacheck's own, per sequence (mc.held) -- fp16 relFro < 1e-3; bf16 < max(2 x SDPA's error on the same problem,
4e-3); LSE rtol 1e-3 / atol 2e-3 with -inf exact on keyless rows.  MI355FA_MLA_ERRORS_JSONL records as there
(profiles/mla_ragged_errors.jsonl is such a record)."""
import torch

import mlacheck as mc
from mlacheck import D, DV

# (S_b, cache length before the step): empty sequences first, in the middle and last, a keyless sequence with a query (no
# append), drafts of 2 .. 5 rows around a tile edge, one prefill chunk of many row blocks, a decode row deep in its 9th tile
BATCH = [(0, 100), (1, 0), (1, 31), (2, 32), (3, 33), (5, 300), (40, 130), (0, 0), (1, 257)]


def R():
    import mla_ragged_kvcache
    return mla_ragged_kvcache.flash_attention_mla_kvcache_ragged


class Step:
    """One packed step.  seqs: [(S_b, fill_b)].  q[b]: [1, H, S_b, 576]; kv [B, S_pad, 576]: every sequence's cache AFTER the
    step (with append its rows [fill_b, fill_b + S_b) are the new rows); Ls: the keys sequence b attends to.  Packed: qp
    [total_q, H, 576], new [total_q, 576], cu (B + 1 entries); pad: packed rows allocated past cu[B]."""

    def __init__(self, seqs, H, dtype, append, seed=0, device="cuda", pad=0, S_pad=None):
        self.seqs, self.H, self.dtype, self.append, self.device = list(seqs), H, dtype, append, device
        self.S = [s for s, _ in seqs]
        self.fills = [f for _, f in seqs]
        self.Ls = [f + (s if append else 0) for s, f in seqs]
        self.B = len(seqs)
        self.rows = sum(self.S)
        self.total_q = self.rows + pad
        self.cu_list = [sum(self.S[:b]) for b in range(self.B + 1)]
        S_pad = S_pad or -(-max(self.Ls + [1]) // 128) * 128
        g = torch.Generator(device=device).manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g, device=device, dtype=torch.float32).to(dtype)
        self.kv = r(self.B, S_pad, D)
        self.q = [r(1, H, s, D) for s in self.S]
        self.qp = pack_rows(self.q, self.total_q, float("nan"))
        self.new = torch.full((self.total_q, D), float("nan"), dtype=dtype, device=device)
        for b, (s, f) in enumerate(seqs):
            self.new[self.cu_list[b]:self.cu_list[b + 1]] = self.kv[b, f:f + s]
        self.cu = torch.tensor(self.cu_list, dtype=torch.int32, device=device)
        self.sl = torch.tensor(self.fills, dtype=torch.int32, device=device)

    def pools(self, page, max_pages, seed, row_stride=D):
        """(the pool before the step, the table, the pool an append must leave): mc.scatter under one permutation; every
        sequence has the pages of its L_b rows"""
        before, table = mc.scatter(self.kv, self.fills, page, max_pages, seed, alloc=self.Ls, row_stride=row_stride)
        after, t2 = mc.scatter(self.kv, self.Ls, page, max_pages, seed, row_stride=row_stride)
        assert torch.equal(table, t2)
        return before, table, after

    def truth(self, causal, scale=None, level=False):
        """per sequence (O [1, H, S_b, 512], LSE [1, H, S_b], SDPA's level or None); None for a sequence without rows"""
        out = []
        for b in range(self.B):
            if self.S[b] == 0:
                out.append(None)
                continue
            O, LSE = mc.truth(self.q[b], self.kv[b:b + 1], [self.Ls[b]], causal, scale)
            lv = mc.sdpa_level(self.q[b], self.kv[b:b + 1], [self.Ls[b]], causal, scale, O) if level and self.dtype == mc.BF16 else None
            out.append((O, LSE, lv))
        return out


def pack_rows(per_seq, total, fill):
    """[1, H, S_b, W] per sequence -> [total, H, W], rows past the last sequence = fill"""
    H, W = per_seq[0].shape[1], per_seq[0].shape[3]
    out = torch.full((total, H, W), fill, dtype=per_seq[0].dtype, device=per_seq[0].device)
    at = 0
    for x in per_seq:
        out[at:at + x.shape[2]] = x[0].transpose(0, 1)
        at += x.shape[2]
    return out


def pack_lse(per_seq, total, fill):
    """[1, H, S_b] per sequence -> [H, total]"""
    H = per_seq[0].shape[1]
    out = torch.full((H, total), fill, dtype=per_seq[0].dtype, device=per_seq[0].device)
    at = 0
    for x in per_seq:
        out[:, at:at + x.shape[2]] = x[0]
        at += x.shape[2]
    return out


def unpack(o, lse, cu_list, b):
    """sequence b of a packed result as mlacheck takes it: O [1, H, S_b, 512], LSE [1, H, S_b]"""
    a, e = cu_list[b], cu_list[b + 1]
    return o[a:e].transpose(0, 1)[None], lse[:, a:e][None]


def held(tag, step, o, lse, truths):
    """a packed (o, lse) against step.truth(): mc.held per sequence"""
    assert o.shape == (step.total_q, step.H, DV) and o.dtype == step.dtype, tag
    assert lse.shape == (step.H, step.total_q) and lse.dtype == torch.float32, tag
    for b, t in enumerate(truths):
        if t is None:
            continue
        ob, lb = unpack(o, lse, step.cu_list, b)
        mc.held("%s seq%d S%d L%d" % (tag, b, step.S[b], step.Ls[b]), step.q[b], ob, lb, t[0], t[1], [step.Ls[b]], t[2])


def same_rows(o, lse, cu_list, b, ref):
    """sequence b's rows of a packed result have the bits of ref = (O [1, H, S_b, 512], LSE [1, H, S_b])"""
    return mc.same(tuple(x.contiguous() for x in unpack(o, lse, cu_list, b)), (ref[0].contiguous(), ref[1].contiguous()))
