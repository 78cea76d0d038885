"""Helpers of the packed-variable-length decode tests (tests/test_host_ragged.py, tests/test_gpu_ragged.py; not a test
module): the packed layout of include/mi355fa_ragged.h -- q / o [total_q, H, D] and LSE [H, total_q], sequence b owning
the rows [cu[b], cu[b + 1]) -- to and from the per-sequence tensors [1, H, S_b, D] / [1, H, S_b] the paged call takes and
returns, and the bound on a step's row blocks the launch is sized by.  Works on any device."""
import torch


def cu_of(S, device="cpu"):
    """int32 [B + 1]: the exclusive prefix sums of the query counts S"""
    cu = [0]
    for s in S:
        cu.append(cu[-1] + s)
    return torch.tensor(cu, dtype=torch.int32, device=device)


def pack(per_seq, total_q, fill=float("nan")):
    """per_seq[b]: [1, H, S_b, D] -> [total_q, H, D], sequence after sequence; the rows past the last one hold `fill`"""
    _, H, _, D = per_seq[0].shape
    out = torch.full((total_q, H, D), fill, dtype=per_seq[0].dtype, device=per_seq[0].device)
    at = 0
    for t in per_seq:
        n = t.shape[2]
        out[at:at + n] = t[0].transpose(0, 1)
        at += n
    assert at <= total_q
    return out


def unpack(packed, S):
    """[total_q, H, D] -> [[1, H, S_b, D]]"""
    out, at = [], 0
    for s in S:
        out.append(packed[at:at + s].transpose(0, 1)[None].contiguous())
        at += s
    return out


def unpack_lse(lse, S):
    """[H, total_q] -> [[1, H, S_b]]"""
    out, at = [], 0
    for s in S:
        out.append(lse[:, at:at + s][None].contiguous())
        at += s
    return out


def blocks(S, g):
    """the 32-row blocks of a step: sum_b ceil(g * S_b / 32)"""
    return sum(-(-g * s // 32) for s in S)


def nb_max(g, total_q, B):
    """the header's bound on blocks(S, g) over every split of at most total_q rows into B lengths"""
    return (g * total_q + 31 * B) // 32


def workspace_bytes(n, total_q, B, H, Hkv, D):
    """include/mi355fa_ragged.h: the plan, rounded up to 16 bytes, then the partials of n > 1 splits"""
    plan = (16 + 8 * nb_max(H // Hkv, total_q, B) + 15) // 16 * 16
    return plan + (n * H * total_q * (D + 2) * 4 if n > 1 else 0)
