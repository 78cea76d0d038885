"""fp64 reference of attention with an ALiBi bias (include/mi355fa_alibi.h), shared by tests/test_host_alibi.py (which
checks it against torch.autograd) and tests/test_gpu_alibi.py (which checks the kernels against it).  Not a test module.

Closed form, on whatever device the inputs live:
    s = scale * Q K^T - slope_h |pos_q(i) - j|  (masked to -inf),  P = exp(s - LSE),  O = P V
    dV = P^T dO,  dS = P (dP - delta),  dQ = scale dS K,  dK = scale dS^T Q   (dK, dV summed over each group)
pos_q(i) = i for the training calls (top-left aligned), L - S_q + i for decoding (bottom-right aligned, L the key count).
"""
import torch

from softcap_ref import visible  # noqa: F401  (the same masks)


def distance(Sq, Sk, device, L=None):
    """[S_q, S_k] fp64 |pos_q(i) - j|: pos_q(i) = i (L None, training) or L - S_q + i (decoding)."""
    i = torch.arange(Sq, device=device, dtype=torch.float64)[:, None]
    j = torch.arange(Sk, device=device, dtype=torch.float64)[None, :]
    return ((i if L is None else i + (L - Sq)) - j).abs()


def bias(slopes, dist, B, H):
    """[B, H, S_q, S_k] fp64 -slope |d| for slopes (H,) or (B, H) and dist [S_q, S_k] or [B, 1, S_q, S_k]."""
    s = slopes.to(torch.float64)
    s = s.view(1, H, 1, 1) if s.dim() == 1 else s.view(B, H, 1, 1)
    return -s * dist


def alibi_fp64(Q, K, V, dO, slopes, scale, vis, dist):
    """O, LSE, dQ, dK, dV (and SABS, max |s| of a row's visible biased scores) in fp64.  Q, dO [B, H, S_q, D], K, V [B, H_kv, S_k, D], slopes (H,) / (B, H) or None (the
    unbiased attention of the same call), vis and dist [S_q, S_k] or [B, 1, S_q, S_k]; dO None: forward only."""
    f = torch.float64
    B, H, Sq, D = Q.shape
    Hkv, Sk = K.shape[1], K.shape[2]
    g = H // Hkv
    q, k, v = Q.to(f), K.to(f).repeat_interleave(g, dim=1), V.to(f).repeat_interleave(g, dim=1)
    s = scale * (q @ k.transpose(-1, -2))
    if slopes is not None:
        s = s + bias(slopes, dist, B, H)
    vis = vis.expand(B, H, Sq, Sk)
    sm = s.masked_fill(~vis, -torch.inf)
    m = sm.amax(-1, keepdim=True)
    mf = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(sm - mf)
    l = e.sum(-1, keepdim=True)
    P = torch.where(l > 0, e / l.clamp_min(1e-300), torch.zeros_like(e))
    lse = torch.where(l[..., 0] > 0, mf[..., 0] + torch.log(l[..., 0].clamp_min(1e-300)), torch.full_like(l[..., 0], -torch.inf))
    O = P @ v
    out = dict(O=O, LSE=lse, SABS=torch.where(vis, s.abs(), torch.zeros_like(s)).amax(-1))
    if dO is None:
        return out
    do = dO.to(f)
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    out["dQ"] = scale * (dS @ k)
    out["dK"] = (scale * (dS.transpose(-1, -2) @ q)).reshape(B, Hkv, g, Sk, D).sum(2)
    out["dV"] = (P.transpose(-1, -2) @ do).reshape(B, Hkv, g, Sk, D).sum(2)
    return out


def alibi_mask(slopes, B, H, Sq, Sk, vis, dtype, device, L=None):
    """The materialised additive mask an eager / SDPA user builds today: [B|1, H, S_q, S_k] in `dtype`, -slope |d| on the
    visible pairs and -inf elsewhere."""
    d = distance(Sq, Sk, device, L)
    b = bias(slopes.to(device), d, B if slopes.dim() == 2 else 1, H)
    return b.masked_fill(~vis.to(device), -torch.inf).to(dtype)


def alibi_eager(Q, K, V, slopes, scale, vis, L=None):
    """The same attention as eager differentiable torch ops (matmul, bias, mask, softmax, matmul), in Q's dtype: the
    reference's own check (test_host_alibi.py)."""
    B, H, Sq, _ = Q.shape
    g = H // K.shape[1]
    k, v = K.repeat_interleave(g, dim=1), V.repeat_interleave(g, dim=1)
    s = scale * (Q @ k.transpose(-1, -2)) + bias(slopes, distance(Sq, K.shape[2], Q.device, L), B, H).to(Q.dtype)
    s = s.masked_fill(~vis, -torch.inf)
    m = s.amax(-1, keepdim=True).detach()
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    P = e / e.sum(-1, keepdim=True).clamp_min(torch.finfo(Q.dtype).tiny)
    return P @ v
