"""fp64 reference of logit soft-capped attention (include/mi355fa_softcap.h), shared by tests/test_host_softcap.py (which
checks it against torch.autograd) and tests/test_gpu_softcap.py (which checks the kernels against it).  Not a test module.

Closed form, on whatever device the inputs live:
    t = tanh(scale * Q K^T / cap),  u = cap * t  (masked to -inf),  P = exp(u - LSE),  O = P V
    dV = P^T dO,  dS = P (dP - delta) (1 - t^2),  dQ = scale dS K,  dK = scale dS^T Q   (dK, dV summed over each group)
"""
import torch


def visible(Sq, Sk, wl, wr, device, L=None):
    """[S_q, S_k] bool: key j visible from query i.  L None: top-left aligned training masks (query i at position i,
    keys < S_k).  L = the sequence's key count: bottom-right aligned decode masks (query i at position L - S_q + i, keys
    < L).  wl / wr = -1: unbounded."""
    i = torch.arange(Sq, device=device)[:, None]
    j = torch.arange(Sk, device=device)[None, :]
    pos = i if L is None else i + (L - Sq)
    vis = j < (Sk if L is None else L)
    if wl >= 0:
        vis = vis & (j >= pos - wl)
    if wr >= 0:
        vis = vis & (j <= pos + wr)
    return vis


def softcap_fp64(Q, K, V, dO, cap, scale, vis):
    """O, LSE, dQ, dK, dV (and SABS, max |u| of a row's visible scores) in fp64.  Q, dO [B, H, S_q, D], K, V
    [B, H_kv, S_k, D], vis [S_q, S_k] or [B, 1, S_q, S_k] bool; dO None: forward only."""
    f = torch.float64
    B, H, Sq, D = Q.shape
    Hkv = K.shape[1]
    g = H // Hkv
    q, k, v = Q.to(f), K.to(f).repeat_interleave(g, dim=1), V.to(f).repeat_interleave(g, dim=1)
    if cap is None:   # the uncapped attention of the same call
        t = None
        u = scale * (q @ k.transpose(-1, -2))
    else:
        t = torch.tanh(scale * (q @ k.transpose(-1, -2)) / cap)
        u = cap * t
    vis = vis.expand(B, H, Sq, K.shape[2])
    um = u.masked_fill(~vis, -torch.inf)
    m = um.amax(-1, keepdim=True)
    mf = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(um - mf)
    l = e.sum(-1, keepdim=True)
    P = torch.where(l > 0, e / l.clamp_min(1e-300), torch.zeros_like(e))
    lse = torch.where(l[..., 0] > 0, mf[..., 0] + torch.log(l[..., 0].clamp_min(1e-300)), torch.full_like(l[..., 0], -torch.inf))
    O = P @ v
    out = dict(O=O, LSE=lse, SABS=torch.where(vis, u.abs(), torch.zeros_like(u)).amax(-1))
    if dO is None:
        return out
    do = dO.to(f)
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    if t is not None:
        dS = dS * (1 - t * t)
    out["dQ"] = scale * (dS @ k)
    out["dK"] = (scale * (dS.transpose(-1, -2) @ q)).reshape(B, Hkv, g, K.shape[2], D).sum(2)
    out["dV"] = (P.transpose(-1, -2) @ do).reshape(B, Hkv, g, K.shape[2], D).sum(2)
    return out


def softcap_eager(Q, K, V, cap, scale, vis):
    """The same attention as eager differentiable torch ops (matmul, tanh, mask, softmax, matmul), in Q's dtype: the
    reference's own check (test_host_softcap.py) and the eager baseline of tools/softcap_bench.py."""
    g = Q.shape[1] // K.shape[1]
    k, v = K.repeat_interleave(g, dim=1), V.repeat_interleave(g, dim=1)
    s = scale * (Q @ k.transpose(-1, -2))
    u = cap * torch.tanh(s / cap)
    u = u.masked_fill(~vis, -torch.inf)
    m = u.amax(-1, keepdim=True).detach()
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(u - m)
    P = e / e.sum(-1, keepdim=True).clamp_min(torch.finfo(Q.dtype).tiny)
    return P @ v
