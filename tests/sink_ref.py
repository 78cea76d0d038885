"""fp64 reference of attention with learned attention sinks (include/mi355fa_sink.h), shared by tests/test_host_sink.py
(which checks it against torch.autograd) and tests/test_gpu_sink.py (which checks the kernels against it).  Not a test
module.

Closed form, on whatever device the inputs live, for the sink logit z_h of query head h (natural-log units, not scaled):
    s = scale * Q K^T (masked to -inf),  LSE = log(exp(z_h) + sum_j exp(s_j)),  P = exp(s - LSE),  O = P V
    p0 = exp(z_h - LSE)   (the mass the sink took; it has no value row)
    dV = P^T dO,  dS = P (dP - delta),  dQ = scale dS K,  dK = scale dS^T Q   (dK, dV summed over each group)
    dz_h = -sum_{b, i} p0 delta,   den_h = sum_{b, i} |p0 delta|   (the scale of dz's rounding error: the terms cancel)
A row with no visible key has O = 0 and LSE = z_h; z_h = -inf is plain attention (such a row then has LSE = -inf).
"""
import torch

from softcap_ref import visible  # noqa: F401  (the same masks)


def sink_fp64(Q, K, V, dO, sinks, scale, vis):
    """O, LSE, P0, SABS (and with dO: dQ, dK, dV, dz, den) in fp64.  Q, dO [B, H, S_q, D], K, V [B, H_kv, S_k, D], sinks (H,) or
    None (the sink-less attention of the same call), vis [S_q, S_k] or [B, 1, S_q, S_k] bool; dO None: forward only."""
    f = torch.float64
    B, H, Sq, D = Q.shape
    Hkv, Sk = K.shape[1], K.shape[2]
    g = H // Hkv
    q, k, v = Q.to(f), K.to(f).repeat_interleave(g, dim=1), V.to(f).repeat_interleave(g, dim=1)
    z = (torch.full((H,), -torch.inf, dtype=f, device=Q.device) if sinks is None else sinks.detach().to(f)).view(1, H, 1, 1)
    z = z.expand(B, H, Sq, 1)
    s = scale * (q @ k.transpose(-1, -2))
    vis = vis.expand(B, H, Sq, Sk)
    sm = s.masked_fill(~vis, -torch.inf)
    m = torch.maximum(sm.amax(-1, keepdim=True) if Sk > 0 else z, z)
    mf = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(sm - mf)
    e0 = torch.exp(z - mf)
    l = e.sum(-1, keepdim=True) + e0
    pos = l > 0
    P = torch.where(pos, e / l.clamp_min(1e-300), torch.zeros_like(e))
    P0 = torch.where(pos, e0 / l.clamp_min(1e-300), torch.zeros_like(e0))[..., 0]
    lse = torch.where(pos[..., 0], mf[..., 0] + torch.log(l[..., 0].clamp_min(1e-300)), torch.full_like(l[..., 0], -torch.inf))
    O = P @ v
    # SABS: the largest |logit| of a row, the visible scores and a finite sink (the scale of LSE's rounding error)
    zabs = torch.where(torch.isfinite(z), z.abs(), torch.zeros_like(z))[..., 0]
    out = dict(O=O, LSE=lse, P0=P0, SABS=torch.maximum(torch.where(vis, s.abs(), torch.zeros_like(s)).amax(-1), zabs) if Sk > 0 else zabs)
    if dO is None:
        return out
    do = dO.to(f)
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    out["dQ"] = scale * (dS @ k)
    out["dK"] = (scale * (dS.transpose(-1, -2) @ q)).reshape(B, Hkv, g, Sk, D).sum(2)
    out["dV"] = (P.transpose(-1, -2) @ do).reshape(B, Hkv, g, Sk, D).sum(2)
    t = P0 * delta[..., 0]
    out["dz"] = -t.sum((0, 2))
    out["den"] = t.abs().sum((0, 2))
    return out


def sink_eager(Q, K, V, sinks, scale, vis):
    """The same attention as eager differentiable torch ops in Q's dtype: the sink is concatenated to the scores as one more
    column, the softmax runs over S_k + 1 columns and the sink's column is dropped before P @ V.  The reference's own check
    (test_host_sink.py) and the eager baseline of tools/sink_bench.py.  Differentiable w.r.t. Q, K, V and sinks."""
    B, H, Sq, _ = Q.shape
    g = H // K.shape[1]
    k, v = K.repeat_interleave(g, dim=1), V.repeat_interleave(g, dim=1)
    s = scale * (Q @ k.transpose(-1, -2))
    s = s.masked_fill(~vis, -torch.inf)
    sz = torch.cat([s, sinks.to(Q.dtype).view(1, H, 1, 1).expand(B, H, Sq, 1)], dim=-1)
    m = sz.amax(-1, keepdim=True).detach()
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(sz - m)
    P = e / e.sum(-1, keepdim=True).clamp_min(torch.finfo(Q.dtype).tiny)
    return P[..., :-1] @ v
