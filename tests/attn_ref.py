"""The tests' one fp64 attention reference: the masks, the closed form with its gradients, the same attention as eager
differentiable torch ops, and the bf16 level of PyTorch's own SDPA.  tests/test_host_attn_ref.py and the per-feature host
tests check it against torch.autograd and fa_oracle; the GPU tests check the kernels against it.  Not a test module.

Closed form, on whatever device the inputs live (z_h: the sink logit of query head h, natural-log units, not scaled):
    s = scale * Q K^T;  capped: t = tanh(s / cap), s = cap * t;  biased: s = s - slope_h |pos_q(i) - j|;  masked to -inf
    LSE = log(exp(z_h) + sum_j exp(s_j)),  P = exp(s - LSE),  O = P V,  p0 = exp(z_h - LSE)  (the mass the sink took)
    dV = P^T dO,  dS = P (dP - delta) [(1 - t^2)],  dQ = scale dS K,  dK = scale dS^T Q   (dK, dV summed over each group)
    dz_h = -sum_{b, i} p0 delta,   den_h = sum_{b, i} |p0 delta|   (the scale of dz's rounding error: the terms cancel)
pos_q(i) = i for the training calls (top-left aligned), L - S_q + i for decoding (bottom-right aligned, L the key count).
A row with no visible key has O = 0, dQ = 0 and LSE = z_h; without sinks z_h = -inf, which is plain attention.  The
kernels take one transform per call; the arguments compose here (cap, then bias, then sink) because that is the shortest
way to write the function."""
import torch
import torch.nn.functional as F

from fa_oracle import rel_fro


def visible(Sq, Sk, wl, wr, device, L=None):
    """[S_q, S_k] bool: key j visible from query i.  L None: top-left aligned training masks (query i at position i,
    keys < S_k).  L = the sequence's key count: bottom-right aligned decode masks (query i at position L - S_q + i, keys
    < L).  wl / wr = -1: unbounded."""
    i = torch.arange(Sq, device=device)[:, None]
    j = torch.arange(Sk, device=device)[None, :]
    pos = i if L is None else i + (L - Sq)
    vis = (j < (Sk if L is None else L)).repeat(Sq, 1)
    if wl >= 0:
        vis = vis & (j >= pos - wl)
    if wr >= 0:
        vis = vis & (j <= pos + wr)
    return vis


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


def alibi_mask(slopes, B, H, Sq, Sk, vis, dtype, device, L=None):
    """The materialised additive mask an eager / SDPA user builds today: [B|1, H, S_q, S_k] in `dtype`, -slope |d| on the
    visible pairs and -inf elsewhere."""
    d = distance(Sq, Sk, device, L)
    b = bias(slopes.to(device), d, B if slopes.dim() == 2 else 1, H)
    return b.masked_fill(~vis.to(device), -torch.inf).to(dtype)


def attention_fp64(Q, K, V, dO, scale, vis, cap=None, slopes=None, dist=None, sinks=None):
    """O, LSE, P0, SABS (and with dO: dQ, dK, dV, dz, den) in fp64.  Q, dO [B, H, S_q, D], K, V [B, H_kv, S_k, D], vis
    (bool) and dist [S_q, S_k] or [B, 1, S_q, S_k], slopes (H,) or (B, H), sinks (H,); dO None: forward only.  SABS: the
    largest |logit| of a row, the visible transformed scores and a finite sink (the scale of LSE's rounding error)."""
    f = torch.float64
    B, H, Sq, D = Q.shape
    Hkv, Sk = K.shape[1], K.shape[2]
    g = H // Hkv
    q, k, v = Q.to(f), K.to(f).repeat_interleave(g, dim=1), V.to(f).repeat_interleave(g, dim=1)
    z = (torch.full((H,), -torch.inf, dtype=f, device=Q.device) if sinks is None else sinks.detach().to(f)).view(1, H, 1, 1)
    z = z.expand(B, H, Sq, 1)
    s = scale * (q @ k.transpose(-1, -2))
    t = None
    if cap is not None:
        t = torch.tanh(s / cap)
        s = cap * t
    if slopes is not None:
        s = s + bias(slopes, dist, B, H)
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
    zabs = torch.where(torch.isfinite(z), z.abs(), torch.zeros_like(z))[..., 0]
    out = dict(O=O, LSE=lse, P0=P0, SABS=torch.maximum(torch.where(vis, s.abs(), torch.zeros_like(s)).amax(-1), zabs) if Sk > 0 else zabs)
    if dO is None:
        return out
    do = dO.to(f)
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    if t is not None:
        dS = dS * (1 - t * t)
    out["dQ"] = scale * (dS @ k)
    out["dK"] = (scale * (dS.transpose(-1, -2) @ q)).reshape(B, Hkv, g, Sk, D).sum(2)
    out["dV"] = (P.transpose(-1, -2) @ do).reshape(B, Hkv, g, Sk, D).sum(2)
    pd = P0 * delta[..., 0]
    out["dz"] = -pd.sum((0, 2))
    out["den"] = pd.abs().sum((0, 2))
    return out


def attention_eager(Q, K, V, scale, vis, cap=None, slopes=None, dist=None, sinks=None):
    """The same attention as eager differentiable torch ops in Q's dtype (matmul, tanh, bias, mask, softmax, matmul): the
    reference's own check in the host tests and the bf16 yardstick of tests/test_gpu_softcap.py.  The bias is cast to Q's
    dtype before the add; the sink is concatenated to the scores as one more column, the softmax runs over S_k + 1 columns
    and the sink's column is dropped before P @ V.  Differentiable w.r.t. Q, K, V and sinks."""
    B, H, Sq, _ = Q.shape
    g = H // K.shape[1]
    k, v = K.repeat_interleave(g, dim=1), V.repeat_interleave(g, dim=1)
    s = scale * (Q @ k.transpose(-1, -2))
    if cap is not None:
        s = cap * torch.tanh(s / cap)
    if slopes is not None:
        s = s + bias(slopes, dist, B, H).to(Q.dtype)
    s = s.masked_fill(~vis, -torch.inf)
    if sinks is not None:
        s = torch.cat([s, sinks.to(Q.dtype).view(1, H, 1, 1).expand(B, H, Sq, 1)], dim=-1)
    m = s.amax(-1, keepdim=True).detach()
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    P = e / e.sum(-1, keepdim=True).clamp_min(torch.finfo(Q.dtype).tiny)
    return (P if sinks is None else P[..., :-1]) @ v


def sdpa_bf16_level(Q, K, V, dO, vis, gt):
    """relFro of PyTorch's own SDPA in the inputs' dtype (same device, expanded K/V, boolean mask vis) against the fp64 gt,
    per output; a NaN (a fully masked row poisoned a matmul) earns no credit."""
    g = Q.shape[1] // K.shape[1]
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    o = F.scaled_dot_product_attention(q, k.repeat_interleave(g, 1), v.repeat_interleave(g, 1), attn_mask=vis)
    o.backward(dO)
    got = {"O": o.detach(), "dQ": q.grad, "dK": k.grad, "dV": v.grad}
    lv = {n: rel_fro(gt[n], torch.nan_to_num(t.float(), nan=0.0)) for n, t in got.items()}
    return {n: (e if e == e else 0.0) for n, e in lv.items()}
