"""Helpers of the soft-capped quantised-cache decode tests (tests/test_gpu_kvcache_quant_softcap.py,
tests/test_gpu_ragged_quant_softcap.py, tests/test_gpu_race_decode_quant_softcap.py; not a test module): one cache object for
the three formats (per-tensor e4m3, per-token e4m3, MXFP4) built by each format's own quantiser, its fp64 dequantisation by the
format's own module, the fp64 truth with the cap on the dequantised cache (tests/attn_ref.py), the per-(sequence, head) check,
pools under a permuted table, and one adapter per geometry for the capped call and for the format's plain call.

Bounds, none of them new: O per (sequence, head) relFro 1e-3 fp16 / 8e-3 bf16 (fp8tokencheck.BOUND = test_gpu_softcap.REL); LSE row
by row by test_gpu_kvcache.check_lse (what the quantised tests use) and by test_gpu_softcap's LSE_BOUND a + u * max |logit| (what
the soft-capped decode test uses); the cap must matter by test_gpu_softcap.CAP_MATTERS on the sequences with at least 300 keys."""
import torch

import attn_ref as ar
import fa_oracle as fo
import fp8tokencheck as tk
import pagedcheck as pc
import raggedcheck as rg
from fp8tokencheck import BF16, BOUND, DT, F16, F8, IDS   # noqa: F401
from test_gpu_kvcache import check_lse, window_of
from test_gpu_softcap import BOUNDS, CAP_MATTERS, REL, _amp

assert BOUND == REL
LSE_BOUND = BOUNDS["LSE_BOUND"]
FORMATS = ["e4m3", "token", "fp4"]
MATTERS_FROM = 300      # keys: below, the cap moves O too little to tell (the L = 2 sequence: < 0.05)


def Q():
    import quant_softcap_kvcache as Q
    return Q


def _M():
    import My_FlashAttention_optimized as M
    return M


def _F4():
    import fp4_kvcache as F
    return F


class Cache:
    """the tensors of a cache of one format, padded [B, H_kv, S, .] or pools [num_pages, H_kv, page, .]: k, v, the scales ks / vs
    (token: fp32 [.., S]; fp4: bytes [.., S, D / 32]; e4m3: None) and the descales kd / vd (e4m3 only, or None)"""

    def __init__(self, fmt, k, v, ks=None, vs=None, kd=None, vd=None):
        self.fmt, self.k, self.v, self.ks, self.vs, self.kd, self.vd = fmt, k, v, ks, vs, kd, vd

    def kw(self):
        """the format's keywords of the capped calls"""
        return dict(k_scale=self.ks, v_scale=self.vs) if self.fmt != "e4m3" else dict(k_descale=self.kd, v_descale=self.vd)

    def tensors(self):
        return [t for t in (self.k, self.v, self.ks, self.vs) if t is not None]

    def clone(self):
        c = lambda t: None if t is None else t.clone()
        return Cache(self.fmt, c(self.k), c(self.v), c(self.ks), c(self.vs), self.kd, self.vd)

    def like(self, tensors):
        t = list(tensors) + [None, None]
        return Cache(self.fmt, t[0], t[1], t[2], t[3], self.kd, self.vd)

    def for_seq(self, b):
        """the same pools for a call on sequence b alone: its row of per-(B, H_kv) descales"""
        d = lambda t: t if t is None or t.dim() == 1 else t[b:b + 1].contiguous()
        return Cache(self.fmt, self.k, self.v, self.ks, self.vs, d(self.kd), d(self.vd))

    def rows(self, b, L):
        """sequence b alone, its first L rows"""
        s = lambda t: None if t is None else t[b:b + 1, :, :L].contiguous()
        d = lambda t: None if t is None or t.dim() == 1 else t[b:b + 1].contiguous()
        return Cache(self.fmt, s(self.k), s(self.v), s(self.ks), s(self.vs), d(self.kd), d(self.vd))

    def deq64(self):
        """K, V in fp64 by the format's own dequantiser"""
        if self.fmt == "fp4":
            return tuple(_F4().dequantize_kv_mxfp4(x, s, torch.float64) for x, s in ((self.k, self.ks), (self.v, self.vs)))
        if self.fmt == "token":
            return tk.deq64(self.k, self.ks), tk.deq64(self.v, self.vs)
        B, Hkv = self.k.shape[:2]
        d = lambda t: 1.0 if t is None else (t.double().view(1, Hkv, 1, 1) if t.dim() == 1 else t.double().view(B, Hkv, 1, 1))
        return self.k.double() * d(self.kd), self.v.double() * d(self.vd)


def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def quantise(fmt, k, v, descale_mul=1.0, per_head=False):
    """K, V [B, H_kv, S, D] (fp32) -> the cache the format's own quantiser gives.  e4m3: the natural per-(B, H_kv) descales amax /
    448 times descale_mul, or (per_head) one (H_kv,) vector of them"""
    if fmt == "fp4":
        (k4, ks), (v4, vs) = _F4().quantize_kv_mxfp4(k), _F4().quantize_kv_mxfp4(v)
        return Cache(fmt, k4, v4, ks, vs)
    if fmt == "token":
        (k8, ks), (v8, vs) = tk.T().quantize_kv_fp8_per_token(k), tk.T().quantize_kv_fp8_per_token(v)
        return Cache(fmt, k8, v8, ks, vs)
    k8, kd = _M().quantize_kv_fp8(k)
    v8, vd = _M().quantize_kv_fp8(v)
    if per_head:
        kd, vd = kd.amax(0).contiguous(), vd.amax(0).contiguous()
        k8, v8 = _M().quantize_kv_fp8(k, kd)[0], _M().quantize_kv_fp8(v, vd)[0]
    assert kd.unique().numel() == kd.numel() and float(kd.max()) < 0.05        # distinct values, about 0.01
    return Cache(fmt, k8, v8, kd=(kd * descale_mul).contiguous(), vd=vd)


def make(fmt, B, H, Hkv, Sq, Sc, D, dtype, cap, scale=None, seed=0, **kw):
    """q with the amplitude that puts the score standard deviation at 0.6 x cap (test_gpu_softcap._amp), and the cache of K, V
    ~ N(0, 1) in the format"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = D ** -0.5 if scale is None else scale
    q = (torch.randn(B, H, Sq, D, generator=g, device="cuda") * _amp(cap, scale, D)).to(dtype)
    k, v = (torch.randn(B, Hkv, Sc, D, generator=g, device="cuda") for _ in range(2))
    return q, quantise(fmt, k, v, **kw)


def new_rows(B, Hkv, Snew, D, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return tuple(torch.randn(B, Hkv, Snew, D, generator=g, device="cuda").to(dtype) for _ in range(2))


def truth(q, cache, lens, cap, is_causal=False, window=(-1, -1), scale=None):
    """fp64 attention with the cap on the fp64 dequantised cache, per sequence on its first L_b rows: dict O [B, H, S_q, D], LSE
    and SABS [B, H, S_q], UNC (the uncapped O on the same cache)"""
    B, H, Sq, D = q.shape
    scale = D ** -0.5 if scale is None else scale
    wl, wr = window_of(is_causal, window)
    K, V = cache.deq64()
    out = dict(O=torch.zeros(B, H, Sq, D, dtype=torch.float64, device=q.device), UNC=torch.zeros(B, H, Sq, D, dtype=torch.float64, device=q.device),
               LSE=torch.full((B, H, Sq), float("-inf"), dtype=torch.float64, device=q.device),
               SABS=torch.zeros(B, H, Sq, dtype=torch.float64, device=q.device))
    for b, L in enumerate(lens):
        if L == 0:
            continue
        kb, vb = (x[b:b + 1, :, :L] if x.shape[0] == B else x[:, :, :L] for x in (K, V))
        vis = ar.visible(Sq, L, wl, wr, q.device, L=L)
        r = ar.attention_fp64(q[b:b + 1], kb, vb, None, scale, vis, cap=cap)
        out["O"][b], out["LSE"][b], out["SABS"][b] = r["O"][0], r["LSE"][0], r["SABS"][0]
        out["UNC"][b] = ar.attention_fp64(q[b:b + 1], kb, vb, None, scale, vis)["O"][0]
    return out


def check(tag, q, o, lse, gt, lens, matters=True):
    """O per (sequence, head) and LSE row by row against `gt` (truth()); the cap is applied (sequences of >= MATTERS_FROM keys)"""
    B, H, Sq, D = q.shape
    assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == (B, H, Sq) and lse.dtype == torch.float32
    err = fo.block_errors(gt["O"], o, block=Sq)[..., 0]                          # [B, H]
    at = tuple(int(x) for x in torch.unravel_index(err.argmax(), err.shape))
    fin = torch.isfinite(gt["LSE"])
    lerr = (lse.double() - gt["LSE"]).abs()[fin]
    print("%s: worst (b, h) %s relFro %.3e bound %.0e; LSE err %.2e" % (tag, at, err[at].item(), BOUND[q.dtype],
                                                                         lerr.max().item() if lerr.numel() else 0.0))
    assert (err < BOUND[q.dtype]).all(), (tag, "(b, h)", at, err[at].item(), lens[at[0]])
    check_lse(lse, gt["LSE"])
    a, u = LSE_BOUND[q.dtype]
    assert (lerr <= a + u * gt["SABS"][fin]).all(), (tag, lerr.max().item())
    assert (o[(gt["O"] == 0).all(-1)] == 0).all(), tag
    if matters:
        for b, L in enumerate(lens):
            if L >= MATTERS_FROM:
                far = fo.rel_fro(gt["UNC"][b], o[b])
                assert far >= CAP_MATTERS, (tag, "the cap is not applied", b, L, far)


def same(a, b):
    return tk.same(a, b)


# ---------------------------------------------------------------- pools
def scatter(cache, lens, page, max_pages, seed=5, alloc=None, spare=3):
    """(pools as a Cache, table): every tensor of the cache under one permuted table (NaN / poison elsewhere)"""
    n = sum(pc.pages_of(L, page) for L in (alloc or lens)) + spare
    if cache.fmt == "token":
        kp, vp, ksp, vsp, table = tk.scatter(cache.k, cache.v, cache.ks, cache.vs, lens, page, n, max_pages, seed, alloc=alloc)
        return cache.like((kp, vp, ksp, vsp)), table
    pools, table = pc.scatter((cache.k, cache.v), lens, page, n, max_pages, seed, alloc=alloc)
    if cache.fmt == "fp4":   # the scale bytes [.., D / 32] through the same table
        pools += pc.scatter((cache.ks, cache.vs), lens, page, n, max_pages, seed, table=table.cpu(), alloc=alloc)[0]
    return cache.like(pools), table


def gather(pools, table):
    """the padded Cache [B, H_kv, max_pages * page, .] the pools and the table describe"""
    out = []
    for t in pools.tensors():
        out.append(tk.gather_scales(t, table) if t.dim() == 3 else pc.gather(t, table))
    return pools.like(out)


# ---------------------------------------------------------------- the calls
def padded(q, c, sl, cap, **kw):
    return Q().flash_attention_kvcache_quant_softcap(q, c.k, c.v, sl, cap, return_lse=True, **c.kw(), **kw)


def paged(q, c, sl, table, cap, **kw):
    return Q().flash_attention_kvcache_quant_softcap_paged(q, c.k, c.v, sl, table, cap, return_lse=True, **c.kw(), **kw)


def packed(qs, c, sl, table, cap, k_new=None, v_new=None, total_q=None, **kw):
    """qs[b]: [1, H, S_b, D] -> the per-sequence (O [1, H, S_b, D], LSE [1, H, S_b]) of one packed call; k_new / v_new: per
    sequence [1, H_kv, S_b, D]; total_q: padding rows past the last sequence"""
    S = [t.shape[2] for t in qs]
    total = total_q or sum(S)
    pk = lambda ts: None if ts is None else rg.pack(ts, total, fill=0.0)
    o, lse = Q().flash_attention_kvcache_quant_softcap_ragged(rg.pack(qs, total, fill=0.0), c.k, c.v, rg.cu_of(S, device="cuda"), sl,
                                                              table, cap, k_new=pk(k_new), v_new=pk(v_new), return_lse=True,
                                                              **c.kw(), **kw)
    return list(zip(rg.unpack(o, S), rg.unpack_lse(lse, S)))


def plain_padded(q, c, sl, **kw):
    """the uncapped padded call of the format (its append writes the reference bytes)"""
    if c.fmt == "fp4":
        return _F4().flash_attention_kvcache_fp4(q, c.k, c.v, c.ks, c.vs, sl, return_lse=True, **kw)
    if c.fmt == "token":
        return tk.padded(q, c.k, c.v, c.ks, c.vs, sl, **kw)
    return _M().flash_attention_kvcache_fp8(q, c.k, c.v, sl, k_descale=c.kd, v_descale=c.vd, return_lse=True, **kw)


def plain_paged(q, c, sl, table, **kw):
    if c.fmt == "fp4":
        return _F4().flash_attention_kvcache_fp4_paged(q, c.k, c.v, c.ks, c.vs, sl, table, return_lse=True, **kw)
    if c.fmt == "token":
        return tk.paged(q, c.k, c.v, c.ks, c.vs, sl, table, **kw)
    import paged_kvcache as P
    return P.flash_attention_kvcache_paged(q, c.k, c.v, sl, table, k_descale=c.kd, v_descale=c.vd, return_lse=True, **kw)


def plain_packed(qp, c, cu, sl, table, **kw):
    """the uncapped packed call of the format on packed tensors"""
    if c.fmt == "fp4":
        import fp4_ragged_kvcache as R4
        return R4.flash_attention_kvcache_fp4_ragged(qp, c.k, c.v, c.ks, c.vs, cu, sl, table, return_lse=True, **kw)
    if c.fmt == "token":
        return tk.T().flash_attention_kvcache_fp8_token_ragged(qp, c.k, c.v, c.ks, c.vs, cu, sl, table, return_lse=True, **kw)
    import ragged_kvcache as R
    return R.flash_attention_kvcache_ragged(qp, c.k, c.v, cu, sl, table, k_descale=c.kd, v_descale=c.vd, return_lse=True, **kw)


def sl_of(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")
