"""Helpers of the per-token-scaled e4m3 decode tests (tests/test_gpu_kvcache_fp8_token.py, tests/test_gpu_ragged_fp8_token.py,
tests/test_gpu_race_decode_fp8_token.py, tests/test_gpu_fp8_token_deep.py; not a test module): the caches and their row scales, the fp64 truth on the fp64
dequantised cache, the per-(sequence, head) check with the bounds of tests/test_gpu_kvcache_fp8.py's per-head test, the pools
of a paged call, and one adapter per geometry."""
import torch

import fa_oracle as fo
import pagedcheck as pc
import raggedcheck as rg
from test_gpu_kvcache import check_lse, ref_fp64, window_of

F16, BF16 = torch.float16, torch.bfloat16
DT, IDS = [F16, BF16], ["fp16", "bf16"]
F8 = torch.float8_e4m3fn
# the per-(sequence, head) bounds of tests/test_gpu_kvcache_fp8.py::test_per_head_against_fp64_at_long_ragged_fill_levels
# (a literal inside that test: relative Frobenius 1e-3 fp16, 8e-3 bf16); LSE is that file's check_lse, imported above
BOUND = {F16: 1e-3, BF16: 8e-3}


def T():
    import fp8_token_kvcache as T
    return T


def rows(shape, lo, hi, g):
    """fp32 rows [..., D] whose amax is 2^e, e uniform in [lo, hi] per row (not an integer: the scales are no powers of two)"""
    x = torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32)
    e = torch.rand(*shape[:-1], 1, generator=g, device="cuda") * (hi - lo) + lo
    return x / x.abs().amax(dim=-1, keepdim=True) * torch.exp2(e)


def make(B, H, Hkv, Sq, Sc, D, dtype, seed=0, span=(-6.0, 6.0), v_span=None, k_span=None):
    """q, the caches and scales quantize_kv_fp8_per_token gives on rows whose amax spans 2^-6 .. 2^6 within every sequence.
    v_span[b]: another span for sequence b's V rows.  k_span: another span for the K rows (None: `span`, the same draws)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, H, Sq, D, generator=g, device="cuda", dtype=torch.float32).to(dtype)
    k, v = rows((B, Hkv, Sc, D), *(k_span or span), g), rows((B, Hkv, Sc, D), *span, g)
    for b, s in (v_span or {}).items():
        v[b] = rows((Hkv, Sc, D), *s, g)
    (k8, ks), (v8, vs) = T().quantize_kv_fp8_per_token(k), T().quantize_kv_fp8_per_token(v)
    assert ks.shape == (B, Hkv, Sc) and ks.dtype == torch.float32 and (torch.frexp(ks)[0] != 0.5).float().mean() > 0.9
    return q, k8, v8, ks, vs


def deq64(x8, s):
    """float(byte) * scale in fp64"""
    return x8.double() * s.double().unsqueeze(-1)


def truth(q, K, V, lens, is_causal=False, window=(-1, -1), scale=None, sinks=None):
    """fp64 attention of q over the fp64 cache K, V [B, H_kv, S, D], sequence b on its first lens[b] rows: O [B, H, S_q, D] and
    LSE [B, H, S_q].  A row without a key has O = 0 and LSE = -inf, or the sink's logit."""
    H = q.shape[1]
    wl, wr = window_of(is_causal, window)
    O, LSE = ref_fp64(q, K, V, lens, wl, wr, scale)
    if sinks is not None:   # one more key with logit sinks[h] and no value row
        z = sinks.double().view(1, H, 1)
        new = torch.logaddexp(LSE, z.expand_as(LSE))
        O = O * torch.exp(LSE - new).nan_to_num(0.0).unsqueeze(-1)
        LSE = new
    return O, LSE


def check(tag, q, o, lse, k8, v8, ks, vs, lens, is_causal=False, window=(-1, -1), scale=None, sinks=None):
    """O per (sequence, head) and LSE row by row against fp64 attention on the fp64 dequantised cache"""
    return held(tag, q, o, lse, *truth(q, deq64(k8, ks), deq64(v8, vs), lens, is_causal, window, scale, sinks), lens)


def held(tag, q, o, lse, O, LSE, lens):
    """check() against a truth() worked out before (one truth serves every split count)"""
    B, H, Sq, D = q.shape
    assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == (B, H, Sq) and lse.dtype == torch.float32
    err = fo.block_errors(O, o, block=Sq)[..., 0]                              # [B, H]
    at = tuple(int(x) for x in torch.unravel_index(err.argmax(), err.shape))
    print("%s: worst (b, h) %s relFro %.3e bound %.0e" % (tag, at, err[at].item(), BOUND[q.dtype]))
    assert (err < BOUND[q.dtype]).all(), (tag, "(b, h)", at, err[at].item(), lens[at[0]])
    check_lse(lse, LSE)
    return O, LSE


def same(a, b):
    """(O, LSE) pairs with the same bits"""
    return a[0].shape == b[0].shape and torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and \
        torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def scatter(k8, v8, ks, vs, lens, page, num_pages, max_pages, seed, alloc=None, fill_scale=float("nan")):
    """pools of the caches (NaN bytes elsewhere) and of the scales (NaN elsewhere) under one permuted table"""
    (kp, vp), table = pc.scatter((k8, v8), lens, page, num_pages, max_pages, seed, alloc=alloc)
    pools = []
    for s in (ks, vs):
        pool = torch.full((num_pages, s.shape[1], page), fill_scale, dtype=torch.float32, device=s.device)
        for b, L in enumerate(lens):
            for i in range(pc.pages_of(L, page)):
                n = min(page, L - i * page)
                pool[int(table[b, i]), :, :n] = s[b, :, i * page:i * page + n]
        pools.append(pool)
    return kp, vp, pools[0], pools[1], table


def gather_scales(pool, table):
    """the padded scales [B, H_kv, max_pages * page] a scale pool and a table describe"""
    B, mp = table.shape
    return pool[table.long()].permute(0, 2, 1, 3).reshape(B, pool.shape[1], mp * pool.shape[2]).contiguous()


def padded(q, k8, v8, ks, vs, sl, **kw):
    return T().flash_attention_kvcache_fp8_token(q, k8, v8, ks, vs, sl, return_lse=True, **kw)


def paged(q, kp, vp, ksp, vsp, sl, table, **kw):
    return T().flash_attention_kvcache_fp8_token_paged(q, kp, vp, ksp, vsp, sl, table, return_lse=True, **kw)


def packed(qs, kp, vp, ksp, vsp, sl, table, k_new=None, v_new=None, total_q=None, **kw):
    """qs[b]: [1, H, S_b, D] -> the per-sequence (O [1, H, S_b, D], LSE [1, H, S_b]) of one packed call; k_new / v_new: per
    sequence [1, H_kv, S_b, D]"""
    S = [t.shape[2] for t in qs]
    total = total_q or sum(S)
    pk = lambda ts: None if ts is None else rg.pack(ts, total, fill=0.0)
    o, lse = T().flash_attention_kvcache_fp8_token_ragged(rg.pack(qs, total, fill=0.0), kp, vp, ksp, vsp, rg.cu_of(S, device="cuda"),
                                                          sl, table, k_new=pk(k_new), v_new=pk(v_new), return_lse=True, **kw)
    return list(zip(rg.unpack(o, S), rg.unpack_lse(lse, S)))
