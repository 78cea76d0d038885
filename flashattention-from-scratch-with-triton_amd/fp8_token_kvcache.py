"""Decoding attention over an e4m3 KV cache with ONE FP32 SCALE PER CACHED TOKEN AND K/V HEAD
(include/mi355fa_kvcache_fp8_token.h): the FP8 cache of a serving stack that has no calibration data.  The bytes are those of
flash_attention_kvcache_fp8; instead of one k_descale[b, hk] fixed for the life of a sequence, every row brings the scale it was
quantised with when it was appended, so there is no calibration pass and one outlier token costs the other tokens nothing.  A
key of D = 128 costs 132 bytes against 128 in a per-tensor e4m3 cache and 256 in a bf16 one.  Padded and paged caches and packed
variable-length queries, plain attention and sinks, D = 64 and 128 (packed queries: also 256).  A module beside fp4_kvcache.py
and the others, whose public names are recorded surfaces; the native side is csrc/torch_binding_fp8_token.cpp ->
_mi355fa_fp8_token_torch.so over libmi355fa.so.  There is NO fallback: a missing library or binding is an ImportError."""
import torch

from My_FlashAttention_optimized import _gqa_window
from paged_kvcache import _check_no_grad, _check_page
from ragged_kvcache import _check_packed, _check_out
from fp4_kvcache import _check_block_table, _check_scale_and_new
import _mi355fa_fp8_token_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["quantize_kv_fp8_per_token", "dequantize_kv_fp8_per_token", "flash_attention_kvcache_fp8_token",
           "flash_attention_kvcache_fp8_token_paged", "flash_attention_kvcache_fp8_token_ragged"]

_E4M3_MAX = 448.0


def quantize_kv_fp8_per_token(x):
    """x [..., D] (any float dtype, any device) -> (x8 torch.float8_e4m3fn [..., D], scale float32 x.shape[:-1]).

    Per row of D elements: amax = max |float(x)|; s = amax / 448 in fp32, and 1.0 where that is not a normal fp32 number (an
    all-zero row, a subnormal quotient); byte = e4m3_rne(clamp(float(x) / s, -448, 448)) -- divide, saturate, round to nearest
    even, -0.0 kept, the cast quantize_kv_fp8 documents.  NaN and Inf inputs are unspecified.  These are the bytes and the
    scale bits the append of flash_attention_kvcache_fp8_token writes for k_new / v_new."""
    assert isinstance(x, torch.Tensor) and x.is_floating_point() and x.dim() >= 1, "x must be a floating-point tensor [..., D]"
    xf = x.detach().float()
    s = xf.abs().amax(dim=-1) / _E4M3_MAX
    field = (s.contiguous().view(torch.int32) >> 23) & 0xFF
    s = torch.where((field >= 1) & (field <= 254), s, torch.ones_like(s))
    x8 = (xf / s.unsqueeze(-1)).clamp(-_E4M3_MAX, _E4M3_MAX).to(torch.float8_e4m3fn)
    return x8, s


def dequantize_kv_fp8_per_token(x8, scale, dtype=torch.float32):
    """(x8 [..., D] torch.float8_e4m3fn, scale float32 [...]) -> [..., D] in `dtype`: float(byte) * scale, the product formed in
    fp32 and then converted."""
    assert isinstance(x8, torch.Tensor) and x8.dtype == torch.float8_e4m3fn, "x8 must be torch.float8_e4m3fn"
    assert isinstance(scale, torch.Tensor) and scale.dtype == torch.float32 and scale.shape == x8.shape[:-1], \
        "scale must be float32 with x8's shape without the last dimension"
    return (x8.float() * scale.unsqueeze(-1)).to(dtype)


def _check_formats(q, k_cache, v_cache, k_scale, v_scale, dims):
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache), ("k_scale", k_scale), ("v_scale", v_scale)):
        assert isinstance(t, torch.Tensor), name + " must be a tensor"
    assert k_cache.dtype == torch.float8_e4m3fn and v_cache.dtype == torch.float8_e4m3fn, \
        "k_cache and v_cache must be torch.float8_e4m3fn (got %s, %s)" % (k_cache.dtype, v_cache.dtype)
    assert k_scale.dtype == torch.float32 and v_scale.dtype == torch.float32, \
        "k_scale and v_scale must be float32 (got %s, %s)" % (k_scale.dtype, v_scale.dtype)
    assert k_cache.dim() == 4 and v_cache.shape == k_cache.shape, "k_cache and v_cache must be 4-d and have the same shape"
    assert tuple(k_scale.shape) == tuple(k_cache.shape[:-1]) and tuple(v_scale.shape) == tuple(k_cache.shape[:-1]), \
        "k_scale and v_scale must have the caches' shape without D, %s (got %s, %s)" % (
            tuple(k_cache.shape[:-1]), tuple(k_scale.shape), tuple(v_scale.shape))
    assert q.shape[-1] in dims, "q's head dim must be %s: a per-token-scaled cache has no D = %d kernel here" % (
        " or ".join(str(d) for d in dims), q.shape[-1])


def _check_paged(k_cache, block_table, pool):
    """the front of a _paged call here and in quant_softcap_kvcache.py; `pool`: the call's word for the pools' shape"""
    _check_block_table(block_table)
    assert isinstance(k_cache, torch.Tensor) and k_cache.dim() == 4, "k_cache must be a pool " + pool
    _check_page(k_cache)
    assert block_table.is_cuda, "block_table must be a device tensor: the kernels read it, the host never does"


def _call(fn, q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, block_table, k_new, v_new, is_causal, window_size,
          softmax_scale, return_lse, sinks):
    wl, wr = _gqa_window(is_causal, window_size)
    assert isinstance(cache_seqlens, torch.Tensor), "cache_seqlens must be a tensor"
    assert isinstance(q, torch.Tensor) and q.dim() == 4, "q must be [B, H, S_q, D]"
    _check_formats(q, k_cache, v_cache, k_scale, v_scale, (64, 128))
    scale = _check_scale_and_new(softmax_scale, k_new, v_new)
    _check_no_grad(fn, q=q, k_scale=k_scale, v_scale=v_scale, k_new=k_new, v_new=v_new, sinks=sinks)
    O, LSE = _ext.kvcache_fp8_token_forward(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, block_table, k_new, v_new,
                                            wl, wr, scale, sinks)
    return (O, LSE) if return_lse else O


def flash_attention_kvcache_fp8_token(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, k_new=None, v_new=None,
                                      is_causal=False, window_size=(-1, -1), softmax_scale=None, return_lse=False, sinks=None):
    """flash_attention_kvcache over an e4m3 cache with one fp32 scale per cached token and K/V head.

    q [B, H, S_q, D], fp16 or bf16, D in {64, 128}.  k_cache, v_cache [B, H_kv, S_cache, D], torch.float8_e4m3fn; k_scale,
    v_scale [B, H_kv, S_cache], float32, so that K[b, hk, j, :] = float(k_cache[b, hk, j, :]) * k_scale[b, hk, j]
    (dequantize_kv_fp8_per_token), V likewise.  All four are read -- and appended to -- in place through their strides
    ([B, S_cache, H_kv, D] caches with [B, S_cache, H_kv] scales go in as .transpose(1, 2)) and are never copied; a cache the
    kernels cannot address is refused.  There is no per-(sequence, head) descale on top.  A scale that is not a finite normal
    number > 0 gives unspecified results.

    cache_seqlens: int32 device tensor [B]; the host never reads it or the scales, so a step can be captured in a graph.
    k_new, v_new [B, H_kv, S_new, D] (both or neither, q's dtype): quantised on the device, exactly as
    quantize_kv_fp8_per_token does, into the rows [cache_seqlens[b], cache_seqlens[b] + S_new) of the caches and of the scales
    before attention.  Rows at or past L_b are never read.  is_causal, window_size, softmax_scale, return_lse as in
    flash_attention_kvcache; sinks: (H,) fp32 logits as in flash_attention_kvcache_sink, or None.  There is no softcap or
    alibi_slopes.

    With every scale 1.0 the result has the bits of flash_attention_kvcache_fp8 without descales.  Returns O [B, H, S_q, D] (and
    LSE [B, H, S_q] fp32 with return_lse=True).  Inference only: an input that requires grad is refused."""
    return _call("flash_attention_kvcache_fp8_token", q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, None, k_new, v_new,
                 is_causal, window_size, softmax_scale, return_lse, sinks)


def flash_attention_kvcache_fp8_token_paged(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, block_table, k_new=None,
                                            v_new=None, is_causal=False, window_size=(-1, -1), softmax_scale=None,
                                            return_lse=False, sinks=None):
    """flash_attention_kvcache_fp8_token over paged pools: k_cache, v_cache [num_pages, H_kv, page_size, D] and k_scale, v_scale
    [num_pages, H_kv, page_size], page_size a positive multiple of 32; block_table int32 device tensor [B, max_pages_per_seq]
    as in flash_attention_kvcache_paged: key j of sequence b is row j % page_size of page block_table[b, j // page_size], in
    the caches and in the scales.  Entries at or past ceil(L_b / page_size) are never read; an entry outside [0, num_pages)
    below that makes that sequence's result unspecified, but nothing outside the pools is touched and an appended row that
    would land there is dropped, bytes and scale together.  Appended rows may cross pages.  The result has the bits of
    flash_attention_kvcache_fp8_token on the gathered cache and scales."""
    _check_paged(k_cache, block_table, "[num_pages, H_kv, page_size, D]")
    return _call("flash_attention_kvcache_fp8_token_paged", q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, block_table,
                 k_new, v_new, is_causal, window_size, softmax_scale, return_lse, sinks)


def flash_attention_kvcache_fp8_token_ragged(q, k_cache, v_cache, k_scale, v_scale, cu_seqlens_q, cache_seqlens, block_table,
                                             k_new=None, v_new=None, is_causal=False, window_size=(-1, -1), softmax_scale=None,
                                             return_lse=False, sinks=None, out=None):
    """ragged_kvcache.flash_attention_kvcache_ragged over the pools of flash_attention_kvcache_fp8_token_paged.

    q [total_q, H, D], fp16 or bf16, D in {64, 128, 256}, packed along the first dimension and read in place through its row
    and head strides.  cu_seqlens_q: int32 device tensor [B + 1]; sequence b owns the rows [cu[b], cu[b + 1]), S_b of them (0
    is allowed); rows at or past cu[B] are padding, never read, and the matching rows of the result and of LSE are never
    written.  The pools, the scale pools, block_table and cache_seqlens as in flash_attention_kvcache_fp8_token_paged.  A padded
    cache [B, H_kv, S_cache, D] with S_cache % 32 == 0 goes in as a pool whose table is arange(B)[:, None] -- at D = 256 the
    only way in.  The host reads none of cu_seqlens_q, cache_seqlens, block_table and the scales: a step captured at a fixed
    total_q and B replays while they change in place.

    Query i of sequence b sits at position L_b - S_b + i, with L_b = cache_seqlens[b], or cache_seqlens[b] + S_b when k_new /
    v_new [total_q, H_kv, D] (both or neither, q's dtype) are given: packed row cu[b] + i is quantised on the device, exactly as
    quantize_kv_fp8_per_token does, into row cache_seqlens[b] + i of sequence b -- bytes and scale -- through the table before
    attention.  Rows past the table, or whose entry is outside the pool, are dropped; cache_seqlens is not modified.

    out: optional, q's shape and dtype, written in place through its strides.  Returns O [total_q, H, D] (and LSE [H, total_q]
    fp32 with return_lse=True).  At D = 64 and 128 the rows of sequence b have the bits of
    flash_attention_kvcache_fp8_token_paged on that sequence alone.  Inference only."""
    wl, wr = _gqa_window(is_causal, window_size)
    _check_packed(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table,
                  "q must be [total_q, H, D], the pools [num_pages, H_kv, page_size, D]")
    _check_formats(q, k_cache, v_cache, k_scale, v_scale, (64, 128, 256))
    _check_page(k_cache)
    scale = _check_scale_and_new(softmax_scale, k_new, v_new)
    _check_out(q, out)
    _check_no_grad("flash_attention_kvcache_fp8_token_ragged", q=q, k_scale=k_scale, v_scale=v_scale, k_new=k_new, v_new=v_new,
                   sinks=sinks, out=out)
    assert cu_seqlens_q.is_cuda, "cu_seqlens_q must be a device tensor: the kernels read it, the host never does"
    assert block_table.is_cuda, "block_table must be a device tensor: the kernels read it, the host never does"
    O, LSE = _ext.kvcache_fp8_token_ragged_forward(q, k_cache, v_cache, k_scale, v_scale, cu_seqlens_q, cache_seqlens,
                                                   block_table, k_new, v_new, wl, wr, scale, sinks, out)
    return (O, LSE) if return_lse else O
