"""Decoding attention with LOGIT SOFT-CAPPING over the quantised KV caches (include_quant/mi355fa_kvcache_quant_softcap.h): what a
model that caps its logits -- Gemma 2 (cap 50, D = 256, alternating sliding windows), Grok-1 -- needs to leave the 16-bit cache.
Every score s = q . dequantised(k) becomes softcap * tanh(softmax_scale * s / softcap) before the masks, as in
flash_attention_kvcache_softcap; the cache is one of the three quantised formats, told from its tensors:

    float8_e4m3fn caches, no k_scale / v_scale        per-tensor e4m3 (flash_attention_kvcache_fp8): k_descale / v_descale optional
    float8_e4m3fn caches, float32 k_scale / v_scale   per-token e4m3 (fp8_token_kvcache.py)
    nibble caches (quantize_kv_mxfp4), uint8 scales   MXFP4 (fp4_kvcache.py)

Padded and paged caches and packed variable-length queries.  D = 64, 128 and 256 for the per-tensor format; 64 and 128 for the
other two, and 256 on their packed call.  A module beside fp8_token_kvcache.py and the others, whose public names are recorded
surfaces; the native side is csrc/torch_binding_quant_softcap.cpp -> _mi355fa_quant_softcap_torch.so over libmi355fa.so.  There is
NO fallback: a missing library or binding is an ImportError."""
import math

import torch

from My_FlashAttention_optimized import _gqa_window
from paged_kvcache import _check_no_grad, _check_page
from ragged_kvcache import _check_packed, _check_out
import fp4_kvcache as _fp4
import fp8_token_kvcache as _tok
import _mi355fa_quant_softcap_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["flash_attention_kvcache_quant_softcap", "flash_attention_kvcache_quant_softcap_paged",
           "flash_attention_kvcache_quant_softcap_ragged"]

E4M3, E4M3_TOKEN, MXFP4 = 0, 1, 2      # the header's MI355FA_QUANT_*
_FORMATS = ("the cache must be one of three: float8_e4m3fn caches without k_scale / v_scale (per-tensor e4m3, k_descale / "
            "v_descale optional), float8_e4m3fn caches with float32 k_scale / v_scale (per-token e4m3), or nibble caches "
            "(uint8 or float4_e2m1fn_x2, what quantize_kv_mxfp4 returns) with uint8 k_scale / v_scale (MXFP4)")


def _format(q, k_cache, v_cache, k_scale, v_scale, k_descale, v_descale, packed):
    """the format of the call's tensors, and the caches and scales as the binding takes them; each format checked by its own
    module's check"""
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        assert isinstance(t, torch.Tensor), name + " must be a tensor"
    assert (k_scale is None) == (v_scale is None), "k_scale and v_scale must be given together"
    scaled, descaled = k_scale is not None, k_descale is not None or v_descale is not None
    assert not (scaled and descaled), \
        "k_descale / v_descale belong to a per-tensor e4m3 cache and k_scale / v_scale to the other two formats: not both"
    fp8 = k_cache.dtype == torch.float8_e4m3fn and v_cache.dtype == torch.float8_e4m3fn
    nibbles = k_cache.dtype in (torch.uint8, torch.float4_e2m1fn_x2) and v_cache.dtype == k_cache.dtype
    if scaled:
        for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
            assert isinstance(t, torch.Tensor), name + " must be a tensor"
    if fp8 and not scaled:
        assert k_cache.dim() == 4 and v_cache.shape == k_cache.shape, "k_cache and v_cache must be 4-d and have the same shape"
        assert q.shape[-1] in (64, 128, 256), "q's head dim must be 64 or 128 or 256 (got %d)" % q.shape[-1]
        for name, t in (("k_descale", k_descale), ("v_descale", v_descale)):
            assert t is None or (isinstance(t, torch.Tensor) and t.dtype == torch.float32), name + " must be a float32 tensor"
        return E4M3, k_cache, v_cache, None, None
    if fp8 and scaled and k_scale.dtype == torch.float32 and v_scale.dtype == torch.float32:
        _tok._check_formats(q, k_cache, v_cache, k_scale, v_scale, (64, 128, 256) if packed else (64, 128))
        return E4M3_TOKEN, k_cache, v_cache, k_scale, v_scale
    if nibbles and scaled and k_scale.dtype in (torch.uint8, torch.float8_e8m0fnu) and v_scale.dtype == k_scale.dtype:
        kc, vc, ks, vs = _fp4._check_formats(k_cache, v_cache, k_scale, v_scale)
        dims = (64, 128, 256) if packed else (64, 128)
        assert q.shape[-1] in dims, "q's head dim must be %s: an MXFP4 cache has no D = %d kernel here" % (
            " or ".join(str(d) for d in dims), q.shape[-1])
        return MXFP4, kc, vc, ks, vs
    raise AssertionError(_FORMATS + " (got caches %s / %s, scales %s / %s)" % (
        k_cache.dtype, v_cache.dtype, getattr(k_scale, "dtype", None), getattr(v_scale, "dtype", None)))


def _check_cap(softcap):
    assert isinstance(softcap, (int, float)) and not isinstance(softcap, bool), "softcap must be a number"
    softcap = float(softcap)
    assert math.isfinite(softcap) and softcap > 0.0, "softcap must be finite and > 0 (got %r)" % softcap
    return softcap


def _call(fn, q, k_cache, v_cache, cache_seqlens, block_table, softcap, k_scale, v_scale, k_descale, v_descale, k_new, v_new,
          is_causal, window_size, softmax_scale, return_lse):
    wl, wr = _gqa_window(is_causal, window_size)
    assert isinstance(cache_seqlens, torch.Tensor), "cache_seqlens must be a tensor"
    assert isinstance(q, torch.Tensor) and q.dim() == 4, "q must be [B, H, S_q, D]"
    cap = _check_cap(softcap)
    fmt, kc, vc, ks, vs = _format(q, k_cache, v_cache, k_scale, v_scale, k_descale, v_descale, False)
    scale = _fp4._check_scale_and_new(softmax_scale, k_new, v_new)
    _check_no_grad(fn, q=q, k_cache=k_cache, v_cache=v_cache, k_scale=k_scale, v_scale=v_scale, k_descale=k_descale,
                   v_descale=v_descale, k_new=k_new, v_new=v_new)
    O, LSE = _ext.kvcache_quant_softcap_forward(q, kc, vc, cache_seqlens, block_table, cap, fmt, ks, vs, k_descale, v_descale,
                                                k_new, v_new, wl, wr, scale)
    return (O, LSE) if return_lse else O


def flash_attention_kvcache_quant_softcap(q, k_cache, v_cache, cache_seqlens, softcap, k_scale=None, v_scale=None,
                                          k_descale=None, v_descale=None, k_new=None, v_new=None, is_causal=False,
                                          window_size=(-1, -1), softmax_scale=None, return_lse=False):
    """flash_attention_kvcache_softcap over a quantised cache.

    q [B, H, S_q, D], fp16 or bf16.  The cache, by its tensors (anything else is refused):
      per-tensor e4m3   k_cache, v_cache [B, H_kv, S_cache, D] torch.float8_e4m3fn, no scales; k_descale / v_descale (H_kv,) or
                        (B, H_kv) float32 device tensors or None (1.0), as in flash_attention_kvcache_fp8.  D in {64, 128, 256}.
      per-token e4m3    the same caches with k_scale, v_scale [B, H_kv, S_cache] float32 (fp8_token_kvcache.py).  D in {64, 128}.
      MXFP4             k_cache, v_cache [B, H_kv, S_cache, D/2] nibbles and k_scale, v_scale [B, H_kv, S_cache, D/32] e8m0 bytes,
                        what quantize_kv_mxfp4 returns (fp4_kvcache.py).  D in {64, 128}.
    Descales together with scales are refused.  Caches and scales are read -- and appended to -- in place through their strides.

    softcap: finite and > 0.  Every score s = q . K with K the DEQUANTISED key becomes softcap * tanh(softmax_scale * s / softcap)
    before the masks: k_descale and the per-token K scale go under the tanh.  There are no sinks and no alibi_slopes here: at
    most one transform.  cache_seqlens, k_new / v_new (quantised on the device by the format's own quantiser into the caches and
    the scales before attention), is_causal, window_size, softmax_scale and return_lse as in the format's own call; the host
    reads none of the device-side lengths, descales or scales, so a step can be captured in a graph.

    Returns O [B, H, S_q, D] (and LSE [B, H, S_q] fp32 with return_lse=True).  Inference only: an input that requires grad is
    refused."""
    return _call("flash_attention_kvcache_quant_softcap", q, k_cache, v_cache, cache_seqlens, None, softcap, k_scale, v_scale,
                 k_descale, v_descale, k_new, v_new, is_causal, window_size, softmax_scale, return_lse)


def flash_attention_kvcache_quant_softcap_paged(q, k_cache, v_cache, cache_seqlens, block_table, softcap, k_scale=None,
                                                v_scale=None, k_descale=None, v_descale=None, k_new=None, v_new=None,
                                                is_causal=False, window_size=(-1, -1), softmax_scale=None, return_lse=False):
    """flash_attention_kvcache_quant_softcap over paged pools: k_cache, v_cache [num_pages, H_kv, page_size, .] and (per-token
    e4m3, MXFP4) the scale pools with the same leading dimensions, page_size a positive multiple of 32; block_table int32 device
    tensor [B, max_pages_per_seq] as in flash_attention_kvcache_paged.  The result has the bits of
    flash_attention_kvcache_quant_softcap on the gathered cache (and scales)."""
    _tok._check_paged(k_cache, block_table, "[num_pages, H_kv, page_size, .]")
    return _call("flash_attention_kvcache_quant_softcap_paged", q, k_cache, v_cache, cache_seqlens, block_table, softcap,
                 k_scale, v_scale, k_descale, v_descale, k_new, v_new, is_causal, window_size, softmax_scale, return_lse)


def flash_attention_kvcache_quant_softcap_ragged(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, softcap,
                                                 k_scale=None, v_scale=None, k_descale=None, v_descale=None, k_new=None,
                                                 v_new=None, is_causal=False, window_size=(-1, -1), softmax_scale=None,
                                                 return_lse=False, out=None):
    """ragged_kvcache.flash_attention_kvcache_ragged, soft-capped, over the pools of flash_attention_kvcache_quant_softcap_paged.

    q [total_q, H, D], fp16 or bf16, D in {64, 128, 256} for every format, packed along the first dimension; cu_seqlens_q int32
    device tensor [B + 1]; rows at or past cu[B] are padding, never read and never written.  k_new / v_new [total_q, H_kv, D]:
    packed row cu[b] + i is quantised into row cache_seqlens[b] + i of sequence b through the table before attention.  out:
    optional, q's shape and dtype, written in place through its strides.  A padded cache with S_cache % 32 == 0 goes in as a pool
    whose table is arange(B)[:, None] -- for the per-token and MXFP4 formats at D = 256 the only way in.  The host reads none of
    cu_seqlens_q, cache_seqlens, block_table, the descales and the scales.

    Returns O [total_q, H, D] (and LSE [H, total_q] fp32 with return_lse=True).  At D = 64 and 128 the rows of sequence b have the
    bits of flash_attention_kvcache_quant_softcap_paged on that sequence alone.  Inference only."""
    fn = "flash_attention_kvcache_quant_softcap_ragged"
    wl, wr = _gqa_window(is_causal, window_size)
    _check_packed(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table,
                  "q must be [total_q, H, D], the pools [num_pages, H_kv, page_size, .]")
    cap = _check_cap(softcap)
    fmt, kc, vc, ks, vs = _format(q, k_cache, v_cache, k_scale, v_scale, k_descale, v_descale, True)
    _check_page(k_cache)
    scale = _fp4._check_scale_and_new(softmax_scale, k_new, v_new)
    _check_out(q, out)
    _check_no_grad(fn, q=q, k_cache=k_cache, v_cache=v_cache, k_scale=k_scale, v_scale=v_scale, k_descale=k_descale,
                   v_descale=v_descale, k_new=k_new, v_new=v_new, out=out)
    assert cu_seqlens_q.is_cuda, "cu_seqlens_q must be a device tensor: the kernels read it, the host never does"
    assert block_table.is_cuda, "block_table must be a device tensor: the kernels read it, the host never does"
    O, LSE = _ext.kvcache_quant_softcap_ragged_forward(q, kc, vc, cu_seqlens_q, cache_seqlens, block_table, cap, fmt, ks, vs,
                                                       k_descale, v_descale, k_new, v_new, wl, wr, scale, out)
    return (O, LSE) if return_lse else O
