"""Decoding attention with PACKED VARIABLE-LENGTH QUERIES over paged MXFP4 pools (include/mi355fa_ragged_fp4.h): the
continuous-batching step of ragged_kvcache.py -- decode rows, speculative drafts and prefill chunks in one launch, the host
reading nothing -- over the cache format of fp4_kvcache.py, e2m1 nibbles with one e8m0 scale byte per 32 elements.  D = 64,
128 and 256: this is the one MXFP4 call at D = 256.  A module beside the two, whose public names are recorded surfaces; the
native side is csrc/torch_binding_fp4.cpp -> _mi355fa_fp4_torch.so over libmi355fa.so.  There is NO fallback: a missing
library or binding is an ImportError."""
import torch

from My_FlashAttention_optimized import _gqa_window
from paged_kvcache import _check_no_grad, _check_page
from ragged_kvcache import _check_packed, _check_out
from fp4_kvcache import _check_formats, _check_scale_and_new
import _mi355fa_fp4_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["flash_attention_kvcache_fp4_ragged"]


def flash_attention_kvcache_fp4_ragged(q, k_cache, v_cache, k_scale, v_scale, cu_seqlens_q, cache_seqlens, block_table,
                                       k_new=None, v_new=None, is_causal=False, window_size=(-1, -1), softmax_scale=None,
                                       return_lse=False, sinks=None, out=None):
    """ragged_kvcache.flash_attention_kvcache_ragged over the pools of fp4_kvcache.flash_attention_kvcache_fp4_paged.

    q [total_q, H, D], fp16 or bf16, D in {64, 128, 256}, packed along the first dimension and read in place through its
    row and head strides (a slice of a fused QKV projection goes in without a copy).  cu_seqlens_q: int32 device tensor
    [B + 1]; sequence b owns the rows [cu[b], cu[b + 1]), S_b of them (0 is allowed); rows at or past cu[B] are padding,
    never read, and the matching rows of the result and of LSE are never written.

    k_cache, v_cache [num_pages, H_kv, page_size, D/2], uint8 or torch.float4_e2m1fn_x2; k_scale, v_scale
    [num_pages, H_kv, page_size, D/32], uint8 or torch.float8_e8m0fnu; page_size a positive multiple of 32.  All four are
    read -- and appended to -- in place through their strides ([num_pages, page_size, H_kv, .] storage goes in as
    .transpose(1, 2)) and are never copied.  block_table [B, max_pages_per_seq] and cache_seqlens [B], int32 device
    tensors, as in flash_attention_kvcache_fp4_paged.  A padded MXFP4 cache [B, H_kv, S_cache, D/2] with S_cache % 32 == 0
    goes in as a pool whose table is arange(B)[:, None] -- at D = 256 the only way in.  The host reads none of cu_seqlens_q,
    cache_seqlens, block_table and the scales: a step captured at a fixed total_q and B replays while they change in place.

    Query i of sequence b sits at position L_b - S_b + i, with L_b = cache_seqlens[b], or cache_seqlens[b] + S_b when
    k_new / v_new [total_q, H_kv, D] (both or neither, q's dtype) are given: packed row cu[b] + i is quantised on the
    device, exactly as quantize_kv_mxfp4 does, into row cache_seqlens[b] + i of sequence b -- nibbles and scale bytes --
    through the table before attention.  Rows past the table, or whose entry is outside the pool, are dropped;
    cache_seqlens is not modified.  is_causal, window_size, softmax_scale, return_lse as in flash_attention_kvcache; sinks:
    (H,) fp32 logits or None.  There is no softcap or alibi_slopes: those have no MXFP4 kernel.

    out: optional, q's shape and dtype, written in place through its strides.  Returns O [total_q, H, D] (and LSE
    [H, total_q] fp32 with return_lse=True).  At D = 64 and 128 the rows of sequence b have the bits of
    flash_attention_kvcache_fp4_paged on that sequence alone.  Inference only: an input that requires grad is refused."""
    wl, wr = _gqa_window(is_causal, window_size)
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        assert isinstance(t, torch.Tensor), name + " must be a tensor"
    _check_packed(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table,
                  "q must be [total_q, H, D], the pools [num_pages, H_kv, page_size, D/2]")
    kc, vc, ks, vs = _check_formats(k_cache, v_cache, k_scale, v_scale)
    assert q.shape[-1] in (64, 128, 256), \
        "q must be [total_q, H, D] with D = 64, 128 or 256: an MXFP4 cache has no D = %d kernel" % q.shape[-1]
    _check_page(k_cache)
    scale = _check_scale_and_new(softmax_scale, k_new, v_new)
    _check_out(q, out)
    _check_no_grad("flash_attention_kvcache_fp4_ragged", q=q, k_new=k_new, v_new=v_new, sinks=sinks, out=out)
    assert cu_seqlens_q.is_cuda, "cu_seqlens_q must be a device tensor: the kernels read it, the host never does"
    assert block_table.is_cuda, "block_table must be a device tensor: the kernels read it, the host never does"
    O, LSE = _ext.kvcache_fp4_ragged_forward(q, kc, vc, ks, vs, cu_seqlens_q, cache_seqlens, block_table, k_new, v_new, wl,
                                             wr, scale, sinks, out)
    return (O, LSE) if return_lse else O
