"""Decoding attention over a paged KV cache with PACKED VARIABLE-LENGTH QUERIES (include/mi355fa_ragged.h): one call for a
step of continuous batching, in which some sequences decode one token, some verify a speculative draft and some run a chunk
of their prefill -- vLLM's flash_attn_varlen_func(..., cu_seqlens_q, seqused_k, block_table), FlashAttention's
flash_attn_with_kvcache(cu_seqlens_q=...).  A module beside paged_kvcache.py, whose public names are a recorded surface, as
those of My_FlashAttention_optimized.py are; the native side is paged_kvcache.py's, csrc/torch_binding_paged.cpp ->
_mi355fa_paged_torch.so over libmi355fa.so.  There is NO fallback: a missing library or binding is an ImportError."""
import torch

from My_FlashAttention_optimized import _gqa_window
import _mi355fa_paged_torch as _ext   # raises if the binding was not built (make -C csrc)
from paged_kvcache import _check_no_grad, _check_variant

__all__ = ["flash_attention_kvcache_ragged"]


def _check_packed(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, shapes):
    """what a packed call checks of its geometry, whatever the pools hold (fp4_ragged_kvcache.py shares it); `shapes`: the
    call's words for q and its pools"""
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache), ("cu_seqlens_q", cu_seqlens_q),
                    ("cache_seqlens", cache_seqlens), ("block_table", block_table)):
        assert isinstance(t, torch.Tensor), name + " must be a tensor"
    assert cu_seqlens_q.dtype == torch.int32, "cu_seqlens_q must be int32 (got %s)" % cu_seqlens_q.dtype
    assert cu_seqlens_q.dim() == 1 and cu_seqlens_q.numel() >= 2, \
        "cu_seqlens_q must be a vector of B + 1 entries, B >= 1 (got shape %s)" % (tuple(cu_seqlens_q.shape),)
    B = cu_seqlens_q.numel() - 1
    assert block_table.dtype == torch.int32, "block_table must be int32 (got %s)" % block_table.dtype
    assert block_table.dim() == 2 and block_table.shape[0] == B, \
        "block_table must be [B, max_pages_per_seq] with B = %d, the sequences of cu_seqlens_q" % B
    assert cache_seqlens.dim() == 1 and cache_seqlens.numel() == B, \
        "cache_seqlens must have B = %d entries, the sequences of cu_seqlens_q" % B
    assert q.dim() == 3 and k_cache.dim() == 4 and v_cache.dim() == 4, shapes


def _check_out(q, out):
    if out is not None:
        assert isinstance(out, torch.Tensor), "out must be a tensor"
        assert out.shape == q.shape, "out must have q's shape %s (got %s)" % (tuple(q.shape), tuple(out.shape))
        assert out.dtype == q.dtype, "out must have q's dtype %s (got %s)" % (q.dtype, out.dtype)


def flash_attention_kvcache_ragged(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, k_new=None, v_new=None,
                                   is_causal=False, window_size=(-1, -1), softmax_scale=None, return_lse=False, softcap=None,
                                   alibi_slopes=None, sinks=None, k_descale=None, v_descale=None, out=None):
    """paged_kvcache.flash_attention_kvcache_paged with a query count per sequence.

    q [total_q, H, D], fp16 or bf16, D in {64, 128, 256}: the queries of all sequences packed along the first dimension, read in
    place through its row and head strides (D innermost, rows 16-byte aligned), so a slice of a fused QKV projection goes
    in without a copy.  cu_seqlens_q: int32 device tensor [B + 1]; sequence b owns the rows [cu[b], cu[b + 1]), S_b of
    them (0 is allowed).  Rows at or past cu[B] are padding -- the tail of a graph-captured step: never read, and the
    matching rows of the result and of LSE are never written.  There is no max_seqlen_q: the launch is sized from total_q
    and B, and a list of the step's row blocks is built on the device.

    k_cache, v_cache, block_table [B, max_pages_per_seq], cache_seqlens [B], the variants (at most one of softcap,
    alibi_slopes and sinks; an fp8 pool takes sinks only, with k_descale / v_descale) and their refusals: exactly as in
    flash_attention_kvcache_paged.  A padded cache [B, H_kv, S_cache, D] with S_cache % 32 == 0 goes in as a pool whose
    table is arange(B)[:, None].  The host reads none of cu_seqlens_q, cache_seqlens and block_table: a step captured at a
    fixed total_q and B replays while all three change in place.  Whatever cu_seqlens_q holds, nothing outside q, out, LSE
    and the pool is touched; sequences whose rows are not their own (a non-monotone, negative or too large entry) get
    unspecified results.

    Query i of sequence b sits at position L_b - S_b + i (bottom-right aligned), with L_b = cache_seqlens[b], or
    cache_seqlens[b] + S_b when k_new / v_new [total_q, H_kv, D] (both or neither, q's dtype) are given: each query row
    brings its key and value, and packed row cu[b] + i is written to cache row cache_seqlens[b] + i of sequence b through
    the table before attention (an fp8 pool quantises it; rows past the table are dropped; cache_seqlens is not
    modified).  A row with no visible key gets O = 0 and LSE = -inf.

    out: optional, q's shape and dtype, written in place through its strides; otherwise a contiguous tensor is allocated.
    Returns O [total_q, H, D] (and LSE [H, total_q] fp32 with return_lse=True).  The rows of sequence b have the bits of
    flash_attention_kvcache_paged on that sequence alone.  Inference only: an input that requires grad is refused."""
    wl, wr = _gqa_window(is_causal, window_size)
    _check_packed(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table,
                  "q must be [total_q, H, D], the pools [num_pages, H_kv, page_size, D]")
    scale, cap = _check_variant(k_cache, softmax_scale, softcap, alibi_slopes, sinks, k_descale, v_descale, k_new, v_new)
    _check_out(q, out)
    _check_no_grad("flash_attention_kvcache_ragged", q=q, k_cache=k_cache, v_cache=v_cache, k_new=k_new, v_new=v_new,
                   alibi_slopes=alibi_slopes, sinks=sinks, k_descale=k_descale, v_descale=v_descale, out=out)
    assert cu_seqlens_q.is_cuda, "cu_seqlens_q must be a device tensor: the kernels read it, the host never does"
    O, LSE = _ext.kvcache_ragged_forward(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, k_new, v_new, wl, wr,
                                         scale, cap, alibi_slopes, sinks, k_descale, v_descale, out)
    return (O, LSE) if return_lse else O
