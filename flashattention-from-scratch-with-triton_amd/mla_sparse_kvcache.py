"""Sparse (top-k indexed) MLA decoding over the paged latent cache (include_mla_sparse/mi355fa_kvcache_mla_sparse.h): the decode
step of DeepSeek-V3.2 and its successors, where an indexer picks per query token the cached tokens -- the same for all heads of
that token -- and attention runs over those alone.  The cache is mla_kvcache's 16-bit pool, read in place by a gathering kernel:
no row is copied.  A module beside the other decode modules; the native side is csrc/torch_binding_mla_sparse.cpp ->
_mi355fa_mla_sparse_torch.so over libmi355fa.so.  There is NO fallback: a missing library or binding is an ImportError."""
import torch

from mla_kvcache import _check_call
import _mi355fa_mla_sparse_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["flash_attention_mla_kvcache_sparse"]


def flash_attention_mla_kvcache_sparse(q, kv_cache, indices, cache_seqlens, block_table, kv_new=None, is_causal=False,
                                       softmax_scale=None, return_lse=False, out=None):
    """Attention of absorbed MLA queries over the cached tokens their index lists name, after appending this step's rows.

    q [B, H, S_q, 576], kv_cache [num_pages, page_size, 576], cache_seqlens, block_table, kv_new, softmax_scale, out and the
    return value are those of mla_kvcache.flash_attention_mla_kvcache: the pool is read and appended to in place through its
    strides, may exceed 4 GiB and is never copied; the host reads no device memory, so a step can be captured in a graph and
    replayed while indices, cache_seqlens and block_table change in place.

    indices: int32 device tensor [B, S_q, topk], topk >= 1, unit stride along topk (batch and row strides are free: a slice of
    a wider tensor goes in as it is).  Entry j of (b, i) is a LOGICAL position of sequence b -- the key in page
    block_table[b, idx // page_size], row idx % page_size --, not a pool row.  With L_b = cache_seqlens[b] + S_new (clamped to
    the table's reach), query i of sequence b attends to exactly the entries with 0 <= idx < L_b and, with is_causal, also
    idx <= L_b - S_q + i.  Every other entry is skipped: -1 padding, garbage, a position behind the query.  An entry that
    appears twice counts twice; the order of a list does not change the mathematical result.  A visible idx whose table entry
    is outside [0, num_pages) reads as skipped and makes that sequence's result unspecified; nothing outside the pool is
    touched whatever the lists hold.  kv_new is appended before attention, so a list may name the rows being appended.

    Returns O [B, H, S_q, 512] and, with return_lse=True, LSE [B, H, S_q] fp32 in natural-log units; a row with no visible
    entry gets O = 0 and LSE = -inf.  softmax_scale defaults to 576 ** -0.5 (DeepSeek passes (128 + 64) ** -0.5 times its
    mscale).  Inference only: an input that requires grad is refused."""
    scale = _check_call("flash_attention_mla_kvcache_sparse",
                        (("q", q), ("kv_cache", kv_cache), ("indices", indices), ("cache_seqlens", cache_seqlens), ("block_table", block_table)), None,
                        (("indices", indices), ("block_table", block_table), ("cache_seqlens", cache_seqlens)),
                        (("indices", indices, "kernel"), ("cache_seqlens", cache_seqlens, "kernels"), ("block_table", block_table, "kernels")),
                        softmax_scale, q=q, kv_cache=kv_cache, kv_new=kv_new, out=out)
    O, LSE = _ext.kvcache_mla_sparse_forward(q, kv_cache, indices, cache_seqlens, block_table, kv_new, bool(is_causal), scale, out)
    return (O, LSE) if return_lse else O
