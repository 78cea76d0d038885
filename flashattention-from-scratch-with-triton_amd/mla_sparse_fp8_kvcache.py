"""Sparse (top-k indexed) MLA decoding over the paged FP8 LATENT cache (include_mla_sparse_fp8/mi355fa_kvcache_mla_sparse_fp8.h):
the decode step of DeepSeek-V3.2 as it is released -- an indexer picks per query token the cached tokens, the same for all heads
of that token, and attention runs over those alone, read out of mla_fp8_kvcache's pool of 656-byte rows in place by a gathering
kernel: no row is copied or dequantised outside it.  A module beside the other decode modules; the native side is
csrc/torch_binding_mla_sparse_fp8.cpp -> _mi355fa_mla_sparse_fp8_torch.so over libmi355fa.so.  There is NO fallback: a missing
library or binding is an ImportError."""
import torch

from mla_kvcache import _check_call
import _mi355fa_mla_sparse_fp8_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["flash_attention_mla_kvcache_sparse_fp8"]


def flash_attention_mla_kvcache_sparse_fp8(q, kv_cache, indices, cache_seqlens, block_table, kv_new=None, is_causal=False,
                                           softmax_scale=None, return_lse=False, out=None):
    """Attention of absorbed MLA queries over the cached FP8 rows their index lists name, after quantising this step's rows in.

    q [B, H, S_q, 576], cache_seqlens, block_table, softmax_scale, out and the return value are those of
    mla_kvcache.flash_attention_mla_kvcache.

    kv_cache and kv_new are those of mla_fp8_kvcache.flash_attention_mla_kvcache_fp8, word for word: the pool torch.uint8
    [num_pages, page_size, 656], rows as quantize_mla_latent_fp8 writes them with the RoPE values in q's dtype, page_size a
    positive multiple of 32, read and appended to in place through its page and row strides (the row stride may exceed 656
    bytes in multiples of 16; the pool may exceed 4 GiB; it is never copied); kv_new [B, S_q, 576] in q's dtype or None,
    UNQUANTISED rows that the call quantises on the device -- the bytes and scale bits of quantize_mla_latent_fp8 -- into the
    rows cache_seqlens[b] + i before attention.  cache_seqlens is not modified.

    indices is that of mla_sparse_kvcache.flash_attention_mla_kvcache_sparse, word for word: an int32 device tensor
    [B, S_q, topk], topk >= 1, unit stride along topk (batch and row strides are free).  Entry j of (b, i) is a LOGICAL
    position of sequence b -- the key in page block_table[b, idx // page_size], row idx % page_size --, not a pool row.  With
    L_b = cache_seqlens[b] + S_new (clamped to the table's reach), query i of sequence b attends to exactly the entries with
    0 <= idx < L_b and, with is_causal, also idx <= L_b - S_q + i.  Every other entry is skipped: -1 padding, garbage, a
    position behind the query.  An entry that appears twice counts twice.  A visible idx whose table entry is outside
    [0, num_pages) reads as skipped and makes that sequence's result unspecified; nothing outside the pool is touched whatever
    the lists hold, and only the rows a visible entry names are read.  A list may name the rows being appended.

    The host reads no device memory, so a step can be captured in a graph and replayed while indices, cache_seqlens and
    block_table change in place.  Returns O [B, H, S_q, 512] in q's dtype and, with return_lse=True, LSE [B, H, S_q] fp32 in
    natural-log units; a row with no visible entry gets O = 0 and LSE = -inf.  Inference only: an input that requires grad is
    refused."""
    def pool_dtype():
        assert kv_cache.dtype == torch.uint8, \
            "kv_cache must be torch.uint8 [num_pages, page_size, 656]: rows of 512 e4m3 bytes, 4 fp32 scales and 64 RoPE values " \
            "in q's dtype (got %s)" % kv_cache.dtype
    scale = _check_call("flash_attention_mla_kvcache_sparse_fp8",
                        (("q", q), ("kv_cache", kv_cache), ("indices", indices), ("cache_seqlens", cache_seqlens), ("block_table", block_table)), pool_dtype,
                        (("indices", indices), ("block_table", block_table), ("cache_seqlens", cache_seqlens)),
                        (("indices", indices, "kernel"), ("cache_seqlens", cache_seqlens, "kernels"), ("block_table", block_table, "kernels")),
                        softmax_scale, q=q, kv_new=kv_new, out=out)
    O, LSE = _ext.kvcache_mla_sparse_fp8_forward(q, kv_cache, indices, cache_seqlens, block_table, kv_new, bool(is_causal), scale, out)
    return (O, LSE) if return_lse else O
