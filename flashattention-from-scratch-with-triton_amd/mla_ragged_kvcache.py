"""MLA (multi-head latent attention) decoding over a paged latent cache with PACKED VARIABLE-LENGTH QUERIES
(include_mla_ragged/mi355fa_ragged_mla.h): one call for a step of continuous batching over DeepSeek-V2 / V3 / R1 or Kimi-K2, in
which some sequences decode one token, some verify an MTP draft of a few tokens and some run a chunk of their prefill.  A module
beside mla_kvcache.py, whose public names are a recorded surface; the native side is csrc/torch_binding_mla_ragged.cpp ->
_mi355fa_mla_ragged_torch.so over libmi355fa.so.  There is NO fallback: a missing library or binding is an ImportError."""
import torch

from paged_kvcache import _check_no_grad
import _mi355fa_mla_ragged_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["flash_attention_mla_kvcache_ragged"]


def flash_attention_mla_kvcache_ragged(q, kv_cache, cu_seqlens_q, cache_seqlens, block_table, kv_new=None, is_causal=False,
                                       softmax_scale=None, return_lse=False, out=None):
    """mla_kvcache.flash_attention_mla_kvcache with a query count per sequence.

    q [total_q, H, 576], fp16 or bf16: the absorbed queries of all sequences packed along the first dimension (dims [0, 512) the
    no-RoPE part, dims [512, 576) the RoPE part), read in place through its row and head strides, so a slice of a wider
    projection goes in without a copy.  cu_seqlens_q: int32 device tensor [B + 1]; sequence b owns the rows [cu[b], cu[b + 1]),
    S_b of them (0 is allowed).  Rows at or past cu[B] are padding -- the tail of a graph-captured step: they are never read,
    and the matching rows of the result and of LSE are never written.  There is no max_seqlen_q: the launch is sized from
    total_q and B, and a list of the step's row blocks is built on the device.

    kv_cache: the pool [num_pages, page_size, 576] of flash_attention_mla_kvcache -- ONE latent head, q's dtype, page_size a
    positive multiple of 32, read and appended to in place through its page and row strides, never copied.  block_table: int32
    device tensor [B, max_pages_per_seq]; cache_seqlens: int32 device tensor [B]; both exactly as there.  The host reads none
    of cu_seqlens_q, cache_seqlens and block_table: a step captured at a fixed total_q and B replays while all three change in
    place.  Whatever cu_seqlens_q holds, nothing outside q, out, LSE and the pool is touched; sequences whose rows are not
    their own (a descending, negative or too large entry) get unspecified results.

    Query i of sequence b sits at position L_b - S_b + i (bottom-right aligned), with L_b = cache_seqlens[b], or
    cache_seqlens[b] + S_b when kv_new [total_q, 576] (q's dtype) is given: each query row brings its cached row, and packed
    row cu[b] + i is written to cache row cache_seqlens[b] + i of sequence b through the table before attention (rows past the
    table, or whose table entry is outside the pool, are dropped; cache_seqlens is not modified).  is_causal hides the keys
    behind a query's position and is the only mask.  softmax_scale defaults to 576 ** -0.5; DeepSeek passes (128 + 64) ** -0.5
    times its mscale -- give it explicitly.

    out: optional, [total_q, H, 512] in q's dtype, written in place through its strides; otherwise a contiguous tensor is
    allocated.  Returns O [total_q, H, 512] (and LSE [H, total_q] fp32, natural-log units, with return_lse=True); a row with no
    visible key gets O = 0 and LSE = -inf.  The rows of sequence b have the bits of flash_attention_mla_kvcache on that
    sequence alone.  Inference only: an input that requires grad is refused.  There is no fallback."""
    for name, t in (("q", q), ("kv_cache", kv_cache), ("cu_seqlens_q", cu_seqlens_q), ("cache_seqlens", cache_seqlens),
                    ("block_table", block_table)):
        assert isinstance(t, torch.Tensor), name + " must be a tensor"
    for name, t in (("kv_new", kv_new), ("out", out)):
        assert t is None or isinstance(t, torch.Tensor), name + " must be a tensor or None"
    assert cu_seqlens_q.dtype == torch.int32, "cu_seqlens_q must be int32 (got %s)" % cu_seqlens_q.dtype
    assert cu_seqlens_q.dim() == 1 and cu_seqlens_q.numel() >= 2, \
        "cu_seqlens_q must be a vector of B + 1 entries, B >= 1 (got shape %s)" % (tuple(cu_seqlens_q.shape),)
    B = cu_seqlens_q.numel() - 1
    assert block_table.dtype == torch.int32, "block_table must be int32 (got %s)" % block_table.dtype
    assert block_table.dim() == 2 and block_table.shape[0] == B, \
        "block_table must be [B, max_pages_per_seq] with B = %d, the sequences of cu_seqlens_q" % B
    assert cache_seqlens.dtype == torch.int32, "cache_seqlens must be int32 (got %s)" % cache_seqlens.dtype
    assert cache_seqlens.dim() == 1 and cache_seqlens.numel() == B, \
        "cache_seqlens must have B = %d entries, the sequences of cu_seqlens_q" % B
    assert cu_seqlens_q.is_cuda, "cu_seqlens_q must be a device tensor: the kernels read it, the host never does"
    assert cache_seqlens.is_cuda, "cache_seqlens must be a device tensor: the kernels read it, the host never does"
    assert block_table.is_cuda, "block_table must be a device tensor: the kernels read it, the host never does"
    if softmax_scale is not None:
        softmax_scale = float(softmax_scale)
        assert softmax_scale > 0.0 and softmax_scale != float("inf"), "softmax_scale must be finite and > 0"
    _check_no_grad("flash_attention_mla_kvcache_ragged", q=q, kv_cache=kv_cache, kv_new=kv_new, out=out)
    O, LSE = _ext.kvcache_mla_ragged_forward(q, kv_cache, cu_seqlens_q, cache_seqlens, block_table, kv_new, bool(is_causal),
                                             0.0 if softmax_scale is None else softmax_scale, out)
    return (O, LSE) if return_lse else O
