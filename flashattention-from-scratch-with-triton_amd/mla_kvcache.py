"""MLA (multi-head latent attention) decoding over a paged latent cache (include_mla/mi355fa_kvcache_mla.h): the absorbed
decode form of DeepSeek-V2 / V3 / R1 and Kimi-K2, where all H query heads share one cached row of 576 values per token -- 512
latent dims, then 64 RoPE dims -- and the value of a key is the first 512 values of that same row.  A module beside the other
decode modules; the native side is csrc/torch_binding_mla.cpp -> _mi355fa_mla_torch.so over libmi355fa.so.  There is NO
fallback: a missing library or binding is an ImportError."""
import torch

from paged_kvcache import _check_no_grad
import _mi355fa_mla_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["flash_attention_mla_kvcache", "MLA_D", "MLA_DV"]

MLA_D, MLA_DV = 576, 512


def flash_attention_mla_kvcache(q, kv_cache, cache_seqlens, block_table, kv_new=None, is_causal=False, softmax_scale=None,
                                return_lse=False, out=None):
    """Attention of absorbed MLA queries over a paged latent cache, after appending this step's rows to it.

    q [B, H, S_q, 576], fp16 or bf16: dims [0, 512) are the absorbed no-RoPE part, dims [512, 576) the RoPE part.  It is read in
    place through its batch, head and row strides, so a [B, S_q, H, 576] tensor goes in as q.transpose(1, 2).

    kv_cache: the pool [num_pages, page_size, 576] in q's dtype -- ONE latent head --, page_size a positive multiple of 32.  It
    is read, and appended to, in place through its page and row strides; the row stride may exceed 576 elements as long as rows
    stay 16-byte aligned, and the pool may be larger than 4 GiB.  It is never copied.  A padded cache [B, S_cache, 576] with
    S_cache % 32 == 0 goes in as a pool of B pages with block_table = arange(B)[:, None].

    block_table: int32 device tensor [B, max_pages_per_seq]; key j of sequence b is row j % page_size of page
    block_table[b, j // page_size].  cache_seqlens: int32 device tensor [B].  The host reads neither, so a decode step can be
    captured in a CUDA/HIP graph and replayed while both change in place.  Sequence b attends to L_b = cache_seqlens[b] + S_new
    keys (at most max_pages_per_seq * page_size); table entries at or past ceil(L_b / page_size) are never read.  An entry
    outside [0, num_pages) below that makes that sequence's result unspecified, but nothing outside the pool is touched.

    kv_new [B, S_q, 576] or None: written to the rows cache_seqlens[b] + i through the table before attention -- they may cross
    page boundaries; rows past the table, or whose table entry is outside the pool, are dropped.  cache_seqlens itself is not
    modified.

    Query i of sequence b sits at position L_b - S_q + i (bottom-right aligned, as in every decode call here); is_causal hides
    the keys behind that position and is the only mask.  softmax_scale defaults to 576 ** -0.5; DeepSeek passes
    (128 + 64) ** -0.5 times its mscale, the scale of the non-absorbed heads -- give it explicitly.

    Returns O [B, H, S_q, 512] in q's dtype (written through the strides of `out` if one is given), and with return_lse=True
    also LSE [B, H, S_q] fp32 in natural-log units; a row with no visible key gets O = 0 and LSE = -inf.  Inference only: an
    input that requires grad is refused."""
    for name, t in (("q", q), ("kv_cache", kv_cache), ("cache_seqlens", cache_seqlens), ("block_table", block_table)):
        assert isinstance(t, torch.Tensor), name + " must be a tensor"
    for name, t in (("kv_new", kv_new), ("out", out)):
        assert t is None or isinstance(t, torch.Tensor), name + " must be a tensor or None"
    assert block_table.dtype == torch.int32, "block_table must be int32 (got %s)" % block_table.dtype
    assert cache_seqlens.dtype == torch.int32, "cache_seqlens must be int32 (got %s)" % cache_seqlens.dtype
    assert cache_seqlens.is_cuda, "cache_seqlens must be a device tensor: the kernels read it, the host never does"
    assert block_table.is_cuda, "block_table must be a device tensor: the kernels read it, the host never does"
    if softmax_scale is not None:
        softmax_scale = float(softmax_scale)
        assert softmax_scale > 0.0 and softmax_scale != float("inf"), "softmax_scale must be finite and > 0"
    _check_no_grad("flash_attention_mla_kvcache", q=q, kv_cache=kv_cache, kv_new=kv_new, out=out)
    O, LSE = _ext.kvcache_mla_forward(q, kv_cache, cache_seqlens, block_table, kv_new, bool(is_causal),
                                      0.0 if softmax_scale is None else softmax_scale, out)
    return (O, LSE) if return_lse else O
