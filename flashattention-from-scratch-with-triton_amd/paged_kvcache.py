"""Decoding attention over a PAGED KV cache (include/mi355fa_paged.h): one pool of fixed-size pages and a per-sequence
table of page numbers, the layout vLLM, SGLang and FlashAttention's flash_attn_with_kvcache(block_table=...) keep, read
in place.  A module beside My_FlashAttention_optimized.py, whose public names are a recorded surface; the native side is
csrc/torch_binding_paged.cpp -> _mi355fa_paged_torch.so over libmi355fa.so, which ragged_kvcache.py shares.  There is NO fallback: a missing library or
binding is an ImportError."""
import torch

from My_FlashAttention_optimized import _gqa_window
import _mi355fa_paged_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["flash_attention_kvcache_paged"]


def _check_page(k_cache):
    """the page size of a pool [num_pages, H_kv, page_size, .], whatever it holds: every paged and packed call's check"""
    page = k_cache.shape[2]
    assert page >= 32 and page % 32 == 0, \
        "the page size (k_cache.shape[2] = %d) must be a positive multiple of 32: a 32-key tile may not straddle pages" % page


def _check_variant(k_cache, softmax_scale, softcap, alibi_slopes, sinks, k_descale, v_descale, k_new, v_new):
    """The checks flash_attention_kvcache_paged and ragged_kvcache.flash_attention_kvcache_ragged share, behind those of
    their own geometry: the page size, at most one score transform, what an fp8 pool takes, the ranges of softcap and
    softmax_scale, k_new with v_new.  Returns (softmax_scale, softcap) as the binding takes them: floats, 0.0 for None."""
    _check_page(k_cache)
    given = [n for n, v in (("softcap", softcap), ("alibi_slopes", alibi_slopes), ("sinks", sinks)) if v is not None]
    assert len(given) <= 1, "at most one of softcap, alibi_slopes and sinks may be given (got %s)" % " and ".join(given)
    if k_cache.dtype == torch.float8_e4m3fn:
        assert not given or given == ["sinks"], "an fp8 cache takes sinks only: %s is not supported with it" % given[0]
    else:
        assert k_descale is None and v_descale is None, \
            "k_descale / v_descale belong to a torch.float8_e4m3fn cache (got a %s cache)" % k_cache.dtype
    if softcap is not None:
        softcap = float(softcap)
        assert softcap > 0.0 and softcap != float("inf"), "softcap must be finite and > 0"
    if softmax_scale is not None:
        softmax_scale = float(softmax_scale)
        assert softmax_scale > 0.0 and softmax_scale != float("inf"), "softmax_scale must be finite and > 0"
    assert (k_new is None) == (v_new is None), "k_new and v_new must be given together"
    return 0.0 if softmax_scale is None else softmax_scale, 0.0 if softcap is None else softcap


def _check_no_grad(fn, **tensors):
    """inference only: none of the call's tensors (by argument name, in the call's order) may require grad"""
    grads = [n for n, t in tensors.items() if isinstance(t, torch.Tensor) and t.requires_grad]
    assert not grads, "%s has no backward: %s must not require grad" % (fn, ", ".join(grads))


def flash_attention_kvcache_paged(q, k_cache, v_cache, cache_seqlens, block_table, k_new=None, v_new=None, is_causal=False,
                                  window_size=(-1, -1), softmax_scale=None, return_lse=False, softcap=None,
                                  alibi_slopes=None, sinks=None, k_descale=None, v_descale=None):
    """flash_attention_kvcache -- and its soft-cap, ALiBi, sink and fp8 forms -- over a paged cache.

    q [B, H, S_q, D], fp16 or bf16, D in {64, 128, 256}.  k_cache, v_cache: the pools [num_pages, H_kv, page_size, D], in q's
    dtype or torch.float8_e4m3fn, page_size a positive multiple of 32, H a multiple of H_kv.  A pool is read -- and
    appended to -- in place through its strides: FlashAttention's / vLLM's [num_pages, page_size, H_kv, D] pool goes in
    as pool.transpose(1, 2).  It is never copied; a pool the kernels cannot address (rows not 16-byte aligned, a head dim
    that is not innermost) is refused.  The pool may be larger than 4 GiB.

    block_table: int32 device tensor [B, max_pages_per_seq]; key j of sequence b is row j % page_size of page
    block_table[b, j // page_size].  cache_seqlens: int32 device tensor [B].  The host reads neither, so a decode step
    can be captured in a CUDA/HIP graph and replayed while both change in place.  Sequence b attends to
    L_b = cache_seqlens[b] + S_new keys (at most max_pages_per_seq * page_size); table entries at or past
    ceil(L_b / page_size) are never read.  An entry outside [0, num_pages) below that makes that sequence's result
    unspecified, but nothing outside the pool is touched.

    k_new, v_new [B, H_kv, S_new, D] (both or neither, q's dtype): written to the rows cache_seqlens[b] + j through the
    table before attention -- they may cross page boundaries; an fp8 pool quantises them as
    flash_attention_kvcache_fp8 does.  cache_seqlens itself is not modified.

    is_causal, window_size, softmax_scale, return_lse: as in flash_attention_kvcache (bottom-right aligned masks; a row
    with no visible key gets O = 0 and LSE = -inf).  At most one of softcap (> 0), alibi_slopes ((H,) or (B, H) fp32) and
    sinks ((H,) fp32); an fp8 pool takes sinks only, with k_descale / v_descale ((B, H_kv) or (H_kv,) fp32, None = 1),
    which a 16-bit pool refuses.

    Returns O [B, H, S_q, D] in q's dtype (and LSE [B, H, S_q] fp32 with return_lse=True): bit for bit what the padded
    call returns on the gathered cache [B, H_kv, max_pages_per_seq * page_size, D].  Inference only: an input that
    requires grad is refused."""
    wl, wr = _gqa_window(is_causal, window_size)
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache), ("cache_seqlens", cache_seqlens),
                    ("block_table", block_table)):
        assert isinstance(t, torch.Tensor), name + " must be a tensor"
    assert block_table.dtype == torch.int32, "block_table must be int32 (got %s)" % block_table.dtype
    assert block_table.dim() == 2, "block_table must be [B, max_pages_per_seq]"
    assert q.dim() == 4 and k_cache.dim() == 4 and v_cache.dim() == 4, \
        "q must be [B, H, S_q, D], the pools [num_pages, H_kv, page_size, D]"
    scale, cap = _check_variant(k_cache, softmax_scale, softcap, alibi_slopes, sinks, k_descale, v_descale, k_new, v_new)
    _check_no_grad("flash_attention_kvcache_paged", q=q, k_cache=k_cache, v_cache=v_cache, k_new=k_new, v_new=v_new,
                   alibi_slopes=alibi_slopes, sinks=sinks, k_descale=k_descale, v_descale=v_descale)
    assert block_table.is_cuda, "block_table must be a device tensor: the kernels read it, the host never does"
    O, LSE = _ext.kvcache_paged_forward(q, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, wl, wr, scale, cap,
                                        alibi_slopes, sinks, k_descale, v_descale)
    return (O, LSE) if return_lse else O
