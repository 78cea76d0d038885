"""MLA decoding over a paged FP8 LATENT cache (include_mla_fp8/mi355fa_kvcache_mla_fp8.h): mla_kvcache.flash_attention_mla_kvcache
over a cache of 656-byte rows -- 512 e4m3 bytes for the latent dims, one fp32 scale per 128 latent dims, and the 64 RoPE values
kept in 16 bits.  It is the row of FlashMLA's FP8 cache and of vLLM's "fp8_ds_mla": 656 bytes per cached token against 1152 in
the 16-bit cache.  A module beside the other decode modules; the native side is csrc/torch_binding_mla_fp8.cpp ->
_mi355fa_mla_fp8_torch.so over libmi355fa.so.  There is NO fallback: a missing library or binding is an ImportError."""
import torch

from mla_kvcache import _check_call
from fp8_token_kvcache import quantize_kv_fp8_per_token
import _mi355fa_mla_fp8_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["quantize_mla_latent_fp8", "dequantize_mla_latent_fp8", "flash_attention_mla_kvcache_fp8", "MLA_FP8_ROW_BYTES"]

MLA_FP8_ROW_BYTES = 656
_D, _DV, _SCALE_OFF, _ROPE_OFF, _BLOCK = 576, 512, 512, 528, 128


def quantize_mla_latent_fp8(kv):
    """kv [..., 576] (fp16 or bf16: 512 latent dims, then 64 RoPE dims) -> rows torch.uint8 [..., 656].

    Bytes [0, 512): the latent dims as OCP e4m3; bytes [512, 528): four fp32 scales, scale j for the dims [128 j, 128 j + 128);
    bytes [528, 656): the 64 RoPE values in kv's dtype, copied bit for bit.  Per 128-dim block the rule of
    fp8_token_kvcache.quantize_kv_fp8_per_token: s = amax / 448 in fp32, and 1.0 where that is not a normal fp32 number (an
    all-zero block, a subnormal quotient); byte = e4m3_rne(clamp(float(x) / s, -448, 448)), -0.0 kept.  NaN and Inf inputs are
    unspecified.  On a CPU tensor these are the bytes and the scale bits the append of flash_attention_mla_kvcache_fp8 writes for
    kv_new; on a device tensor PyTorch may form amax / 448 as amax * (1 / 448), whose last bit can differ -- a valid cache all
    the same, every byte quantised with the scale stored beside it."""
    assert isinstance(kv, torch.Tensor) and kv.dtype in (torch.float16, torch.bfloat16), "kv must be a float16 or bfloat16 tensor"
    assert kv.dim() >= 1 and kv.shape[-1] == _D, "kv's last dim must be 576: 512 latent dims, then 64 RoPE dims (got %d)" % kv.shape[-1]
    kv = kv.detach()
    lead = kv.shape[:-1]
    x8, s = quantize_kv_fp8_per_token(kv[..., :_DV].reshape(*lead, _DV // _BLOCK, _BLOCK))
    rows = torch.empty(*lead, MLA_FP8_ROW_BYTES, dtype=torch.uint8, device=kv.device)
    rows[..., :_SCALE_OFF] = x8.view(torch.uint8).reshape(*lead, _DV)
    rows[..., _SCALE_OFF:_ROPE_OFF] = s.contiguous().view(torch.uint8).reshape(*lead, 16)
    rows[..., _ROPE_OFF:] = kv[..., _DV:].contiguous().view(torch.uint8).reshape(*lead, 128)
    return rows


def dequantize_mla_latent_fp8(rows, dtype, out_dtype=torch.float32):
    """rows torch.uint8 [..., 656] -> [..., 576] in out_dtype (float32 or float64): the latent dims float(byte) * scale, the
    product formed in out_dtype (exact in float64: 4 significant bits times 24; rounded once in float32), then the RoPE values,
    read as `dtype` (float16 or bfloat16)."""
    assert isinstance(rows, torch.Tensor) and rows.dtype == torch.uint8 and rows.dim() >= 1 and rows.shape[-1] == MLA_FP8_ROW_BYTES, \
        "rows must be torch.uint8 [..., 656]"
    assert dtype in (torch.float16, torch.bfloat16), "dtype, the type of the RoPE values, must be float16 or bfloat16"
    assert out_dtype in (torch.float32, torch.float64), "out_dtype must be float32 or float64"
    lead = rows.shape[:-1]
    lat = rows[..., :_SCALE_OFF].contiguous().view(torch.float8_e4m3fn).to(out_dtype).reshape(*lead, _DV // _BLOCK, _BLOCK)
    s = rows[..., _SCALE_OFF:_ROPE_OFF].contiguous().view(torch.float32).to(out_dtype)
    rope = rows[..., _ROPE_OFF:].contiguous().view(dtype).to(out_dtype)
    return torch.cat([(lat * s.unsqueeze(-1)).reshape(*lead, _DV), rope], dim=-1)


def flash_attention_mla_kvcache_fp8(q, kv_cache, cache_seqlens, block_table, kv_new=None, is_causal=False, softmax_scale=None,
                                    return_lse=False, out=None):
    """mla_kvcache.flash_attention_mla_kvcache over an FP8 latent cache: the same contract, word for word, but for the pool.

    q [B, H, S_q, 576], fp16 or bf16, read in place through its batch, head and row strides ([B, S_q, H, 576] goes in as
    q.transpose(1, 2)).

    kv_cache: the pool torch.uint8 [num_pages, page_size, 656] -- ONE latent head, rows as quantize_mla_latent_fp8 writes them,
    the RoPE values in q's dtype --, page_size a positive multiple of 32.  It is read, and appended to, in place through its
    page and row strides; the row stride may exceed 656 bytes as long as it is a multiple of 16, and the pool may be larger than
    4 GiB.  It is never copied.  The key of a token is float(byte) * scale on its 512 latent dims followed by its RoPE values
    (dequantize_mla_latent_fp8); its value is the latent part.  A scale that is not a finite normal number > 0, or a NaN byte,
    below L_b gives unspecified results.

    block_table int32 device tensor [B, max_pages_per_seq] and cache_seqlens int32 device tensor [B] as in
    flash_attention_mla_kvcache: the host reads neither, so a decode step can be captured in a CUDA/HIP graph and replayed while
    both change in place.  Sequence b attends to L_b = cache_seqlens[b] + S_new keys; table entries at or past
    ceil(L_b / page_size) and rows at or past L_b are never read, and nothing outside the pool is touched whatever they hold.

    kv_new [B, S_q, 576] in q's dtype or None: UNQUANTISED rows, quantised on the device -- the bytes and the scale bits of
    quantize_mla_latent_fp8 -- into the rows cache_seqlens[b] + i through the table before attention.  They may cross page
    boundaries; rows past the table, or whose table entry is outside the pool, are dropped.  cache_seqlens is not modified.

    Query i of sequence b sits at position L_b - S_q + i (bottom-right aligned); is_causal hides the keys behind that position
    and is the only mask.  softmax_scale defaults to 576 ** -0.5; DeepSeek passes (128 + 64) ** -0.5 times its mscale.

    Returns O [B, H, S_q, 512] in q's dtype (written through the strides of `out` if one is given), and with return_lse=True
    also LSE [B, H, S_q] fp32 in natural-log units; a row with no visible key gets O = 0 and LSE = -inf.  Inference only."""
    def pool_dtype():
        assert kv_cache.dtype == torch.uint8, \
            "kv_cache must be torch.uint8 [num_pages, page_size, 656]: rows of 512 e4m3 bytes, 4 fp32 scales and 64 RoPE values " \
            "in q's dtype (got %s)" % kv_cache.dtype
    scale = _check_call("flash_attention_mla_kvcache_fp8", (("q", q), ("kv_cache", kv_cache), ("cache_seqlens", cache_seqlens),
                                                             ("block_table", block_table)), pool_dtype,
                        (("block_table", block_table), ("cache_seqlens", cache_seqlens)),
                        (("cache_seqlens", cache_seqlens, "kernels"), ("block_table", block_table, "kernels")), softmax_scale,
                        q=q, kv_new=kv_new, out=out)
    O, LSE = _ext.kvcache_mla_fp8_forward(q, kv_cache, cache_seqlens, block_table, kv_new, bool(is_causal), scale, out)
    return (O, LSE) if return_lse else O
