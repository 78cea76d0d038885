"""Decoding attention over an MXFP4 KV cache (include/mi355fa_kvcache_fp4.h): 4-bit e2m1 elements, two per byte, with one
e8m0 scale byte per 32 elements in a tensor of its own -- OCP Microscaling v1.0, the block-scaled format gfx950 converts in
hardware.  A key of D = 128 costs 68 bytes against 128 in an e4m3 cache and 256 in a bf16 one.  Padded and paged caches,
plain attention and sinks, D = 64 and 128 (packed variable-length queries, and D = 256, are fp4_ragged_kvcache.py's call).  A module beside paged_kvcache.py and ragged_kvcache.py, whose public names are
recorded surfaces; the native side is csrc/torch_binding_fp4.cpp -> _mi355fa_fp4_torch.so over libmi355fa.so.  There is NO
fallback: a missing library or binding is an ImportError."""
import torch

from My_FlashAttention_optimized import _gqa_window
from paged_kvcache import _check_no_grad, _check_page
import _mi355fa_fp4_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["quantize_kv_mxfp4", "dequantize_kv_mxfp4", "flash_attention_kvcache_fp4", "flash_attention_kvcache_fp4_paged"]

_BLOCK = 32                                          # elements that share one scale
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)    # the magnitudes of codes 0..7; bit 3 is the sign
# the midpoints between neighbouring magnitudes, and whether the tie at each goes up: to the code with mantissa bit 0
_MID = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False))


def quantize_kv_mxfp4(x):
    """x [..., D] (fp16, bf16 or fp32; D a multiple of 32) -> (packed uint8 [..., D/2], scales uint8 [..., D/32]).

    Per block of 32 consecutive elements: amax = max |x|; X = floor(log2(amax)) - 2; e = clamp(X + 127, 0, 254), the e8m0
    scale byte, 2^(e - 127); each element is x / 2^(e - 127) rounded to nearest even onto the e2m1 grid
    +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, saturating at +-6, -0.0 staying -0.0.  A block with amax = 0 gets e = 127 and all nibbles
    0.  Element 2i goes to the low nibble of byte i, 2i + 1 to the high one (torch.float4_e2m1fn_x2's packing).  NaN and
    Inf inputs are unspecified.  These are the bytes the append of flash_attention_kvcache_fp4 writes for k_new / v_new."""
    assert isinstance(x, torch.Tensor) and x.dtype in (torch.float16, torch.bfloat16, torch.float32), \
        "x must be a float16, bfloat16 or float32 tensor"
    D = x.shape[-1]
    assert x.dim() >= 1 and D >= _BLOCK and D % _BLOCK == 0, "the last dimension must be a positive multiple of 32"
    xb = x.detach().float().reshape(*x.shape[:-1], D // _BLOCK, _BLOCK)
    amax = xb.abs().amax(dim=-1)
    # floor(log2(amax)) from the exponent field (every fp16 / bf16 value is a normal fp32 number but the bf16 subnormals,
    # whose field 0 the clamp takes to e = 0 as it would their true exponent)
    field = (amax.contiguous().view(torch.int32) >> 23) & 0xFF
    e = (field - 2).clamp(0, 254)
    e = torch.where(amax == 0, torch.full_like(e, 127), e)
    y = xb.abs() * torch.ldexp(torch.ones_like(amax), 127 - e).unsqueeze(-1)   # exact: a power of two
    code = torch.zeros_like(y, dtype=torch.int32)
    for mid, up in _MID:
        code += (y >= mid) if up else (y > mid)
    sign = (torch.signbit(xb) & (amax != 0).unsqueeze(-1)).to(torch.int32) << 3
    code = (code | sign).reshape(*x.shape[:-1], D // 2, 2)
    packed = (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8)
    return packed, e.to(torch.uint8)


def dequantize_kv_mxfp4(packed, scales, dtype):
    """(packed [..., D/2], scales [..., D/32]) -> [..., D] in `dtype`: e2m1(nibble) * 2^(scale byte - 127), the products
    formed exactly in fp32 and then converted.  packed may be uint8 or torch.float4_e2m1fn_x2, scales uint8 or
    torch.float8_e8m0fnu."""
    packed, scales = _as_bytes(packed), _as_bytes(scales)
    D = packed.shape[-1] * 2
    assert D % _BLOCK == 0 and scales.shape[-1] == D // _BLOCK and scales.shape[:-1] == packed.shape[:-1], \
        "packed must be [..., D/2] and scales [..., D/32]"
    p = packed.to(torch.int32)
    code = torch.stack((p & 0xF, p >> 4), dim=-1).reshape(*packed.shape[:-1], D)
    lut = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float32, device=packed.device)
    val = lut[code].reshape(*packed.shape[:-1], D // _BLOCK, _BLOCK)
    out = torch.ldexp(val, (scales.to(torch.int32) - 127).unsqueeze(-1))
    return out.reshape(*packed.shape[:-1], D).to(dtype)


def _as_bytes(t):
    """an MXFP4 cache (uint8 or torch.float4_e2m1fn_x2) or its scales (uint8 or torch.float8_e8m0fnu) as a uint8 view"""
    assert isinstance(t, torch.Tensor) and t.dtype in (torch.uint8, torch.float4_e2m1fn_x2, torch.float8_e8m0fnu), \
        "MXFP4 caches are uint8 or torch.float4_e2m1fn_x2 and their scales uint8 or torch.float8_e8m0fnu (got %s)" % (
            t.dtype if isinstance(t, torch.Tensor) else type(t))
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def _call(fn, q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, block_table, k_new, v_new, is_causal, window_size,
          softmax_scale, return_lse, sinks):
    wl, wr = _gqa_window(is_causal, window_size)
    for name, t in (("q", q), ("cache_seqlens", cache_seqlens)):
        assert isinstance(t, torch.Tensor), name + " must be a tensor"
    kc, vc, ks, vs = _check_formats(k_cache, v_cache, k_scale, v_scale)
    assert q.dim() == 4 and q.shape[-1] in (64, 128), \
        "q must be [B, H, S_q, D] with D = 64 or 128: an MXFP4 cache has no D = %d kernel" % q.shape[-1]
    scale = _check_scale_and_new(softmax_scale, k_new, v_new)
    _check_no_grad(fn, q=q, k_new=k_new, v_new=v_new, sinks=sinks)
    O, LSE = _ext.kvcache_fp4_forward(q, kc, vc, ks, vs, cache_seqlens, block_table, k_new, v_new, wl, wr, scale, sinks)
    return (O, LSE) if return_lse else O


def _check_formats(k_cache, v_cache, k_scale, v_scale):
    """the dtypes of an MXFP4 cache and its scales; all four as uint8 views (fp4_ragged_kvcache.py shares this and the next)"""
    assert k_cache.dtype in (torch.uint8, torch.float4_e2m1fn_x2) and v_cache.dtype == k_cache.dtype, \
        "k_cache and v_cache must both be uint8 or torch.float4_e2m1fn_x2"
    assert k_scale.dtype in (torch.uint8, torch.float8_e8m0fnu) and v_scale.dtype == k_scale.dtype, \
        "k_scale and v_scale must both be uint8 or torch.float8_e8m0fnu"
    return tuple(_as_bytes(t) for t in (k_cache, v_cache, k_scale, v_scale))


def _check_block_table(block_table):
    """the front of a quantised cache's _paged call (fp8_token_kvcache.py and quant_softcap_kvcache.py share it)"""
    assert isinstance(block_table, torch.Tensor) and block_table.dtype == torch.int32 and block_table.dim() == 2, \
        "block_table must be an int32 tensor [B, max_pages_per_seq]"


def _check_scale_and_new(softmax_scale, k_new, v_new):
    """softmax_scale as the binding takes it (0.0: 1/sqrt(D)), and k_new with v_new (every quantised cache's call shares it)"""
    if softmax_scale is not None:
        softmax_scale = float(softmax_scale)
        assert softmax_scale > 0.0 and softmax_scale != float("inf"), "softmax_scale must be finite and > 0"
    assert (k_new is None) == (v_new is None), "k_new and v_new must be given together"
    return 0.0 if softmax_scale is None else softmax_scale


def flash_attention_kvcache_fp4(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, k_new=None, v_new=None,
                                is_causal=False, window_size=(-1, -1), softmax_scale=None, return_lse=False, sinks=None):
    """flash_attention_kvcache over an MXFP4 cache.

    q [B, H, S_q, D], fp16 or bf16, D in {64, 128}.  k_cache, v_cache [B, H_kv, S_cache, D/2], uint8 or
    torch.float4_e2m1fn_x2: e2m1 nibbles, element 2i in the low nibble of byte i.  k_scale, v_scale
    [B, H_kv, S_cache, D/32], uint8 or torch.float8_e8m0fnu: one e8m0 byte per 32 elements, so that
    K[b, hk, j, d] = e2m1(nibble) * 2^(k_scale[b, hk, j, d // 32] - 127) (dequantize_kv_mxfp4).  All four are read -- and
    appended to -- in place through their strides ([B, S_cache, H_kv, .] storage goes in as .transpose(1, 2)) and are never
    copied; one the kernels cannot address is refused.  There is no per-tensor descale.

    cache_seqlens: int32 device tensor [B]; the host never reads it, so a step can be captured in a graph.  k_new, v_new
    [B, H_kv, S_new, D] (both or neither, q's dtype): quantised on the device, exactly as quantize_kv_mxfp4 does, into the
    rows [cache_seqlens[b], cache_seqlens[b] + S_new) of the caches and of the scales before attention.  is_causal,
    window_size, softmax_scale, return_lse as in flash_attention_kvcache; sinks: (H,) fp32 logits as in
    flash_attention_kvcache_sink, or None.

    The kernel converts nibbles and scales to q's dtype without rounding wherever q's dtype represents the product, so the
    result is flash_attention_kvcache's on the dequantised cache.  Returns O [B, H, S_q, D] (and LSE [B, H, S_q] fp32 with
    return_lse=True).  Inference only: an input that requires grad is refused."""
    return _call("flash_attention_kvcache_fp4", q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, None, k_new, v_new,
                 is_causal, window_size, softmax_scale, return_lse, sinks)


def flash_attention_kvcache_fp4_paged(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, block_table, k_new=None,
                                      v_new=None, is_causal=False, window_size=(-1, -1), softmax_scale=None, return_lse=False,
                                      sinks=None):
    """flash_attention_kvcache_fp4 over paged pools: k_cache, v_cache [num_pages, H_kv, page_size, D/2] and k_scale, v_scale
    [num_pages, H_kv, page_size, D/32], page_size a positive multiple of 32; block_table int32 device tensor
    [B, max_pages_per_seq] as in flash_attention_kvcache_paged: key j of sequence b is row j % page_size of page
    block_table[b, j // page_size], in the caches and in the scales.  Entries at or past ceil(L_b / page_size) are never
    read; an entry outside [0, num_pages) below that makes that sequence's result unspecified, but nothing outside the
    pools is touched and an appended row that would land there is dropped.  Appended rows may cross pages.  The result has
    the bits of flash_attention_kvcache_fp4 on the gathered cache."""
    _check_block_table(block_table)
    assert block_table.is_cuda, "block_table must be a device tensor: the kernels read it, the host never does"
    _check_page(k_cache)
    return _call("flash_attention_kvcache_fp4_paged", q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, block_table,
                 k_new, v_new, is_causal, window_size, softmax_scale, return_lse, sinks)
