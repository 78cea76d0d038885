"""ctypes binding of libmi355fa.so (C ABI declared in include/mi355fa.h).

This is the only place the Python host touches native code.  There is NO fallback: if the
shared library is missing or does not export the expected ABI, importing this module
raises, and every caller fails loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi355fa.so")

ABI_VERSION = 7
FP16, BF16 = 0, 1
ERR_WINDOW = -7   # include/mi355fa_local.h: a window value below -1
ERR_GROUP = -8    # include/mi355fa_gqa.h: H_kv < 1 or H not a multiple of H_kv
ERR_WORKSPACE = -9   # include/mi355fa_kvcache.h: a workspace below fa_fwd_kvcache_workspace_bytes
ERR_SOFTCAP = -10    # include/mi355fa_softcap.h: softcap not finite and > 0
ERR_ALIBI = -11      # include/mi355fa_alibi.h: slopes_batch_stride negative, 0 < stride < H, or too large
ERR_PAGED = -12      # include/mi355fa_paged.h: page size, page counts, table stride or a combination of mods
ERR_RAGGED = -13     # include/mi355fa_ragged.h: total_q, B, or a stride of the packed q / o

_vp, _i, _f, _u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_ulonglong
_sp = ctypes.POINTER(ctypes.c_longlong)   # const long long* strides (3 element strides) or NULL

class Opts(ctypes.Structure):
    """mi355fa_opts (include/mi355fa.h): strides, cu_seqlens and dropout in any combination for the fa_*_ex entry points.
    `Opts.make(...)` zero-initialises and sets `size`."""
    _fields_ = ([("size", ctypes.c_uint)] +
                [(n, _sp) for n in ("q_strides", "k_strides", "v_strides", "o_strides", "dout_strides", "dq_strides",
                                    "dk_strides", "dv_strides")] +
                [("cu_seqlens_q", _vp), ("cu_seqlens_k", _vp), ("total_q", _i), ("total_k", _i),
                 ("p_drop", _f), ("seed", _u64), ("offset", _u64), ("q_scaled", _vp)])

    @classmethod
    def make(cls, **kw):
        o = cls()
        o.size = ctypes.sizeof(cls)
        for k, v in kw.items():
            setattr(o, k, v)
        return o


_op = ctypes.POINTER(Opts)

# name -> (restype, argtypes); mirrors include/mi355fa.h one to one
SIGNATURES = {
    "fa_abi_version": (_i, []),
    "fa_last_error": (ctypes.c_char_p, []),
    "fa_supported": (_i, [_i, _i]),
    "fa_fwd": (_i, [_vp] * 5 + [_i] * 7 + [_f, _vp]),
    "fa_bwd_dq": (_i, [_vp] * 8 + [_i] * 7 + [_f, _vp]),
    "fa_bwd_dkv": (_i, [_vp] * 8 + [_i] * 7 + [_f, _vp]),
    # strided tensors: (ptr, strides) pairs for q, k, v, (o), (dout) and for the outputs o / dq / dk / dv
    "fa_fwd_strided": (_i, [_vp, _sp] * 4 + [_vp] + [_i] * 7 + [_f, _vp]),
    "fa_bwd_dq_strided": (_i, [_vp, _sp] * 5 + [_vp] + [_vp, _sp] + [_vp] + [_i] * 7 + [_f, _vp]),
    "fa_bwd_dkv_strided": (_i, [_vp, _sp] * 4 + [_vp] * 2 + [_vp, _sp] * 2 + [_i] * 7 + [_f, _vp]),
    # variable-length: packed [total, H, D] tensors, then cu_seqlens_q, cu_seqlens_k (device int32), then
    # batch, H, total_q, total_k, max_seqlen_q, max_seqlen_k, D, dtype, causal, scale, stream
    "fa_fwd_varlen": (_i, [_vp] * 5 + [_vp] * 2 + [_i] * 9 + [_f, _vp]),
    "fa_bwd_dq_varlen": (_i, [_vp] * 8 + [_vp] * 2 + [_i] * 9 + [_f, _vp]),
    "fa_bwd_dkv_varlen": (_i, [_vp] * 8 + [_vp] * 2 + [_i] * 9 + [_f, _vp]),
    # attention dropout: the fixed-length signatures + p_drop (float), seed, offset (unsigned long long), stream
    "fa_dropout_keep_scale": (_f, [_f]),
    "fa_fwd_dropout": (_i, [_vp] * 5 + [_i] * 7 + [_f, _f, _u64, _u64, _vp]),
    "fa_bwd_dq_dropout": (_i, [_vp] * 8 + [_i] * 7 + [_f, _f, _u64, _u64, _vp]),
    "fa_bwd_dkv_dropout": (_i, [_vp] * 8 + [_i] * 7 + [_f, _f, _u64, _u64, _vp]),
    # general form: the plain signatures + const mi355fa_opts* (NULL = plain launch), stream
    "fa_fwd_ex": (_i, [_vp] * 5 + [_i] * 7 + [_f, _op, _vp]),
    "fa_bwd_dq_ex": (_i, [_vp] * 8 + [_i] * 7 + [_f, _op, _vp]),
    "fa_bwd_dkv_ex": (_i, [_vp] * 8 + [_i] * 7 + [_f, _op, _vp]),
    # sliding window (include/mi355fa_local.h): the _ex signatures without `causal`, + window_left, window_right
    "fa_fwd_local": (_i, [_vp] * 5 + [_i] * 6 + [_f, _i, _i, _op, _vp]),
    "fa_bwd_dq_local": (_i, [_vp] * 8 + [_i] * 6 + [_f, _i, _i, _op, _vp]),
    "fa_bwd_dkv_local": (_i, [_vp] * 8 + [_i] * 6 + [_f, _i, _i, _op, _vp]),
    # grouped-query attention (include/mi355fa_gqa.h): the _local signatures + H_kv after H
    "fa_fwd_gqa": (_i, [_vp] * 5 + [_i] * 7 + [_f, _i, _i, _op, _vp]),
    "fa_bwd_dq_gqa": (_i, [_vp] * 8 + [_i] * 7 + [_f, _i, _i, _op, _vp]),
    "fa_bwd_dkv_gqa": (_i, [_vp] * 8 + [_i] * 7 + [_f, _i, _i, _op, _vp]),
    # decoding over a padded KV cache (include/mi355fa_kvcache.h): q, k_cache, v_cache, k_new, v_new, cache_seqlens, o,
    # lse, workspace, workspace_bytes, then B, H, H_kv, S_q, S_cache, S_new, D, dtype, scale, window_left, window_right
    "fa_fwd_kvcache_workspace_bytes": (ctypes.c_longlong, [_i] * 7),
    "fa_fwd_kvcache": (_i, [_vp] * 9 + [ctypes.c_longlong] + [_i] * 8 + [_f, _i, _i, _op, _vp]),
}

# logit soft-capping (include/mi355fa_softcap.h): the _gqa and fa_fwd_kvcache signatures + softcap after scale.  A table of
# its own: SIGNATURES is the table of the four headers before it (tests/test_host_scale.py enumerates it), and
# ALL_SIGNATURES is both.
SOFTCAP_SIGNATURES = {
    "fa_fwd_softcap": (_i, [_vp] * 5 + [_i] * 7 + [_f, _f, _i, _i, _op, _vp]),
    "fa_bwd_dq_softcap": (_i, [_vp] * 8 + [_i] * 7 + [_f, _f, _i, _i, _op, _vp]),
    "fa_bwd_dkv_softcap": (_i, [_vp] * 8 + [_i] * 7 + [_f, _f, _i, _i, _op, _vp]),
    "fa_fwd_kvcache_softcap": (_i, [_vp] * 9 + [ctypes.c_longlong] + [_i] * 8 + [_f, _f, _i, _i, _op, _vp]),
}
# ALiBi (include/mi355fa_alibi.h): the _gqa and fa_fwd_kvcache signatures + (const float* alibi_slopes, long long
# slopes_batch_stride) after scale.  A table of its own for the same reason as SOFTCAP_SIGNATURES.
_ab = [_vp, ctypes.c_longlong]
ALIBI_SIGNATURES = {
    "fa_fwd_alibi": (_i, [_vp] * 5 + [_i] * 7 + [_f] + _ab + [_i, _i, _op, _vp]),
    "fa_bwd_dq_alibi": (_i, [_vp] * 8 + [_i] * 7 + [_f] + _ab + [_i, _i, _op, _vp]),
    "fa_bwd_dkv_alibi": (_i, [_vp] * 8 + [_i] * 7 + [_f] + _ab + [_i, _i, _op, _vp]),
    "fa_fwd_kvcache_alibi": (_i, [_vp] * 9 + [ctypes.c_longlong] + [_i] * 8 + [_f] + _ab + [_i, _i, _op, _vp]),
}
# FP8 (e4m3) KV caches (include/mi355fa_kvcache_fp8.h): fa_fwd_kvcache + (k_descale, v_descale, descale_bstride) after
# cache_seqlens and kv_dtype after dtype.  A table of its own for the same reason as SOFTCAP_SIGNATURES.
KV_FP8_E4M3 = 0
KVCACHE_FP8_SIGNATURES = {
    "fa_fwd_kvcache_fp8_workspace_bytes": (ctypes.c_longlong, [_i] * 7),
    "fa_fwd_kvcache_fp8": (_i, [_vp] * 8 + [ctypes.c_longlong] + [_vp] * 3 + [ctypes.c_longlong] + [_i] * 9 +
                           [_f, _i, _i, _op, _vp]),
}
# Attention sinks (include/mi355fa_sink.h): fa_fwd_gqa, fa_fwd_kvcache and fa_fwd_kvcache_fp8 + (const float* sinks) after
# scale, and fa_bwd_dsink(lse, delta, sinks, dsinks, B, H, S_q, opts, stream).  A table of its own for the same reason.
SINK_SIGNATURES = {
    "fa_fwd_sink": (_i, [_vp] * 5 + [_i] * 7 + [_f, _vp, _i, _i, _op, _vp]),
    "fa_bwd_dsink": (_i, [_vp] * 4 + [_i] * 3 + [_op, _vp]),
    "fa_fwd_kvcache_sink": (_i, [_vp] * 9 + [ctypes.c_longlong] + [_i] * 8 + [_f, _vp, _i, _i, _op, _vp]),
    "fa_fwd_kvcache_fp8_sink": (_i, [_vp] * 8 + [ctypes.c_longlong] + [_vp] * 3 + [ctypes.c_longlong] + [_i] * 9 +
                                [_f, _vp, _i, _i, _op, _vp]),
}
# Paged KV caches (include/mi355fa_paged.h): q, k_pool, v_pool, k_new, v_new, cache_seqlens, block_table, o, lse, workspace,
# workspace_bytes, then B, H, H_kv, S_q, num_pages, page_size, max_pages_per_seq, block_table_stride, S_new, D, dtype,
# cache_dtype, scale, window_left, window_right, mods, opts, stream.  A table of its own for the same reason.
PAGED_CACHE_16BIT, PAGED_CACHE_FP8_E4M3 = 0, 1


class PagedMods(ctypes.Structure):
    """mi355fa_paged_mods (include/mi355fa_paged.h): the score transform and the fp8 descales of a paged call; all zero =
    plain attention."""
    _fields_ = [("softcap", _f), ("alibi_slopes", _vp), ("slopes_batch_stride", ctypes.c_longlong), ("sinks", _vp),
                ("k_descale", _vp), ("v_descale", _vp), ("descale_bstride", ctypes.c_longlong)]


_pm = ctypes.POINTER(PagedMods)
PAGED_SIGNATURES = {
    "fa_fwd_kvcache_paged_workspace_bytes": (ctypes.c_longlong, [_i] * 9),
    "fa_fwd_kvcache_paged": (_i, [_vp] * 10 + [ctypes.c_longlong] + [_i] * 7 + [ctypes.c_longlong] + [_i] * 4 +
                             [_f, _i, _i, _pm, _op, _vp]),
}
# Packed variable-length queries over a paged cache (include/mi355fa_ragged.h): q, k_pool, v_pool, k_new, v_new, cu_seqlens_q,
# cache_seqlens, block_table, o, lse, workspace, workspace_bytes, then total_q, B, H, H_kv, num_pages, page_size,
# max_pages_per_seq, block_table_stride, D, dtype, cache_dtype, scale, window_left, window_right, mods, opts, stream.  A table
# of its own for the same reason.
RAGGED_SIGNATURES = {
    "fa_fwd_kvcache_ragged_workspace_bytes": (ctypes.c_longlong, [_i] * 8),
    "fa_fwd_kvcache_ragged": (_i, [_vp] * 11 + [ctypes.c_longlong] + [_i] * 7 + [ctypes.c_longlong] + [_i] * 3 +
                              [_f, _i, _i, _pm, _op, _vp]),
}
# MXFP4 KV caches (include/mi355fa_kvcache_fp4.h): q, k_cache, v_cache, k_scale, v_scale, k_new, v_new, cache_seqlens, (paged:
# block_table,) k_scale_strides, v_scale_strides, sinks, o, lse, workspace, workspace_bytes, then the integers of
# fa_fwd_kvcache_fp8 (paged: of fa_fwd_kvcache_paged, with kv_dtype for cache_dtype), scale, window_left, window_right, opts,
# stream.  A table of its own for the same reason.
KV_MXFP4 = 1
KVCACHE_FP4_SIGNATURES = {
    "fa_fwd_kvcache_fp4_workspace_bytes": (ctypes.c_longlong, [_i] * 7),
    "fa_fwd_kvcache_fp4": (_i, [_vp] * 8 + [_sp] * 2 + [_vp] * 4 + [ctypes.c_longlong] + [_i] * 9 + [_f, _i, _i, _op, _vp]),
    "fa_fwd_kvcache_fp4_paged_workspace_bytes": (ctypes.c_longlong, [_i] * 8),
    "fa_fwd_kvcache_fp4_paged": (_i, [_vp] * 9 + [_sp] * 2 + [_vp] * 4 + [ctypes.c_longlong] + [_i] * 7 +
                                 [ctypes.c_longlong] + [_i] * 4 + [_f, _i, _i, _op, _vp]),
}
# Packed variable-length queries over paged MXFP4 pools (include/mi355fa_ragged_fp4.h): q, k_pool, v_pool, k_scale, v_scale,
# k_new, v_new, cu_seqlens_q, cache_seqlens, block_table, k_scale_strides, v_scale_strides, sinks, o, lse, workspace,
# workspace_bytes, then the integers of fa_fwd_kvcache_ragged (with kv_dtype for cache_dtype), scale, window_left,
# window_right, opts, stream.  A table of its own for the same reason.
RAGGED_FP4_SIGNATURES = {
    "fa_fwd_kvcache_fp4_ragged_workspace_bytes": (ctypes.c_longlong, [_i] * 7),
    "fa_fwd_kvcache_fp4_ragged": (_i, [_vp] * 10 + [_sp] * 2 + [_vp] * 4 + [ctypes.c_longlong] + [_i] * 7 +
                                  [ctypes.c_longlong] + [_i] * 3 + [_f, _i, _i, _op, _vp]),
}
# Per-token-scaled e4m3 KV caches (include/mi355fa_kvcache_fp8_token.h): the three MXFP4 signatures with float* scales, element
# strides for them and no kv_dtype.  A table of its own for the same reason.
KVCACHE_FP8_TOKEN_SIGNATURES = {
    "fa_fwd_kvcache_fp8_token_workspace_bytes": (ctypes.c_longlong, [_i] * 7),
    "fa_fwd_kvcache_fp8_token": (_i, [_vp] * 8 + [_sp] * 2 + [_vp] * 4 + [ctypes.c_longlong] + [_i] * 8 + [_f, _i, _i, _op, _vp]),
    "fa_fwd_kvcache_fp8_token_paged_workspace_bytes": (ctypes.c_longlong, [_i] * 8),
    "fa_fwd_kvcache_fp8_token_paged": (_i, [_vp] * 9 + [_sp] * 2 + [_vp] * 4 + [ctypes.c_longlong] + [_i] * 7 +
                                       [ctypes.c_longlong] + [_i] * 3 + [_f, _i, _i, _op, _vp]),
    "fa_fwd_kvcache_fp8_token_ragged_workspace_bytes": (ctypes.c_longlong, [_i] * 7),
    "fa_fwd_kvcache_fp8_token_ragged": (_i, [_vp] * 10 + [_sp] * 2 + [_vp] * 4 + [ctypes.c_longlong] + [_i] * 7 +
                                        [ctypes.c_longlong] + [_i] * 2 + [_f, _i, _i, _op, _vp]),
}
# Soft-capped decoding over the quantised caches (include_quant/mi355fa_kvcache_quant_softcap.h): the signatures of fa_fwd_kvcache,
# fa_fwd_kvcache_paged and fa_fwd_kvcache_ragged without cache_dtype and mods, with softcap after scale and the cache struct in
# front of opts; the workspace functions take the format first.  A table of its own for the same reason.
QUANT_E4M3, QUANT_E4M3_TOKEN, QUANT_MXFP4 = 0, 1, 2


class QuantCache(ctypes.Structure):
    """mi355fa_quant_cache (include_quant/mi355fa_kvcache_quant_softcap.h): the format of a call's cache and that format's members"""
    _fields_ = [("format", _i), ("k_descale", _vp), ("v_descale", _vp), ("descale_bstride", ctypes.c_longlong),
                ("k_scale", _vp), ("v_scale", _vp), ("k_scale_strides", _sp), ("v_scale_strides", _sp)]


_qc = ctypes.POINTER(QuantCache)
KVCACHE_QUANT_SOFTCAP_SIGNATURES = {
    "fa_fwd_kvcache_quant_softcap_workspace_bytes": (ctypes.c_longlong, [_i] * 8),
    "fa_fwd_kvcache_quant_softcap": (_i, [_vp] * 9 + [ctypes.c_longlong] + [_i] * 8 + [_f, _f, _i, _i, _qc, _op, _vp]),
    "fa_fwd_kvcache_quant_softcap_paged_workspace_bytes": (ctypes.c_longlong, [_i] * 9),
    "fa_fwd_kvcache_quant_softcap_paged": (_i, [_vp] * 10 + [ctypes.c_longlong] + [_i] * 7 + [ctypes.c_longlong] + [_i] * 3 +
                                           [_f, _f, _i, _i, _qc, _op, _vp]),
    "fa_fwd_kvcache_quant_softcap_ragged_workspace_bytes": (ctypes.c_longlong, [_i] * 8),
    "fa_fwd_kvcache_quant_softcap_ragged": (_i, [_vp] * 11 + [ctypes.c_longlong] + [_i] * 7 + [ctypes.c_longlong] + [_i] * 2 +
                                            [_f, _f, _i, _i, _qc, _op, _vp]),
}
# MLA decoding over a paged latent cache (include_mla/mi355fa_kvcache_mla.h): q, kv_pool, kv_new, cache_seqlens, block_table, o,
# lse, workspace, workspace_bytes, B, H, S_q, num_pages, page_size, max_pages_per_seq, block_table_stride, S_new, dtype, scale,
# causal, q_strides, kv_strides, o_strides, stream.  A table of its own for the same reason.
KVCACHE_MLA_SIGNATURES = {
    "fa_fwd_kvcache_mla_workspace_bytes": (ctypes.c_longlong, [_i] * 6),
    "fa_fwd_kvcache_mla": (_i, [_vp] * 8 + [ctypes.c_longlong] + [_i] * 6 + [ctypes.c_longlong] + [_i] * 2 + [_f, _i] + [_sp] * 3 +
                           [_vp]),
}
# Its packed variable-length form (include_mla_ragged/mi355fa_ragged_mla.h): q, kv_pool, kv_new, cu_seqlens_q, cache_seqlens,
# block_table, o, lse, workspace, workspace_bytes, total_q, B, H, num_pages, page_size, max_pages_per_seq, block_table_stride,
# has_new, dtype, scale, causal, q_strides, kv_strides, o_strides, stream.  A table of its own: KVCACHE_MLA_SIGNATURES is a
# recorded set.
KVCACHE_MLA_RAGGED_SIGNATURES = {
    "fa_fwd_kvcache_mla_ragged_workspace_bytes": (ctypes.c_longlong, [_i] * 5),
    "fa_fwd_kvcache_mla_ragged": (_i, [_vp] * 9 + [ctypes.c_longlong] + [_i] * 6 + [ctypes.c_longlong] + [_i] * 2 + [_f, _i] +
                                  [_sp] * 3 + [_vp]),
}
ALL_SIGNATURES = {**SIGNATURES, **SOFTCAP_SIGNATURES, **ALIBI_SIGNATURES, **KVCACHE_FP8_SIGNATURES, **SINK_SIGNATURES,
                  **PAGED_SIGNATURES, **RAGGED_SIGNATURES, **KVCACHE_FP4_SIGNATURES, **RAGGED_FP4_SIGNATURES,
                  **KVCACHE_FP8_TOKEN_SIGNATURES, **KVCACHE_QUANT_SOFTCAP_SIGNATURES, **KVCACHE_MLA_SIGNATURES,
                  **KVCACHE_MLA_RAGGED_SIGNATURES}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libmi355fa.so not found at %s -- build it first: "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C %s`"
            % (LIB_PATH, os.path.join(_HERE, "csrc")))
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in ALL_SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    got = lib.fa_abi_version()
    if got != ABI_VERSION:
        raise ImportError("libmi355fa.so ABI version %d, host expects %d" % (got, ABI_VERSION))
    return lib


lib = _load()


def strides3(t):
    """ctypes array {batch, head, seq} of element strides for a [B, H, S, D] tensor, or None (= NULL, contiguous)
    when `t` is contiguous.  Callers must have checked `strided_ok(t)` first."""
    if t.is_contiguous():
        return None
    # a size-1 dimension may carry any stride in PyTorch: it is never multiplied by a non-zero index
    return (ctypes.c_longlong * 3)(*(t.stride(i) if t.shape[i] > 1 else 0 for i in range(2)),
                                   t.stride(2) if t.shape[2] > 1 else t.shape[3])


def strided_ok(t):
    """True if the kernels can read `t` in place: 16-byte aligned base, and either contiguous or unit head-dim stride
    with the other strides multiples of 8 elements (16-byte rows; batch / head may be 0), rows not overlapping and one
    (batch, head) slice within 2^31 bytes (include/mi355fa.h).  Anything else is copied by the caller."""
    if t.data_ptr() % 16:
        return False
    if t.is_contiguous():
        return True
    if t.stride(3) != 1:
        return False
    if t.stride(2) < t.shape[3]:
        return False
    if t.shape[2] > 1 and t.stride(2) % 8:
        return False
    if (t.shape[2] - 1) * t.stride(2) * 2 + 2 * t.shape[3] > (1 << 31) - 1:   # 32-bit buffer offsets inside a slice
        return False
    # batch / head strides may be 0: an expanded K/V shared by several heads is read in place
    return all(t.shape[i] == 1 or (t.stride(i) >= 0 and t.stride(i) % 8 == 0) for i in range(2))


def check(rc, what):
    """Non-zero return code -> RuntimeError carrying fa_last_error()."""
    if rc != 0:
        raise RuntimeError("%s failed (code %d): %s" % (what, rc, lib.fa_last_error().decode()))
