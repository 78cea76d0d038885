"""The DeepSeek-V3.2 "lightning indexer" over a paged FP8 key cache (include_mla_indexer/mi355fa_mla_indexer.h): for every query
token a score of every cached token, I[t] = sum_h w[h] * ReLU(q_h . k_t) over 64 FP8 index heads of 128 dims, read out of a
second, small FP8 cache (one 128-byte key and one fp32 scale per token) in place by a kernel on the FP8 matrix instructions --
the step that produces the `indices` of mla_sparse_kvcache / mla_sparse_fp8_kvcache.  A module beside the other decode modules;
the native side is csrc/torch_binding_mla_indexer.cpp -> _mi355fa_mla_indexer_torch.so over libmi355fa.so.  There is NO fallback:
a missing library or binding is an ImportError."""
import torch

from paged_kvcache import _check_no_grad
import _mi355fa_mla_indexer_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["mla_indexer_logits_fp8", "mla_indexer_topk", "mla_indexer_select", "mla_indexer_logits_fp8_prefill"]

_BYTES = (torch.float8_e4m3fn, torch.uint8)


def mla_indexer_logits_fp8(q, weights, k_cache, k_scale, cache_seqlens, block_table, k_new=None, is_causal=False, out=None):
    """logits[b, i, t] = k_scale[t] * sum_h weights[b, i, h] * max(0, sum_d q[b, i, h, d] * k[t, d]) over the cached keys of
    sequence b, after quantising this step's keys in.

    q torch.float8_e4m3fn (or its uint8 view) [B, S_q, H_i, 128], H_i a multiple of 16 in [16, 64], read in place through its
    batch, row and head strides when the last dim is contiguous and the strides are multiples of 16 bytes (copied otherwise).
    weights float32 [B, S_q, H_i], any strides: the caller folds q's per-token dequantisation scale, H_i ** -0.5 and the softmax
    scale into it, as the model's code does.  ReLU comes before the weights, which may be negative.

    k_cache e4m3 bytes [num_pages, page_size, 128] and k_scale float32 [num_pages, page_size], page_size a positive multiple of
    32, both read and appended to in place through their page and row strides (k_cache's row stride at least 128 and a multiple
    of 16; the pool may exceed 4 GiB; neither is ever copied).  Two views of ONE buffer with a page stride of page_size * 132
    bytes -- k_cache over the first page_size * 128 bytes of a block, k_scale over the fp32 values behind them -- express the
    "all bytes of a block, then its scales" layout of other stacks.

    cache_seqlens, block_table: int32 device tensors, those of mla_kvcache.flash_attention_mla_kvcache; the host reads
    neither, so a step can be captured in a graph and replayed while both change in place.  L_b = cache_seqlens[b] + S_new.
    Table entries at or past ceil(L_b / page_size) and rows and scales at or past L_b are never read.  An entry outside the pool
    makes that page's logits unspecified; nothing outside the pools is touched.

    k_new [B, S_q, 128] float16 / bfloat16 or None: appended first, to rows cache_seqlens[b] + i through the table (rows may cross
    pages), quantised on the device by the rule of fp8_token_kvcache.quantize_kv_fp8_per_token.  cache_seqlens is not modified.

    Returns float32 [B, S_q, W], W = out.shape[-1] if out is given (written through its batch and row strides), else
    max_pages_per_seq * page_size.  A column is visible when t < L_b and, with is_causal, t <= L_b - S_q + i (bottom-right
    aligned); every other column of [0, W) is exactly -inf, so torch.topk runs on the row as it is.  Any S_q >= 1 is correct; the
    kernel is tuned for S_q <= 4.  Inference only: an input that requires grad is refused."""
    for name, t in (("q", q), ("weights", weights), ("k_cache", k_cache), ("k_scale", k_scale), ("cache_seqlens", cache_seqlens),
                    ("block_table", block_table)):
        assert isinstance(t, torch.Tensor), name + " must be a tensor"
    for name, t in (("k_new", k_new), ("out", out)):
        assert t is None or isinstance(t, torch.Tensor), name + " must be a tensor or None"
    assert q.dtype in _BYTES, "q must be torch.float8_e4m3fn or its uint8 view (got %s)" % q.dtype
    assert k_cache.dtype in _BYTES, "k_cache must be torch.float8_e4m3fn or its uint8 view (got %s)" % k_cache.dtype
    assert weights.dtype == torch.float32, "weights must be float32 (got %s)" % weights.dtype
    assert k_scale.dtype == torch.float32, "k_scale must be float32 (got %s)" % k_scale.dtype
    assert q.dim() == 4 and q.shape[3] == 128, "q must be [B, S_q, H_i, 128] (got %s)" % (tuple(q.shape),)
    assert 16 <= q.shape[2] <= 64 and q.shape[2] % 16 == 0, "H_i (q.shape[2]) must be a multiple of 16 in [16, 64] (got %d)" % q.shape[2]
    assert k_cache.dim() == 3 and k_cache.shape[2] == 128, "k_cache must be [num_pages, page_size, 128] (got %s)" % (tuple(k_cache.shape),)
    assert k_cache.shape[1] >= 32 and k_cache.shape[1] % 32 == 0, \
        "the page size (k_cache.shape[1] = %d) must be a positive multiple of 32" % k_cache.shape[1]
    assert block_table.dtype == torch.int32, "block_table must be int32 (got %s)" % block_table.dtype
    assert cache_seqlens.dtype == torch.int32, "cache_seqlens must be int32 (got %s)" % cache_seqlens.dtype
    assert cache_seqlens.is_cuda, "cache_seqlens must be a device tensor: the kernels read it, the host never does"
    assert block_table.is_cuda, "block_table must be a device tensor: the kernels read it, the host never does"
    _check_no_grad("mla_indexer_logits_fp8", weights=weights, k_scale=k_scale, k_new=k_new, out=out)
    return _ext.indexer_logits_fp8(q, weights, k_cache, k_scale, cache_seqlens, block_table, k_new, bool(is_causal), out)


def mla_indexer_topk(logits, topk):
    """The `indices` of flash_attention_mla_kvcache_sparse / _sparse_fp8 from a logits tensor [B, S_q, W]: plain torch, a few
    lines -- torch.topk over the row, cast to int32, -1 where the picked logit is -inf (a hidden column), and -1 padding where
    topk > W.  Returns int32 [B, S_q, topk].  (The selection kernel is mla_indexer_select below.)"""
    assert isinstance(logits, torch.Tensor) and logits.dim() == 3 and logits.dtype == torch.float32, "logits must be float32 [B, S_q, W]"
    assert int(topk) >= 1, "topk must be >= 1"
    k = min(int(topk), logits.shape[-1])
    val, idx = torch.topk(logits, k, dim=-1)
    idx = torch.where(val == float("-inf"), torch.full_like(idx, -1), idx).to(torch.int32)
    return torch.nn.functional.pad(idx, (0, int(topk) - k), value=-1)


def mla_indexer_select(logits, topk, lengths=None, out=None):
    """The `indices` of flash_attention_mla_kvcache_sparse / _sparse_fp8 from a logits tensor, by a HIP selection kernel
    (include_mla_select/mi355fa_mla_select.h): int32 [B, S_q, topk], per row the best min(topk, #candidates) columns in
    ASCENDING column order -- the sparse kernels' gather then walks the pages in order --, then -1.

    logits float32 device tensor [B, S_q, W], read in place through its batch and row strides (last dim contiguous, rows that do
    not overlap); a row needs no alignment beyond its 4 bytes, so any `out` slice of mla_indexer_logits_fp8 serves.  Never copied.
    lengths None or an int32 device tensor [B]: columns at or past clamp(lengths[b], 0, W) are not read and count as hidden --
    pass the L_b of the logits call.  The host never reads it, so a captured step replays while it changes in place.
    topk an int in [1, 65536].  out None or int32 [B, S_q, topk], written in place through its batch and row strides, every entry
    of every row; with `out` the call allocates nothing.

    A column is a candidate when it is below the row's length and its value is neither -inf nor NaN.  Candidates are ordered by
    value descending (-0.0 == +0.0, +inf an ordinary largest value), ties by lower column first; the result is exact, unique and
    the same bits on every launch.  Rows of W <= 32768 are held in LDS and read from memory once.  Inference only: logits that
    require grad are refused."""
    assert isinstance(logits, torch.Tensor) and logits.dim() == 3 and logits.dtype == torch.float32, "logits must be float32 [B, S_q, W]"
    assert isinstance(topk, int) and 1 <= topk <= 65536, "topk must be an int in [1, 65536] (got %r)" % (topk,)
    assert lengths is None or (isinstance(lengths, torch.Tensor) and lengths.dtype == torch.int32 and lengths.shape == logits.shape[:1]), \
        "lengths must be None or an int32 tensor [B]"
    assert lengths is None or lengths.is_cuda, "lengths must be a device tensor: the kernel reads it, the host never does"
    assert out is None or (isinstance(out, torch.Tensor) and out.dtype == torch.int32 and tuple(out.shape) == (*logits.shape[:2], topk)), \
        "out must be None or an int32 tensor [B, S_q, topk]"
    assert logits.shape[2] == 1 or logits.stride(2) == 1, "logits must have unit stride along W (got %d)" % logits.stride(2)
    _check_no_grad("mla_indexer_select", logits=logits)
    return _ext.indexer_select(logits, topk, lengths, out)


def mla_indexer_logits_fp8_prefill(q, weights, k, k_scale, ks, ke, out=None):
    """The indexer logits of a prefill step (include_mla_indexer_prefill/mi355fa_mla_indexer_prefill.h): one packed query tensor
    over several sequences, one contiguous FP8 key array, a visible key range per query row -- float32 [M, W],

        logits[m, t] = k_scale[t] * sum_h weights[m, h] * max(0, sum_d q[m, h, d] * k[t, d])    for ks[m] <= t < ke[m]
                     = -inf, bit for bit                                                        for every other t in [0, W).

    q torch.float8_e4m3fn (or its uint8 view) [M, H_i, 128], H_i 16, 32, 48 or 64, read in place through its row and head strides
    when the last dim is contiguous and the strides are multiples of 16 bytes (copied otherwise).  weights float32 [M, H_i], any
    non-negative strides: the caller folds q's dequantisation scale, H_i ** -0.5 and the softmax scale into it, as for
    mla_indexer_logits_fp8.  ReLU comes before the weights, which may be negative.

    k e4m3 bytes [N, 128] -- the keys of all sequences gathered into one array, quantised by
    fp8_token_kvcache.quantize_kv_fp8_per_token --, row stride at least 128 and a multiple of 16, read in place and never copied;
    it may exceed 4 GiB.  k_scale float32 [N], any non-negative stride.

    ks, ke contiguous int32 device tensors [M]: the host never reads them, so a captured step replays while both change in place.  The
    kernel clamps both to [0, N]; a row with ke <= ks is all -inf.  No key row or scale outside the union of the ranges has to be
    valid: what a range excludes is masked by a select and never reaches a logit.  The column index is the position in the packed
    k, which is what mla_indexer_select(logits.view(M, 1, -1), topk, lengths=ke) then returns.  Three uses:
        a single causal prompt              ks = 0,        ke = i + 1
        a chunk with cached context         ks = 0,        ke = N - M + i + 1
        several sequences packed            ks = cu_k[s],  ke = cu_k[s] + prior_s + i + 1   (row i of sequence s, prior_s keys cached)

    out None or float32 [M, W], W >= N, written through its row stride (last dim contiguous, rows 4-byte aligned); every column of
    every row is written, columns [N, W) as -inf.  Without out, W = N.  M == 0 launches nothing; N == 0 gives -inf everywhere.
    The result is the same bits on every launch.  Inference only: an input that requires grad is refused."""
    for name, t in (("q", q), ("weights", weights), ("k", k), ("k_scale", k_scale), ("ks", ks), ("ke", ke)):
        assert isinstance(t, torch.Tensor), name + " must be a tensor"
    assert out is None or isinstance(out, torch.Tensor), "out must be a tensor or None"
    assert q.dtype in _BYTES, "q must be torch.float8_e4m3fn or its uint8 view (got %s)" % q.dtype
    assert k.dtype in _BYTES, "k must be torch.float8_e4m3fn or its uint8 view (got %s)" % k.dtype
    assert weights.dtype == torch.float32, "weights must be float32 (got %s)" % weights.dtype
    assert k_scale.dtype == torch.float32, "k_scale must be float32 (got %s)" % k_scale.dtype
    assert q.dim() == 3 and q.shape[2] == 128, "q must be [M, H_i, 128] (got %s)" % (tuple(q.shape),)
    assert q.shape[1] in (16, 32, 48, 64), "H_i (q.shape[1]) must be 16, 32, 48 or 64 (got %d)" % q.shape[1]
    assert tuple(weights.shape) == tuple(q.shape[:2]), "weights must be [M, H_i] (got %s)" % (tuple(weights.shape),)
    assert k.dim() == 2 and k.shape[1] == 128, "k must be [N, 128] (got %s)" % (tuple(k.shape),)
    assert k.shape[0] <= 1 or (k.stride(1) == 1 and k.stride(0) >= 128 and k.stride(0) % 16 == 0), \
        "k is read in place: unit stride along the 128 bytes, a row stride that is a multiple of 16 and at least 128 (got %s)" % (k.stride(),)
    assert tuple(k_scale.shape) == (k.shape[0],), "k_scale must be [N] (got %s)" % (tuple(k_scale.shape),)
    for name, t in (("ks", ks), ("ke", ke)):
        assert t.dtype == torch.int32 and tuple(t.shape) == (q.shape[0],), "%s must be int32 [M] (got %s %s)" % (name, t.dtype, tuple(t.shape))
        assert t.is_cuda, name + " must be a device tensor: the kernel reads it, the host never does"
    assert out is None or (out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == q.shape[0] and out.shape[1] >= k.shape[0]), \
        "out must be None or a float32 tensor [M, W] with W >= N"
    _check_no_grad("mla_indexer_logits_fp8_prefill", weights=weights, k_scale=k_scale, out=out)
    return _ext.indexer_logits_fp8_prefill(q, weights, k, k_scale, ks, ke, out)
