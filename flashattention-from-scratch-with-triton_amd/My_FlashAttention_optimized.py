"""FlashAttention forward/backward for MI355X behind the reference's call surface.

Counterpart of the reference's code/My_FlashAttention_optimized.py: same module name, same
public names, argument order and defaults --

    flash_attention(Q, K, V, is_causal=False) -> O                       (M:169)
    FlashAttentionFunction.forward / .backward                           (M:130-166)
    flash_attention_forward(Q, K, V, is_causal) -> (O, LSE)              (M:14-60)
    flash_attention_backward(Q, K, V, O, dO, LSE, is_causal) -> (dQ, dK, dV)   (M:62-128)
    compare_with_sdpa(Q, K, V, is_causal)                                (M:172-212)

-- but the three Triton launches are three calls into libmi355fa.so (hand-written gfx950
HIP kernels, C ABI in include/mi355fa.h) on PyTorch's current stream.  PyTorch only
provides device memory, the stream and autograd.  There is no Triton and no fallback: on
a machine without the built libraries the import fails.

Host path: the launchers and the autograd function that `flash_attention` uses live in
_mi355fa_torch.so (csrc/torch_binding.cpp: the same checks / allocations / C-ABI calls as the
Python code below, without the interpreter -- at the reference's S = 512 benchmark points a
Python autograd.Function costs more host time per step than the three kernels take).
`FlashAttentionFunction` keeps the reference's Python class (same forward / backward
signatures, M:130-166) on top of the same launchers; _mi355fa.py is the ctypes view of the
C ABI used by the tools and the tests that drive the library directly.

What the per-feature functions share is written once: _checked_scale (the softmax_scale check), _seq_args (fixed length
against varlen), _decode (the guards, binding call and return of the six flash_attention_kvcache* wrappers) and
_twin_forward / _twin_backward (the five Python twins of the C++ autograd function).  A wrapper checks its own argument
(softcap, slopes, sinks) and hands over.
"""
import torch
import torch.nn.functional as F

import _mi355fa as _fa
import _mi355fa_torch as _ext   # raises if the binding was not built (make -C csrc)

_DTYPES = {torch.float16: _fa.FP16, torch.bfloat16: _fa.BF16}

def _in_place(*tensors):
    """The reference makes every input contiguous (M:138-140,156): a 64 MiB copy per tensor at the headline size
    whenever Q/K/V are transposed views of a fused projection ([B,S,H,D] seen as [B,H,S,D]).  The kernels read such
    views in place and write O / dQ / dK / dV in the same storage order (fa_*_strided); only layouts they cannot address (non-unit head-dim stride, rows not 16-byte
    multiples, a base pointer off a 16-byte boundary, K and V with different sequence strides) are still copied --
    into a fresh (hence aligned) allocation."""
    return tuple(t if _fa.strided_ok(t) else t.clone(memory_format=torch.contiguous_format) for t in tensors)


def _kv_in_place(K, V):
    K, V = _in_place(K, V)
    if K.stride(2) != V.stride(2) and K.shape[2] > 1:   # the kernels use one row stride for the K/V pair
        K, V = K.contiguous(), V.contiguous()
    return K, V


def _check_qkv(Q, K, V):
    """The kernels take B and H from Q and address K / V slices as b*stride_b + h*stride_h: a K or V with fewer batches
    or heads would be read past its allocation (the reference's descriptors cover the whole tensor instead).  MQA / GQA
    callers pass K / V expanded to Q's head count (a stride-0 view is read in place).  The ranks and the head dim are
    FlashAttentionFunction's own asserts."""
    assert K.shape[:2] == Q.shape[:2], "K must have Q's batch and head counts (expand shared K/V heads)"
    assert V.shape == K.shape, "K and V must have the same shape"
    assert Q.device == K.device == V.device, "Q, K, V must be on the same device"
    assert Q.dtype == K.dtype == V.dtype


def flash_attention_forward(Q, K, V, is_causal):
    """Allocate O / LSE and enqueue the forward kernel (M:14-60).  Q, K, V: contiguous, or strided views accepted
    by _mi355fa.strided_ok with K and V sharing their sequence stride.  Runs in _mi355fa_torch.forward_launch."""
    return _ext.forward_launch(Q, K, V, bool(is_causal))


def flash_attention_backward(Q, K, V, O, dO, LSE, is_causal):
    """Allocate dQ/dK/dV/delta and enqueue dQ (+delta) then dK/dV (M:62-128): _mi355fa_torch.backward_launch."""
    return _ext.backward_launch(Q, K, V, O, dO, LSE, bool(is_causal))


class FlashAttentionFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Q, K, V, is_causal: bool):
        assert Q.is_cuda and K.is_cuda and V.is_cuda
        assert Q.dtype in (torch.float16, torch.bfloat16)
        assert Q.dtype == K.dtype == V.dtype
        assert Q.shape[-1] == K.shape[-1] == V.shape[-1]
        assert Q.ndim == 4 and K.ndim == 4 and V.ndim == 4
        assert Q.shape[-1] in (64, 128), "head dim must be 64 or 128"
        _check_qkv(Q, K, V)   # beyond M:133-136: the raw-pointer kernels cannot bound a smaller K / V themselves
        if Q.is_contiguous() and K.is_contiguous() and V.is_contiguous() and not (
                (Q.data_ptr() | K.data_ptr() | V.data_ptr()) & 15):
            Q_, K_, V_ = Q, K, V
        else:                         # no copy for views the kernels can read in place (M:138-140 copies them)
            (Q_,) = _in_place(Q)
            K_, V_ = _kv_in_place(K, V)
        O, LSE = flash_attention_forward(Q_, K_, V_, is_causal)
        ctx.save_for_backward(Q_, K_, V_, O, LSE)
        ctx.is_causal = is_causal
        return O

    @staticmethod
    def backward(ctx, dO):
        Q, K, V, O, LSE = ctx.saved_tensors
        dO_ = dO if (dO.is_contiguous() and not dO.data_ptr() & 15) else _in_place(dO)[0]
        dQ, dK, dV = flash_attention_backward(Q, K, V, O, dO_, LSE, ctx.is_causal)
        return dQ, dK, dV, None


def flash_attention(Q, K, V, is_causal=False):
    """M:169-170.  The autograd function behind it is the C++ twin of FlashAttentionFunction (torch_binding.cpp)."""
    return _ext.flash_attention(Q, K, V, bool(is_causal))


def flash_attention_varlen(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal=False,
                           dropout_p=0.0, seed=0, offset=0):
    """Variable-length attention over PACKED sequences -- the extension the reference leaves as an exercise
    (Phase_6.md:119-178: "concatenate the batch into one long sequence and record where each sequence starts").

    Q: [total_q, H, D], K, V: [total_k, H, D] (fp16 / bf16, device); cu_seqlens_*: int32 device vectors of batch + 1
    prefix sums starting at 0; max_seqlen_*: Python ints >= the longest sequence (they size the launch grid).  Returns
    O [total_q, H, D]; differentiable w.r.t. Q, K, V.  Each sequence attends to itself only; is_causal applies each
    sequence's own top-left aligned mask.  No padding is computed: workgroups beyond a sequence's length exit at once.
    dropout_p / seed / offset: attention dropout as in flash_attention_dropout; the mask of sequence b is the one the same
    sequence gets at batch index b of a padded [B, H, S, D] launch with the same (seed, offset)."""
    return _ext.flash_attention_varlen(Q, K, V, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k),
                                       bool(is_causal), float(dropout_p), int(seed), int(offset))


def flash_attention_dropout(Q, K, V, is_causal=False, dropout_p=0.0, seed=0, offset=0):
    """Attention with dropout on the attention weights -- the other extension the reference leaves as an exercise
    (Phase_6.md:54-113): P is masked and rescaled by 1 / (1 - p) inside the tile loop, and the backward regenerates the
    SAME mask from (seed, offset) with Philox4x32-10 instead of storing it (include/mi355fa.h, fa_*_dropout, gives the
    exact counter layout).  Q, K, V: [B, H, S, D] fp16 / bf16 device tensors (strided views are read in place, as in
    flash_attention); dropout_p in [0, 1), quantised to 1/256;
    seed / offset: Python ints (the caller owns the RNG stream: pass a fresh offset per layer and step).  Differentiable
    w.r.t. Q, K, V.  dropout_p = 0 is flash_attention."""
    if dropout_p == 0.0:
        return flash_attention(Q, K, V, is_causal)
    return _ext.flash_attention_dropout(Q, K, V, bool(is_causal), float(dropout_p), int(seed), int(offset))


def flash_attention_local(Q, K, V, window_left, window_right=0):
    """Sliding-window (local) attention, FlashAttention-2's window_size=(left, right): key j is visible from query i iff
    i - window_left <= j <= i + window_right (and j < S_k), top-left aligned like is_causal; -1 leaves that side unbounded,
    so (-1, 0) is causal and (-1, -1) full attention.  Q, K, V: [B, H, S, D] fp16 / bf16 device tensors, D in {64, 128}
    (strided views are read in place, O comes back in Q's memory order); scale 1/sqrt(D).  A query that sees no key gets
    O = 0 (LSE = -inf).  Differentiable w.r.t. Q, K, V.  The kernels (include/mi355fa_local.h) visit only the tiles that
    meet the band: the work scales with the visible pairs (local_attention_flops), not with S_q * S_k."""
    return _ext.flash_attention_local(Q, K, V, int(window_left), int(window_right))


def flash_attention_local_forward(Q, K, V, window_left, window_right):
    """Allocate O / LSE and enqueue the sliding-window forward: _mi355fa_torch.local_forward_launch."""
    return _ext.local_forward_launch(Q, K, V, int(window_left), int(window_right))


def flash_attention_local_backward(Q, K, V, O, dO, LSE, window_left, window_right):
    """Allocate dQ/dK/dV/delta and enqueue the sliding-window dQ (+delta) then dK/dV: _mi355fa_torch.local_backward_launch."""
    return _ext.local_backward_launch(Q, K, V, O, dO, LSE, int(window_left), int(window_right))


def _twin_forward(ctx, launch, Q, K, V, args, extra=()):
    """Forward of the Python twins (FlashAttentionLocalFunction, FlashAttentionGQAFunction, ...): the twin's forward launcher,
    which checks and prepares Q, K, V as the C++ function does.  args: the launcher's arguments after Q, K, V; extra: a
    tensor argument in front of them that is saved for the backward and gets a gradient (flash_attention_sink's sinks)."""
    assert Q.shape[-1] in (64, 128), "head dim must be 64 or 128"   # as the C++ function (the local launchers leave it to the C ABI)
    O, LSE = launch(Q, K, V, *extra, *args)
    ctx.save_for_backward(Q, K, V, O, LSE, *extra)
    ctx.args = args
    return O


def _twin_backward(ctx, launch, dO):
    """Backward of the Python twins: the twin's backward launcher, which returns one gradient per saved input (Q, K, V and
    the extra tensor, if any); no gradient for the arguments after them."""
    Q, K, V, O, LSE, *extra = ctx.saved_tensors
    return (*launch(Q, K, V, O, dO, LSE, *extra, *ctx.args),) + (None,) * len(ctx.args)


class FlashAttentionLocalFunction(torch.autograd.Function):
    """Python twin of the C++ autograd function behind flash_attention_local (torch_binding.cpp FlashAttnFn)."""

    @staticmethod
    def forward(ctx, Q, K, V, window_left, window_right=0):
        return _twin_forward(ctx, flash_attention_local_forward, Q, K, V, (int(window_left), int(window_right)))

    @staticmethod
    def backward(ctx, dO):
        return _twin_backward(ctx, flash_attention_local_backward, dO)


def local_attention_visible_pairs(S_q, S_k, window_left, window_right):
    """Number of (query, key) pairs of one (batch, head) slice that a (window_left, window_right) window leaves visible."""
    total = 0
    for i in range(S_q):
        lo = max(0, i - window_left) if window_left >= 0 else 0
        hi = min(S_k - 1, i + window_right) if window_right >= 0 else S_k - 1
        total += max(0, hi - lo + 1)
    return total


def local_attention_flops(B, H, S_q, S_k, D, window_left, window_right, mode="fwd_bwd"):
    """FLOPs credited to a sliding-window launch: 4 * D per visible (query, key) pair for the forward (QK^T and PV);
    mode "fwd_bwd" is 3.5x that, the convention bench.py uses for full and causal attention."""
    assert mode in ("fwd", "fwd_bwd"), mode
    f = 4.0 * D * B * H * local_attention_visible_pairs(S_q, S_k, window_left, window_right)
    return f if mode == "fwd" else 3.5 * f


def _gqa_window(is_causal, window_size):
    """(window_left, window_right) of a flash_attention_gqa call: is_causal means window_right = 0."""
    wl, wr = (int(w) for w in window_size)
    assert wl >= -1 and wr >= -1, "window_left / window_right must be >= -1 (-1 = unbounded)"   # before is_causal sets wr
    if is_causal:
        assert wr <= 0, "is_causal=True with window_right > 0: the causal mask has window_right = 0"
        wr = 0
    return wl, wr


def _seq_args(cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, given=lambda m: m is not None):
    """The binding's arguments after the window / scale of a training call: none for fixed length (no cu_seqlens); for
    varlen (either one given: the binding refuses a lone one) the cu_seqlens and the then required max_seqlen_q / _k."""
    if cu_seqlens_q is None and cu_seqlens_k is None:
        return ()
    assert given(max_seqlen_q) and given(max_seqlen_k), "varlen: max_seqlen_q and max_seqlen_k are required"
    return cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k)


def flash_attention_gqa(Q, K, V, is_causal=False, window_size=(-1, -1), cu_seqlens_q=None, cu_seqlens_k=None,
                        max_seqlen_q=None, max_seqlen_k=None):
    """Grouped-query attention: Q [B, H, S_q, D], K and V [B, H_kv, S_k, D] with H a multiple of H_kv; query head h
    attends to K/V head h // (H // H_kv) -- repeat_interleave(H // H_kv, dim=1) of K and V, as SDPA's enable_gqa and
    FlashAttention-2 -- without materialising it.  H_kv = 1 is multi-query attention.  fp16 / bf16 device tensors,
    D in {64, 128}, scale 1/sqrt(D); strided views (e.g. [B, S, H, D] buffers seen as [B, H, S, D]) are read in place.

    window_size = (left, right) is flash_attention_local's window ((-1, -1) full attention); is_causal=True sets
    window_right = 0 (it refuses window_right > 0).  Differentiable w.r.t. Q, K, V: dK and dV have K's and V's shape and
    are the sums over each group of query heads, taken in fp32 inside the kernel and rounded once (deterministic).

    Varlen: with cu_seqlens_q / cu_seqlens_k (int32 device vectors of batch + 1 prefix sums) and max_seqlen_q /
    max_seqlen_k, Q is packed [total_q, H, D] and K, V [total_k, H_kv, D], as flash_attention_varlen."""
    wl, wr = _gqa_window(is_causal, window_size)
    return _ext.flash_attention_gqa(Q, K, V, wl, wr, *_seq_args(cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k))


def flash_attention_gqa_forward(Q, K, V, window_left, window_right, cu_seqlens_q=None, cu_seqlens_k=None,
                                max_seqlen_q=0, max_seqlen_k=0):
    """Allocate O / LSE and enqueue the GQA forward: _mi355fa_torch.gqa_forward_launch."""
    return _ext.gqa_forward_launch(Q, K, V, int(window_left), int(window_right), cu_seqlens_q, cu_seqlens_k,
                                   int(max_seqlen_q), int(max_seqlen_k))


def flash_attention_gqa_backward(Q, K, V, O, dO, LSE, window_left, window_right, cu_seqlens_q=None, cu_seqlens_k=None,
                                 max_seqlen_q=0, max_seqlen_k=0):
    """Allocate dQ/dK/dV/delta and enqueue the GQA dQ (+delta) then dK/dV: _mi355fa_torch.gqa_backward_launch."""
    return _ext.gqa_backward_launch(Q, K, V, O, dO, LSE, int(window_left), int(window_right), cu_seqlens_q, cu_seqlens_k,
                                    int(max_seqlen_q), int(max_seqlen_k))


class FlashAttentionGQAFunction(torch.autograd.Function):
    """Python twin of the C++ autograd function behind flash_attention_gqa (torch_binding.cpp FlashAttnFn).
    apply(Q, K, V, window_left, window_right[, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k])."""

    @staticmethod
    def forward(ctx, Q, K, V, window_left, window_right, cu_seqlens_q=None, cu_seqlens_k=None, max_seqlen_q=0,
                max_seqlen_k=0):
        args = (int(window_left), int(window_right), cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k))
        return _twin_forward(ctx, flash_attention_gqa_forward, Q, K, V, args)

    @staticmethod
    def backward(ctx, dO):
        return _twin_backward(ctx, flash_attention_gqa_backward, dO)


def _checked_scale(softmax_scale):
    """softmax_scale of every call but flash_attention_kvcache (which keeps its older check): None, or as a float, finite
    and > 0."""
    if softmax_scale is not None:
        softmax_scale = float(softmax_scale)
        assert softmax_scale > 0.0 and softmax_scale != float("inf"), "softmax_scale must be finite and > 0"
    return softmax_scale


def _kvcache_scale(softmax_scale):
    """flash_attention_kvcache's softmax_scale, in its own wording: None, or as a float, > 0."""
    if softmax_scale is not None:
        softmax_scale = float(softmax_scale)
        assert softmax_scale > 0.0, "softmax_scale must be > 0"
    return softmax_scale


def _decode(name, launch, q, k_cache, v_cache, cache_seqlens, mods, k_new, v_new, is_causal, window_size, softmax_scale,
            return_lse, check_scale=None, fp8=False):
    """The six decode wrappers behind the checks of their own arguments: the window, the guards the wrappers share -- in
    the order each cache format has always run them --, the binding call
    launch(q, k_cache, v_cache, cache_seqlens, *mods, k_new, v_new, window_left, window_right, scale) and the return.
    mods: the call's own arguments (softcap | alibi_slopes | sinks, then for fp8 caches k_descale, v_descale);
    check_scale: for a softmax_scale the wrapper has not checked yet, applied where it always was, behind the device
    check; name: the wrapper, as the "no backward" refusals spell it."""
    wl, wr = _gqa_window(is_causal, window_size)
    if fp8:   # the cache dtype in front of the ranks; k_new / v_new in front of the device check and may not want a gradient
        assert k_cache.dtype == torch.float8_e4m3fn and v_cache.dtype == torch.float8_e4m3fn, \
            "k_cache and v_cache must be torch.float8_e4m3fn (got %s / %s)" % (k_cache.dtype, v_cache.dtype)
        assert q.dim() == 4 and k_cache.dim() == 4, "q must be [B, H, S_q, D], the caches [B, H_kv, S_cache, D]"
        for d, what in zip(mods[-2:], ("k_descale", "v_descale")):
            if d is not None:
                _descale_4d(d, k_cache.shape[0], k_cache.shape[1], what)
                assert not d.requires_grad, what + " must not require grad"
        assert (k_new is None) == (v_new is None), "k_new and v_new must be given together"
        assert not (q.requires_grad or k_cache.requires_grad or v_cache.requires_grad or
                    (k_new is not None and (k_new.requires_grad or v_new.requires_grad))), \
            name + " has no backward: q, the caches, k_new and v_new must not require grad"
    else:
        assert not (q.requires_grad or k_cache.requires_grad or v_cache.requires_grad), \
            name + " has no backward: q, k_cache and v_cache must not require grad"
    assert q.is_cuda and k_cache.is_cuda and v_cache.is_cuda and cache_seqlens.is_cuda, \
        "q, the caches and cache_seqlens must be device tensors"
    if not fp8:
        assert (k_new is None) == (v_new is None), "k_new and v_new must be given together"
    if check_scale is not None:
        softmax_scale = check_scale(softmax_scale)
    O, LSE = launch(q, k_cache, v_cache, cache_seqlens, *mods, k_new, v_new, wl, wr,
                    0.0 if softmax_scale is None else softmax_scale)
    return (O, LSE) if return_lse else O


def flash_attention_kvcache(q, k_cache, v_cache, cache_seqlens, k_new=None, v_new=None, is_causal=False,
                            window_size=(-1, -1), softmax_scale=None, return_lse=False):
    """Decoding attention over a padded KV cache (FlashAttention-2's flash_attn_with_kvcache; include/mi355fa_kvcache.h).

    q [B, H, S_q, D] (S_q >= 1: one token, or a speculative / chunked step); k_cache, v_cache [B, H_kv, S_cache, D],
    fp16 or bf16, D in {64, 128, 256} (256: this and the other KV-cache decode calls only), H a multiple of H_kv: query head
    h reads K/V head h // (H // H_kv), as in
    flash_attention_gqa.  Strided views are read in place, e.g. a [B, S_cache, H_kv, D] cache seen through
    .transpose(1, 2).  cache_seqlens: int32 device tensor [B], the valid rows of each sequence's cache (0 allowed); the
    host never reads it, so a decode step can be captured in a CUDA/HIP graph and replayed as it advances.

    k_new, v_new [B, H_kv, S_new, D] (optional, both or neither): written into cache rows
    [cache_seqlens[b], cache_seqlens[b] + S_new) before attention, which then sees L_b = cache_seqlens[b] + S_new keys
    (S_new = 0 without them).  cache_seqlens itself is not modified: advance it yourself.  The caller guarantees
    L_b <= S_cache; otherwise that sequence's result is unspecified, but nothing outside the caches is touched.

    The mask is bottom-right aligned: query i sits at position p_i = L_b - S_q + i, and key j is visible iff j < L_b,
    (wl < 0 or j >= p_i - wl) and (wr < 0 or j <= p_i + wr), with window_size = (wl, wr) as in flash_attention_local
    (-1 = unbounded on that side).  is_causal=True sets wr = 0 and refuses wr > 0.  A row with no visible key gets O = 0
    and LSE = -inf.  The scale is softmax_scale (> 0), default 1/sqrt(D).

    Returns O [B, H, S_q, D] in q's dtype, and with return_lse=True also LSE [B, H, S_q] (fp32, natural log).
    Inference only: there is no backward, and an input that requires grad is refused.  Deterministic: the same inputs
    give the same bits from run to run, whatever the split count the kernel picks.
    """
    return _decode("flash_attention_kvcache", _ext.kvcache_forward, q, k_cache, v_cache, cache_seqlens, (), k_new, v_new,
                   is_causal, window_size, softmax_scale, return_lse, check_scale=_kvcache_scale)


FP8_E4M3_MAX = 448.0   # the largest finite float8_e4m3fn value


def _descale_4d(descale, B, H_kv, what="descale"):
    """A (B, H_kv) or (H_kv,) fp32 descale tensor as a view that broadcasts over [B, H_kv, S, D]"""
    assert isinstance(descale, torch.Tensor) and descale.dtype == torch.float32, what + " must be a float32 tensor"
    assert tuple(descale.shape) in ((B, H_kv), (H_kv,)), what + " must have shape (B, H_kv) or (H_kv,)"
    return descale.reshape((-1, H_kv, 1, 1))


def quantize_kv_fp8(x, descale=None):
    """Quantise K or V rows [B, H_kv, S, D] (any float dtype, any device) to torch.float8_e4m3fn for
    flash_attention_kvcache_fp8: returns (x8, descale) with x ~ x8.float() * descale[b, hk].

    descale: float32 (B, H_kv) or (H_kv,), > 0; default amax(|x|) over (S, D) / 448 per (b, hk), and 1.0 where that is 0.
    The cast is the one the kernels' append performs, e4m3_rne(clamp(float(x) / descale, -448, 448)): it saturates
    (torch's own cast of a value beyond 448 gives NaN), rounds to nearest even, e4m3 subnormals included, and keeps
    -0.0.  A cache filled through this helper and one filled by appending k_new / v_new hold the same bytes."""
    assert x.dim() == 4, "x must be [B, H_kv, S, D]"
    B, H_kv = x.shape[0], x.shape[1]
    xf = x.float()
    if descale is None:
        amax = xf.abs().amax(dim=(2, 3)) if xf.shape[2] * xf.shape[3] > 0 else xf.new_zeros((B, H_kv))
        descale = amax / FP8_E4M3_MAX
        descale = torch.where(descale > 0, descale, torch.ones_like(descale))
    d4 = _descale_4d(descale, B, H_kv)
    assert d4.device == x.device, "descale must be on x's device"
    x8 = (xf / d4).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX).to(torch.float8_e4m3fn)
    return x8, descale


def flash_attention_kvcache_fp8(q, k_cache, v_cache, cache_seqlens, k_descale=None, v_descale=None, k_new=None,
                                v_new=None, is_causal=False, window_size=(-1, -1), softmax_scale=None, return_lse=False):
    """Decoding attention over a padded KV cache stored as torch.float8_e4m3fn (include/mi355fa_kvcache_fp8.h):
    flash_attention_kvcache on

        K[b, hk, j, :] = k_cache[b, hk, j, :].float() * k_descale[b, hk],   V likewise with v_descale,

    read in place, one byte per element.  q [B, H, S_q, D] is fp16 or bf16 and is not quantised; every e4m3 value is exact
    in q's dtype, so against the dequantised cache the result carries the 16-bit kernel's rounding only.  The caches must
    be torch.float8_e4m3fn (OCP e4m3: float8_e4m3fnuz, float8_e5m2, uint8 and 16-bit caches are refused); a transposed
    [B, S_cache, H_kv, D] cache is read in place when its strides are multiples of 16.  k_descale / v_descale: float32
    device tensors (B, H_kv) or (H_kv,), finite and > 0, None = 1.0; the host never reads them (nor cache_seqlens), so a
    step can be captured in a graph.  quantize_kv_fp8 builds a cache and its descales.

    k_new, v_new [B, H_kv, S_new, D] in q's dtype (both or neither) are quantised with the same descales,
    e4m3_rne(clamp(x.float() / descale, -448, 448)), into cache rows [cache_seqlens[b], cache_seqlens[b] + S_new) before
    attention.  The mask (bottom-right aligned, query i at position L_b - S_q + i), window_size, is_causal, softmax_scale
    and rows with no visible key (O = 0, LSE = -inf) are flash_attention_kvcache's.  Inference only: there is no backward,
    and an input that requires grad is refused.  Deterministic at any split count.
    Returns O [B, H, S_q, D] in q's dtype, and with return_lse=True also LSE [B, H, S_q] (fp32, natural log)."""
    return _decode("flash_attention_kvcache_fp8", _ext.kvcache_fp8_forward, q, k_cache, v_cache, cache_seqlens,
                   (k_descale, v_descale), k_new, v_new, is_causal, window_size, softmax_scale, return_lse,
                   check_scale=_checked_scale, fp8=True)


def _softcap_args(softcap, softmax_scale):
    """softcap and softmax_scale of the soft-capped calls, checked: softcap > 0, softmax_scale None or > 0."""
    softcap = float(softcap)
    assert softcap > 0.0 and softcap != float("inf"), "softcap must be finite and > 0"
    return softcap, _checked_scale(softmax_scale)


def flash_attention_softcap(Q, K, V, softcap, is_causal=False, window_size=(-1, -1), softmax_scale=None, cu_seqlens_q=None,
                            cu_seqlens_k=None, max_seqlen_q=None, max_seqlen_k=None):
    """Attention with logit soft-capping (FlashAttention-2's softcap; Gemma 2 caps at 50, Grok-1 at 30).

    Every score is capped before the masks and the softmax:
        t_ij = tanh(scale * q_i . k_j / softcap),   u_ij = softcap * t_ij,
        P = softmax over the visible j of u_ij,   O = P V,   LSE_i = logsumexp_j u_ij (natural log),
    and the backward is dV = P^T dO, dS_ij = P_ij (dP_ij - delta_i) (1 - t_ij^2), dQ = scale dS K, dK = scale dS^T Q.
    scale = softmax_scale (> 0), default 1/sqrt(D); softcap must be finite and > 0.

    Shapes, masks and varlen are those of flash_attention_gqa: Q [B, H, S_q, D], K and V [B, H_kv, S_k, D] with H a
    multiple of H_kv (H_kv = H is plain multi-head attention), fp16 / bf16 device tensors, D in {64, 128}; strided views are
    read in place.  The mask is top-left aligned: window_size = (left, right) as in flash_attention_local ((-1, -1) full
    attention), is_causal=True sets window_right = 0.  A row with no visible key gets O = 0 (LSE = -inf, dQ = 0).
    Differentiable w.r.t. Q, K, V; dK and dV are summed over each group of query heads.  Dropout is not supported with
    softcap (the C ABI refuses it).  With cu_seqlens_q / cu_seqlens_k and max_seqlen_q / max_seqlen_k, Q is packed
    [total_q, H, D] and K, V [total_k, H_kv, D]."""
    softcap, softmax_scale = _softcap_args(softcap, softmax_scale)
    wl, wr = _gqa_window(is_causal, window_size)
    return _ext.flash_attention_softcap(Q, K, V, softcap, wl, wr, softmax_scale,
                                        *_seq_args(cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k))


def flash_attention_softcap_forward(Q, K, V, softcap, window_left, window_right, softmax_scale=None, cu_seqlens_q=None,
                                    cu_seqlens_k=None, max_seqlen_q=0, max_seqlen_k=0):
    """Allocate O / LSE and enqueue the soft-capped forward: _mi355fa_torch.softcap_forward_launch."""
    return _ext.softcap_forward_launch(Q, K, V, float(softcap), int(window_left), int(window_right), softmax_scale,
                                       cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k))


def flash_attention_softcap_backward(Q, K, V, O, dO, LSE, softcap, window_left, window_right, softmax_scale=None,
                                     cu_seqlens_q=None, cu_seqlens_k=None, max_seqlen_q=0, max_seqlen_k=0):
    """Allocate dQ/dK/dV/delta and enqueue the soft-capped dQ (+delta) then dK/dV: _mi355fa_torch.softcap_backward_launch."""
    return _ext.softcap_backward_launch(Q, K, V, O, dO, LSE, float(softcap), int(window_left), int(window_right),
                                        softmax_scale, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k))


class FlashAttentionSoftcapFunction(torch.autograd.Function):
    """Python twin of the C++ autograd function behind flash_attention_softcap (torch_binding.cpp FlashAttnFn).
    apply(Q, K, V, softcap, window_left, window_right[, softmax_scale, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
    max_seqlen_k])."""

    @staticmethod
    def forward(ctx, Q, K, V, softcap, window_left, window_right, softmax_scale=None, cu_seqlens_q=None, cu_seqlens_k=None,
                max_seqlen_q=0, max_seqlen_k=0):
        softcap, softmax_scale = _softcap_args(softcap, softmax_scale)
        args = (softcap, int(window_left), int(window_right), softmax_scale, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q),
                int(max_seqlen_k))
        return _twin_forward(ctx, flash_attention_softcap_forward, Q, K, V, args)

    @staticmethod
    def backward(ctx, dO):
        return _twin_backward(ctx, flash_attention_softcap_backward, dO)


def flash_attention_kvcache_softcap(q, k_cache, v_cache, cache_seqlens, softcap, k_new=None, v_new=None, is_causal=False,
                                    window_size=(-1, -1), softmax_scale=None, return_lse=False):
    """Decoding attention over a padded KV cache with logit soft-capping: flash_attention_kvcache with every score s
    replaced by u = softcap * tanh(scale * s / softcap) before the masks and the softmax (LSE = logsumexp of u, natural
    log).  softcap must be finite and > 0; scale = softmax_scale (> 0), default 1/sqrt(D).

    Everything else is flash_attention_kvcache: q [B, H, S_q, D], the caches [B, H_kv, S_cache, D], cache_seqlens an int32
    device tensor [B] (0 allowed) that the host never reads, so a step can be captured in a graph; k_new / v_new are
    appended first.  The mask is bottom-right aligned (query i at position L_b - S_q + i), window_size as in
    flash_attention_kvcache, is_causal=True sets window_right = 0.  A row with no visible key gets O = 0 and LSE = -inf.
    Inference only (an input that requires grad is refused); deterministic at any split count.
    Returns O, and with return_lse=True also LSE [B, H, S_q] (fp32)."""
    softcap, softmax_scale = _softcap_args(softcap, softmax_scale)
    return _decode("flash_attention_kvcache_softcap", _ext.kvcache_softcap_forward, q, k_cache, v_cache, cache_seqlens,
                   (softcap,), k_new, v_new, is_causal, window_size, softmax_scale, return_lse)


def alibi_slopes(H, device=None):
    """The ALiBi head slopes of Press et al. (2022), fp32 [H]: for H a power of two the geometric sequence
    2^(-8/H), 2^(-16/H), ..., 2^(-8); otherwise the H' = 2^floor(log2 H) slopes of H' heads followed by every other slope
    of 2H' heads, (the paper's reference code; BLOOM and MPT use it), up to H in all."""
    H = int(H)
    assert H >= 1, "H must be >= 1"

    def pow2(n):
        return [2.0 ** (-8.0 * (i + 1) / n) for i in range(n)]

    p = 1 << (H.bit_length() - 1)
    vals = pow2(p) if p == H else pow2(p) + pow2(2 * p)[0::2][:H - p]
    return torch.tensor(vals, dtype=torch.float32, device=device)


def _alibi_args(alibi_slopes, B, H, device, softmax_scale):
    """Check the slopes of an ALiBi call before anything is launched, in the C++ binding's order: fp32, (H,) or (B, H),
    contiguous, not requiring grad (there is no gradient for them), on `device`.  Returns softmax_scale checked (None
    or finite > 0)."""
    s = alibi_slopes
    assert isinstance(s, torch.Tensor), "alibi_slopes must be a tensor"
    assert s.dtype == torch.float32, "alibi_slopes must be float32"
    assert tuple(s.shape) in ((H,), (B, H)), "alibi_slopes must have shape (H,) or (B, H)"
    assert s.is_contiguous(), "alibi_slopes must be contiguous"
    assert not s.requires_grad, "alibi_slopes must not require grad: there is no gradient for the slopes"
    assert s.device == device, "alibi_slopes must be a device tensor on q's device"
    return _checked_scale(softmax_scale)


def _batch(Q, cu_seqlens_q):
    """B of a training call: Q's batch size, or the number of packed sequences"""
    return Q.shape[0] if cu_seqlens_q is None else cu_seqlens_q.numel() - 1


def flash_attention_alibi(Q, K, V, alibi_slopes, is_causal=False, window_size=(-1, -1), softmax_scale=None,
                          cu_seqlens_q=None, cu_seqlens_k=None, max_seqlen_q=None, max_seqlen_k=None):
    """Attention with an ALiBi position bias (FlashAttention-2's alibi_slopes; BLOOM, MPT, Falcon-RW, Baichuan-13B).

    A per-head linear bias is added to every score before the masks and the softmax:
        s_ij = scale * q_i . k_j - slope_h * |i - j|,
        P = softmax over the visible j of s_ij,   O = P V,   LSE_i = logsumexp_j s_ij (natural log, bias included),
    and the backward is dV = P^T dO, dS = P o (dP - delta), dQ = scale dS K, dK = scale dS^T Q (the bias adds no factor).
    alibi_slopes: float32 device tensor, contiguous, (H,) or (B, H) (B = sequences under varlen), indexed by query head;
    alibi_slopes(H) gives the paper's.  It gets no gradient; one that requires grad is refused.  Any finite slope works,
    0 and negative ones included; NaN or inf slopes give undefined output (their values are never read on the host).
    scale = softmax_scale (> 0), default 1/sqrt(D).

    Query i sits at position i: the mask is top-left aligned, as for every training call here.  This is FA2's
    |i + S_k - S_q - j| whenever S_q = S_k (per sequence).  FA2's causal kernel biases by +slope * j instead, which
    shifts its LSE by a per-row constant; O is the same.

    Shapes, masks and varlen are those of flash_attention_gqa: Q [B, H, S_q, D], K and V [B, H_kv, S_k, D] with H a
    multiple of H_kv, fp16 / bf16, D in {64, 128}, strided views read in place; window_size = (left, right),
    is_causal=True sets window_right = 0.  Differentiable w.r.t. Q, K, V; dK and dV are summed over each group of query
    heads.  Dropout and softcap do not combine with it."""
    softmax_scale = _alibi_args(alibi_slopes, _batch(Q, cu_seqlens_q), Q.shape[-3 if cu_seqlens_q is None else 1],
                                Q.device, softmax_scale)
    wl, wr = _gqa_window(is_causal, window_size)
    return _ext.flash_attention_alibi(Q, K, V, alibi_slopes, wl, wr, softmax_scale,
                                      *_seq_args(cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k))


def flash_attention_alibi_forward(Q, K, V, alibi_slopes, window_left, window_right, softmax_scale=None, cu_seqlens_q=None,
                                  cu_seqlens_k=None, max_seqlen_q=0, max_seqlen_k=0):
    """Allocate O / LSE and enqueue the ALiBi forward: _mi355fa_torch.alibi_forward_launch."""
    return _ext.alibi_forward_launch(Q, K, V, alibi_slopes, int(window_left), int(window_right), softmax_scale,
                                     cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k))


def flash_attention_alibi_backward(Q, K, V, O, dO, LSE, alibi_slopes, window_left, window_right, softmax_scale=None,
                                   cu_seqlens_q=None, cu_seqlens_k=None, max_seqlen_q=0, max_seqlen_k=0):
    """Allocate dQ/dK/dV/delta and enqueue the ALiBi dQ (+delta) then dK/dV: _mi355fa_torch.alibi_backward_launch."""
    return _ext.alibi_backward_launch(Q, K, V, O, dO, LSE, alibi_slopes, int(window_left), int(window_right),
                                      softmax_scale, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k))


class FlashAttentionAlibiFunction(torch.autograd.Function):
    """Python twin of the C++ autograd function behind flash_attention_alibi (torch_binding.cpp FlashAttnFn).
    apply(Q, K, V, alibi_slopes, window_left, window_right[, softmax_scale, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
    max_seqlen_k]); no gradient for the slopes."""

    @staticmethod
    def forward(ctx, Q, K, V, alibi_slopes, window_left, window_right, softmax_scale=None, cu_seqlens_q=None,
                cu_seqlens_k=None, max_seqlen_q=0, max_seqlen_k=0):
        softmax_scale = _alibi_args(alibi_slopes, _batch(Q, cu_seqlens_q), Q.shape[-3 if cu_seqlens_q is None else 1],
                                    Q.device, softmax_scale)
        args = (alibi_slopes, int(window_left), int(window_right), softmax_scale, cu_seqlens_q, cu_seqlens_k,
                int(max_seqlen_q), int(max_seqlen_k))
        return _twin_forward(ctx, flash_attention_alibi_forward, Q, K, V, args)

    @staticmethod
    def backward(ctx, dO):
        return _twin_backward(ctx, flash_attention_alibi_backward, dO)


def flash_attention_kvcache_alibi(q, k_cache, v_cache, cache_seqlens, alibi_slopes, k_new=None, v_new=None,
                                  is_causal=False, window_size=(-1, -1), softmax_scale=None, return_lse=False):
    """Decoding attention over a padded KV cache with an ALiBi bias: flash_attention_kvcache with -slope_h |p_i - j|
    added to every score before the masks and the softmax, p_i = L_b - S_q + i the query's position (bottom-right
    aligned, FA2's convention).  LSE is the logsumexp of the biased scores (natural log).  alibi_slopes: float32 device
    tensor, contiguous, (H,) or (B, H), indexed by query head, never read on the host: a step stays graph-capturable and
    the slopes may change between replays.  scale = softmax_scale (> 0), default 1/sqrt(D).

    Everything else is flash_attention_kvcache: q [B, H, S_q, D], the caches [B, H_kv, S_cache, D], cache_seqlens int32
    [B]; k_new / v_new are appended first; window_size and is_causal as there.  A row with no visible key gets O = 0 and
    LSE = -inf.  Inference only (an input that requires grad is refused); deterministic at any split count.
    Returns O, and with return_lse=True also LSE [B, H, S_q] (fp32)."""
    softmax_scale = _alibi_args(alibi_slopes, q.shape[0], q.shape[1], q.device, softmax_scale)
    return _decode("flash_attention_kvcache_alibi", _ext.kvcache_alibi_forward, q, k_cache, v_cache, cache_seqlens,
                   (alibi_slopes,), k_new, v_new, is_causal, window_size, softmax_scale, return_lse)


def _sink_args(sinks, H, device, softmax_scale, training):
    """Check the sinks of a call before anything is launched, in the C++ binding's order: fp32, (H,), contiguous, on
    `device`; the decoding calls (training False) also refuse sinks that require grad.  Returns softmax_scale checked
    (None or finite > 0)."""
    s = sinks
    assert isinstance(s, torch.Tensor), "sinks must be a tensor"
    assert s.dtype == torch.float32, "sinks must be float32"
    assert tuple(s.shape) == (H,), "sinks must have shape (H,)"
    assert s.is_contiguous(), "sinks must be contiguous"
    assert s.device == device, "sinks must be a device tensor on q's device"
    assert training or not s.requires_grad, "the decoding calls have no backward: sinks must not require grad"
    return _checked_scale(softmax_scale)


def flash_attention_sink(Q, K, V, sinks, is_causal=False, window_size=(-1, -1), softmax_scale=None, cu_seqlens_q=None,
                         cu_seqlens_k=None, max_seqlen_q=0, max_seqlen_k=0):
    """Attention with learned attention sinks (gpt-oss; FlashAttention-3's s_aux, vLLM's sinks; include/mi355fa_sink.h).

    sinks[h] is one extra logit per query head that joins the softmax denominator of every row and carries no value:
        LSE_i = log(exp(sinks[h]) + sum over the visible j of exp(s_ij)),   s_ij = scale * q_i . k_j,
        P_ij = exp(s_ij - LSE_i) (rows sum to less than 1),   O = P V,
    with LSE the natural log, the sink included.  sinks[h] is in natural-log units and is NOT multiplied by scale.  The
    backward is dV = P^T dO, dS = P o (dP - delta), dQ = scale dS K, dK = scale dS^T Q and
        dsinks[h] = -sum over b, i of exp(sinks[h] - LSE_i) * delta_i,   delta_i = dO_i . O_i.
    sinks: float32 device tensor, contiguous, (H,), indexed by query head.  It MAY require grad and then receives dsinks
    as float32 (H,), computed in fp32 in a fixed order (the same bits run after run); when it does not, that kernel is
    not launched.  A row with no visible key gets O = 0, LSE = sinks[h] and dQ = 0.  sinks[h] = -inf is defined: the
    result is flash_attention_gqa's, bit for bit, and dsinks[h] = 0; +inf and NaN give undefined output (the values are
    never read on the host).  scale = softmax_scale (> 0), default 1/sqrt(D).

    Shapes, masks and varlen are those of flash_attention_gqa: Q [B, H, S_q, D], K and V [B, H_kv, S_k, D] with H a
    multiple of H_kv, fp16 / bf16, D in {64, 128}, strided views read in place; window_size = (left, right), top-left
    aligned, is_causal=True sets window_right = 0; with cu_seqlens_q / cu_seqlens_k and max_seqlen_q / max_seqlen_k, Q is
    packed [total_q, H, D] and K, V [total_k, H_kv, D].  Dropout, softcap and ALiBi do not combine with it."""
    varlen = cu_seqlens_q is not None or cu_seqlens_k is not None
    softmax_scale = _sink_args(sinks, Q.shape[1 if varlen else -3], Q.device, softmax_scale, True)
    wl, wr = _gqa_window(is_causal, window_size)
    return _ext.flash_attention_sink(Q, K, V, sinks, wl, wr, softmax_scale,   # max_seqlen_* default to 0 here: 0 is "not given"
                                     *_seq_args(cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, given=bool))


def flash_attention_sink_forward(Q, K, V, sinks, window_left, window_right, softmax_scale=None, cu_seqlens_q=None,
                                 cu_seqlens_k=None, max_seqlen_q=0, max_seqlen_k=0):
    """Allocate O / LSE and enqueue the sink forward: _mi355fa_torch.sink_forward_launch."""
    return _ext.sink_forward_launch(Q, K, V, sinks, int(window_left), int(window_right), softmax_scale, cu_seqlens_q,
                                    cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k))


def flash_attention_sink_backward(Q, K, V, O, dO, LSE, sinks, window_left, window_right, softmax_scale=None,
                                  cu_seqlens_q=None, cu_seqlens_k=None, max_seqlen_q=0, max_seqlen_k=0, need_dsinks=True):
    """Allocate dQ/dK/dV/delta and enqueue the GQA dQ (+delta), the GQA dK/dV and, with need_dsinks, the sink gradient:
    _mi355fa_torch.sink_backward_launch.  Returns (dQ, dK, dV, dsinks); dsinks is None without need_dsinks."""
    return _ext.sink_backward_launch(Q, K, V, O, dO, LSE, sinks, int(window_left), int(window_right), softmax_scale,
                                     cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), bool(need_dsinks))


class FlashAttentionSinkFunction(torch.autograd.Function):
    """Python twin of the C++ autograd function behind flash_attention_sink (torch_binding.cpp FlashAttnFn).
    apply(Q, K, V, sinks, window_left, window_right[, softmax_scale, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
    max_seqlen_k]); sinks gets its gradient when it requires one."""

    @staticmethod
    def forward(ctx, Q, K, V, sinks, window_left, window_right, softmax_scale=None, cu_seqlens_q=None, cu_seqlens_k=None,
                max_seqlen_q=0, max_seqlen_k=0):
        softmax_scale = _sink_args(sinks, Q.shape[-3 if cu_seqlens_q is None else 1], Q.device, softmax_scale, True)
        args = (int(window_left), int(window_right), softmax_scale, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q),
                int(max_seqlen_k))
        return _twin_forward(ctx, flash_attention_sink_forward, Q, K, V, args, extra=(sinks,))

    @staticmethod
    def backward(ctx, dO):
        need = ctx.needs_input_grad[3]     # without it the sink-gradient kernel is not launched and dsinks is None
        return _twin_backward(ctx, lambda *a: flash_attention_sink_backward(*a, need_dsinks=need), dO)


def flash_attention_kvcache_sink(q, k_cache, v_cache, cache_seqlens, sinks, k_new=None, v_new=None, is_causal=False,
                                 window_size=(-1, -1), softmax_scale=None, return_lse=False):
    """Decoding attention over a padded KV cache with attention sinks: flash_attention_kvcache with exp(sinks[h]) added to
    the softmax denominator of every row of query head h (flash_attention_sink's formulas; LSE includes the sink).
    sinks: float32 device tensor, contiguous, (H,), natural-log units, never read on the host: a step stays
    graph-capturable and the sinks may change between replays.  scale = softmax_scale (> 0), default 1/sqrt(D).

    Everything else is flash_attention_kvcache: q [B, H, S_q, D], the caches [B, H_kv, S_cache, D], cache_seqlens int32
    [B]; k_new / v_new are appended first; window_size and is_causal as there (bottom-right aligned).  A row with no
    visible key (an empty sequence included) gets O = 0 and LSE = sinks[h].  Inference only (an input that requires grad
    is refused, sinks included); deterministic at any split count: the sink enters each row exactly once.
    Returns O, and with return_lse=True also LSE [B, H, S_q] (fp32)."""
    softmax_scale = _sink_args(sinks, q.shape[1], q.device, softmax_scale, False)
    return _decode("flash_attention_kvcache_sink", _ext.kvcache_sink_forward, q, k_cache, v_cache, cache_seqlens,
                   (sinks,), k_new, v_new, is_causal, window_size, softmax_scale, return_lse)


def flash_attention_kvcache_fp8_sink(q, k_cache, v_cache, cache_seqlens, sinks, k_descale=None, v_descale=None, k_new=None,
                                     v_new=None, is_causal=False, window_size=(-1, -1), softmax_scale=None,
                                     return_lse=False):
    """flash_attention_kvcache_fp8 with attention sinks (flash_attention_kvcache_sink over torch.float8_e4m3fn caches).
    k_descale scales the scores only, never the sink; v_descale the output only.  sinks as in
    flash_attention_kvcache_sink; every other argument as in flash_attention_kvcache_fp8.  Inference only."""
    softmax_scale = _sink_args(sinks, q.shape[1], q.device, softmax_scale, False)
    return _decode("flash_attention_kvcache_fp8_sink", _ext.kvcache_fp8_sink_forward, q, k_cache, v_cache, cache_seqlens,
                   (sinks, k_descale, v_descale), k_new, v_new, is_causal, window_size, softmax_scale, return_lse, fp8=True)


def sdpa_reference(Q, K, V, is_causal):
    """torch SDPA on the device, fp16/bf16 (the reference pins the FLASH backend, M:178;
    here whatever backend this PyTorch-ROCm build selects)."""
    return F.scaled_dot_product_attention(Q, K, V, attn_mask=None, dropout_p=0.0, is_causal=is_causal)


def compare_with_sdpa(Q, K, V, is_causal, verbose=True):
    """Fwd+bwd of SDPA and of flash_attention on the same inputs and dO; verifies O, dQ, dK, dV
    in that order (M:172-212).  Returns the four metric dicts."""
    Q_ref = Q.detach().clone().requires_grad_(True)
    K_ref = K.detach().clone().requires_grad_(True)
    V_ref = V.detach().clone().requires_grad_(True)
    O_ref = sdpa_reference(Q_ref, K_ref, V_ref, is_causal)
    dO = torch.randn_like(O_ref)
    O_ref.backward(dO)
    dQ_ref, dK_ref, dV_ref = Q_ref.grad, K_ref.grad, V_ref.grad

    Q_ = Q.detach().clone().requires_grad_(True)
    K_ = K.detach().clone().requires_grad_(True)
    V_ = V.detach().clone().requires_grad_(True)
    O = flash_attention(Q_, K_, V_, is_causal=is_causal)
    O.backward(dO)
    dQ, dK, dV = Q_.grad, K_.grad, V_.grad

    from _verify_func import verify_results
    out = {}
    for name, ref, got in (("O", O_ref, O), ("dQ", dQ_ref, dQ), ("dK", dK_ref, dK), ("dV", dV_ref, dV)):
        if verbose:
            print("=" * 30 + " " + name + " test " + "=" * 30)
        out[name] = verify_results(ref, got, name=name, verbose=verbose)
    return out


if __name__ == "__main__":
    DEVICE = torch.device(torch.cuda.current_device())
    B, H, S_q, S_k, D = 4, 8, 256, 256, 64
    Q = torch.randn((B, H, S_q, D), dtype=torch.float16, device=DEVICE)
    K = torch.randn((B, H, S_k, D), dtype=torch.float16, device=DEVICE)
    V = torch.randn((B, H, S_k, D), dtype=torch.float16, device=DEVICE)
    compare_with_sdpa(Q, K, V, is_causal=True)
