"""Sparse (top-k indexed) MLA prefill over one contiguous latent array
(include_mla_sparse_prefill/mi355fa_mla_sparse_prefill.h): the prefill step of DeepSeek-V3.2, where the indexer
(mla_indexer.mla_indexer_logits_fp8_prefill, then mla_indexer.mla_indexer_select) picks per packed query token rows of the
step's packed key array -- the same for all heads of that token -- and attention runs over those alone.  The rows are read in
place by a gathering kernel: no row is copied.  A module beside the other MLA modules; the native side is
csrc/torch_binding_mla_sparse_prefill.cpp -> _mi355fa_mla_sparse_prefill_torch.so over libmi355fa.so.  There is NO fallback: a
missing library or binding is an ImportError."""
import torch

from mla_kvcache import _check_call
import _mi355fa_mla_sparse_prefill_torch as _ext   # raises if the binding was not built (make -C csrc)

__all__ = ["flash_attention_mla_sparse_prefill"]


def flash_attention_mla_sparse_prefill(q, kv, indices, softmax_scale=None, return_lse=False, out=None):
    """Attention of packed absorbed MLA queries over the rows of kv their index lists name.

    q [M, H, 576], fp16 or bf16, packed over all sequences of the step: dims [0, 512) the absorbed no-RoPE part, [512, 576) the
    RoPE part.  Read in place through its row and head strides when the last dim is contiguous and both strides are non-negative
    multiples of 8 elements (copied otherwise).  Any H >= 1; the kernel works on blocks of 32 heads.

    kv [N, 576] in q's dtype: the latent rows (512) and RoPE part (64) of all keys of the step in one array -- the array the
    `k` positions of mla_indexer_logits_fp8_prefill refer to.  Last dim contiguous, a row stride that is a multiple of 8 elements
    and at least 576; read in place with 64-bit addresses and never copied, so it may exceed 4 GiB.

    indices: int32 device tensor [M, topk], topk >= 1, unit stride along topk, any non-negative row stride -- exactly
    mla_indexer_select(logits.view(M, 1, -1), topk, lengths=ke)[:, 0].  The host never reads it, so a captured step replays while
    it changes in place.  Entry j of row m is a row of kv, visible iff 0 <= idx < N; every other value is skipped and causes no
    access at all: -1 padding, anything negative, anything at or past N.  An entry that appears twice counts twice.  There is no
    causal flag: the indexer's [ks, ke) already decided what a row may see.

    Returns O [M, H, 512] in q's dtype (`out`, written through its row and head strides, if given) and, with return_lse=True,
    LSE [M, H] fp32 in natural-log units; a row with no visible entry gets O = 0 and LSE = -inf.  softmax_scale defaults to
    576 ** -0.5, as for mla_kvcache.flash_attention_mla_kvcache, and must be finite and > 0.  M == 0 launches nothing.  The
    summation order is list order, so the result is the same bits on every launch.  Inference only: an input that requires grad
    is refused."""
    scale = _check_call("flash_attention_mla_sparse_prefill", (("q", q), ("kv", kv), ("indices", indices)), None,
                        (("indices", indices),), (("indices", indices, "kernel"),), softmax_scale, q=q, kv=kv, kv_new=None, out=out)
    O, LSE = _ext.mla_sparse_prefill_forward(q, kv, indices, scale, out)
    return (O, LSE) if return_lse else O
