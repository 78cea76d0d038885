"""CPU tests of the indexer logits (include_mla_indexer/mi355fa_mla_indexer.h, mla_indexer.py): the refusals of the wrapper and
of the C call with their messages, and the header against the signature table."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT
import variantcheck as vck
from test_host_mla import OnDevice

NULL, SHAPE, ALIGN, STRIDE, PAGED = -1, -2, -5, -6, -12
FN = "fa_mla_indexer_logits_fp8"
ARGS = ("q", "w", "k", "ks", "new", "sl", "bt", "out", "B", "Sq", "Hi", "W", "pages", "page", "mp", "bts", "Snew", "dtype", "causal",
        "qs", "ws", "kst", "sst", "os")


def _call(fa, p, **kw):
    a = dict(q=p, w=p, k=p, ks=p, new=None, sl=p, bt=p, out=p, B=2, Sq=1, Hi=64, W=256, pages=8, page=64, mp=4, bts=4, Snew=0,
             dtype=fa.BF16, causal=1, qs=None, ws=None, kst=None, sst=None, os=None)
    a.update(kw)
    return fa.lib.fa_mla_indexer_logits_fp8(*[a[k] for k in ARGS], None)


def test_the_wrapper_refuses_malformed_calls_with_their_messages():
    import mla_indexer as M
    f = M.mla_indexer_logits_fp8
    q, w = torch.zeros(2, 1, 64, 128, dtype=torch.uint8), torch.zeros(2, 1, 64)
    k, ks = torch.zeros(6, 32, 128).to(torch.float8_e4m3fn), torch.zeros(6, 32)
    dev = lambda *s: torch.zeros(*s, dtype=torch.int32).as_subclass(OnDevice)
    sl, bt = dev(2), dev(2, 3)

    def refused(msg, *a, **kw):
        with pytest.raises(AssertionError) as e:
            f(*a, **kw)
        assert str(e.value) == msg, str(e.value)
    refused("q must be torch.float8_e4m3fn or its uint8 view (got torch.bfloat16)", q.to(torch.bfloat16), w, k, ks, sl, bt)
    refused("k_cache must be torch.float8_e4m3fn or its uint8 view (got torch.float32)", q, w, k.float(), ks, sl, bt)
    refused("weights must be float32 (got torch.float16)", q, w.half(), k, ks, sl, bt)
    refused("H_i (q.shape[2]) must be a multiple of 16 in [16, 64] (got 24)", q[:, :, :24], w, k, ks, sl, bt)
    refused("q must be [B, S_q, H_i, 128] (got (2, 1, 64, 64))", q[..., :64], w, k, ks, sl, bt)
    refused("k_cache must be [num_pages, page_size, 128] (got (6, 32, 96))", q, w, k[..., :96], ks, sl, bt)
    refused("the page size (k_cache.shape[1] = 48) must be a positive multiple of 32", q, w, torch.zeros(6, 48, 128, dtype=torch.uint8), ks, sl, bt)
    refused("cache_seqlens must be a device tensor: the kernels read it, the host never does", q, w, k, ks, torch.zeros(2, dtype=torch.int32), bt)
    refused("block_table must be a device tensor: the kernels read it, the host never does", q, w, k, ks, sl, torch.zeros(2, 3, dtype=torch.int32))
    refused("mla_indexer_logits_fp8 has no backward: weights must not require grad", q, w.clone().requires_grad_(True), k, ks, sl, bt)
    refused("q, weights, k_cache, k_scale, cache_seqlens and block_table must be device tensors", q, w, k, ks, sl, bt)
    assert M.mla_indexer_topk(torch.tensor([[[1.0, float("-inf"), 3.0]]]), 4).tolist() == [[[2, 0, -1, -1]]]


def test_c_refusals_and_the_signature_table():
    import _mi355fa as fa
    _, _, names = vck.header_functions(os.path.join(ROOT, "include_mla_indexer", "mi355fa_mla_indexer.h"))
    assert names == [FN] and set(fa.MLA_INDEXER_SIGNATURES) == {FN} and FN in fa.ALL_SIGNATURES and fa.lib.fa_abi_version() == 7
    buf, p = vck.aligned_ptr()
    st = lambda *v: (ctypes.c_longlong * len(v))(*v)
    for kw, code, text in [(dict(q=None), NULL, "q is NULL (argument 1)"),
                           (dict(ks=None), NULL, "k_scale is NULL (argument 4)"),
                           (dict(Snew=1), NULL, "S_new != 0 needs k_new (S_new 1)"),
                           (dict(new=p, Snew=2), SHAPE, "k_new holds one row per query row: S_new must be S_q (S_new 2)"),
                           (dict(Hi=24), SHAPE, "H_i must be 16, 32, 48 or 64 (got 24)"),
                           (dict(page=48), PAGED, "page_size must be a positive multiple of 32 (got 48)"),
                           (dict(qs=st(8192, 8192, 136)), STRIDE, "q_strides must be non-negative multiples of 16 bytes (got 136)"),
                           (dict(qs=st(8192, 8192, 64)), STRIDE, "the head stride of q must be at least 128 bytes (got 64)"),
                           (dict(kst=st(8192, 112)), STRIDE, "the row stride of k_cache must be in [128, 2^24] bytes (got 112)"),
                           (dict(Sq=2, os=st(512, 128)), STRIDE,
                            "the rows of logits must not overlap: a row stride of at least W, a non-zero batch stride (row stride 128)"),
                           (dict(k=p + 8), ALIGN, "k_cache must be 16-byte aligned (ends in 8)")]:
        assert _call(fa, p, **kw) == code, (kw, fa.lib.fa_last_error())
        assert fa.lib.fa_last_error().decode() == FN + ": " + text
