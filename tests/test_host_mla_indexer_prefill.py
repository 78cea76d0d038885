"""CPU tests of mla_indexer.mla_indexer_logits_fp8_prefill (include_mla_indexer_prefill/mi355fa_mla_indexer_prefill.h): the
refusals of the wrapper and of the C call with their messages, and the header against the signature table."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT
import variantcheck as vck
from test_host_mla import OnDevice

NULL, SHAPE, ALIGN, STRIDE = -1, -2, -5, -6
FN = "fa_mla_indexer_logits_fp8_prefill"
ARGS = ("q", "w", "k", "s", "ks", "ke", "out", "M", "Hi", "N", "W", "qs", "ws", "krs", "srs", "ors")


def test_the_wrapper_refuses_malformed_calls_with_their_messages():
    import mla_indexer as M
    assert FN[3:] in M.__all__
    q, w = torch.zeros(5, 64, 128, dtype=torch.uint8), torch.zeros(5, 64)
    k, s = torch.zeros(40, 128).to(torch.float8_e4m3fn), torch.zeros(40)
    lo = hi = torch.zeros(5, dtype=torch.int32).as_subclass(OnDevice)

    def refused(msg, *a, **kw):
        with pytest.raises(AssertionError) as e:
            M.mla_indexer_logits_fp8_prefill(*a, **kw)
        assert str(e.value) == msg, str(e.value)
    refused("q must be torch.float8_e4m3fn or its uint8 view (got torch.bfloat16)", q.to(torch.bfloat16), w, k, s, lo, hi)
    refused("weights must be float32 (got torch.float16)", q, w.half(), k, s, lo, hi)
    refused("q must be [M, H_i, 128] (got (5, 64, 64))", q[..., :64], w, k, s, lo, hi)
    refused("H_i (q.shape[1]) must be 16, 32, 48 or 64 (got 24)", q[:, :24], w[:, :24], k, s, lo, hi)
    refused("k is read in place: unit stride along the 128 bytes, a row stride that is a multiple of 16 and at least 128 (got (264, 1))",
            q, w, torch.zeros(40, 264, dtype=torch.uint8)[:, :128], s, lo, hi)
    refused("ke must be a device tensor: the kernel reads it, the host never does", q, w, k, s, lo, torch.zeros(5, dtype=torch.int32))
    refused("out must be None or a float32 tensor [M, W] with W >= N", q, w, k, s, lo, hi, out=torch.zeros(5, 39))
    refused("mla_indexer_logits_fp8_prefill has no backward: weights must not require grad", q, w.clone().requires_grad_(True), k, s, lo, hi)
    refused("q, weights, k, k_scale, ks, ke and out must be device tensors", q, w, k, s, lo, hi)


def test_c_refusals_and_the_signature_table():
    import _mi355fa as fa
    _, _, names = vck.header_functions(os.path.join(ROOT, "include_mla_indexer_prefill", "mi355fa_mla_indexer_prefill.h"))
    assert names == [FN] and set(fa.MLA_INDEXER_PREFILL_SIGNATURES) == {FN} and FN in fa.ALL_SIGNATURES and fa.lib.fa_abi_version() == 7
    buf, p = vck.aligned_ptr()
    st = lambda *v: (ctypes.c_longlong * len(v))(*v)
    for kw, code, text in [(dict(q=None), NULL, "q is NULL (argument 1)"),
                           (dict(Hi=24), SHAPE, "H_i must be 16, 32, 48 or 64 (got 24)"),
                           (dict(N=257), SHAPE, "N must be in [0, W] (got 257)"),
                           (dict(qs=st(8192, 136)), STRIDE, "q_strides must be non-negative multiples of 16 bytes (got 136)"),
                           (dict(krs=112), STRIDE, "k_row_stride must be a multiple of 16 in [128, 2^24] bytes (got 112)"),
                           (dict(ors=255), STRIDE, "the rows of logits must not overlap: logits_row_stride must be at least W (got 255)"),
                           (dict(k=p + 8), ALIGN, "k must be 16-byte aligned (ends in 8)"),
                           (dict(ks=p + 2), ALIGN, "weights, k_scale, ks, ke and logits must be 4-byte aligned (one ends in 2)")]:
        a = dict(q=p, w=p, k=p, s=p, ks=p, ke=p, out=p, M=8, Hi=64, N=256, W=256, qs=None, ws=None, krs=128, srs=1, ors=256)
        a.update(kw)
        assert fa.lib.fa_mla_indexer_logits_fp8_prefill(*[a[k] for k in ARGS], None) == code, (kw, fa.lib.fa_last_error())
        assert fa.lib.fa_last_error().decode() == FN + ": " + text
