"""CPU tests of the top-k selection (include_mla_select/mi355fa_mla_select.h, mla_indexer.mla_indexer_select): the refusals of the
wrapper and of the C call with their messages, the header against the signature table, and the two kernels' resources."""
import ctypes
import os
import sys

import pytest
import torch

from conftest import ROOT
import variantcheck as vck
from test_host_mla import OnDevice

sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

NULL, SHAPE, ALIGN, STRIDE = -1, -2, -5, -6
FN = "fa_mla_indexer_select"
ARGS = ("logits", "lengths", "out", "B", "Sq", "W", "topk", "ls", "os")


def test_the_wrapper_refuses_malformed_calls_with_their_messages():
    import mla_indexer as M
    x = torch.zeros(2, 1, 40)

    def refused(msg, *a, **kw):
        with pytest.raises(AssertionError) as e:
            M.mla_indexer_select(*a, **kw)
        assert str(e.value) == msg, str(e.value)
    refused("logits must be float32 [B, S_q, W]", x.half(), 4)
    refused("logits must be float32 [B, S_q, W]", x[0], 4)
    refused("topk must be an int in [1, 65536] (got 0)", x, 0)
    refused("topk must be an int in [1, 65536] (got 65537)", x, 65537)
    refused("lengths must be None or an int32 tensor [B]", x, 4, lengths=torch.zeros(3, dtype=torch.int32))
    refused("lengths must be a device tensor: the kernel reads it, the host never does", x, 4, lengths=torch.zeros(2, dtype=torch.int32))
    refused("out must be None or an int32 tensor [B, S_q, topk]", x, 4, out=torch.zeros(2, 1, 5, dtype=torch.int32))
    refused("logits must have unit stride along W (got 2)", x[..., ::2], 4)
    refused("mla_indexer_select has no backward: logits must not require grad", x.clone().requires_grad_(True), 4)
    refused("logits, lengths and out must be device tensors", x, 4, lengths=torch.zeros(2, dtype=torch.int32).as_subclass(OnDevice))


def test_c_refusals_and_the_signature_table():
    import _mi355fa as fa
    _, _, names = vck.header_functions(os.path.join(ROOT, "include_mla_select", "mi355fa_mla_select.h"))
    assert names == [FN] and set(fa.MLA_SELECT_SIGNATURES) == {FN} and FN in fa.ALL_SIGNATURES and fa.lib.fa_abi_version() == 7
    buf, p = vck.aligned_ptr()
    st = lambda *v: (ctypes.c_longlong * len(v))(*v)
    for kw, code, text in [(dict(logits=None), NULL, "logits is NULL (argument 1)"),
                           (dict(out=None), NULL, "indices is NULL (argument 3)"),
                           (dict(B=0), SHAPE, "B must be in [1, 65535] (got 0)"),
                           (dict(W=0), SHAPE, "W must be in [1, 2^30] (got 0)"),
                           (dict(topk=65537), SHAPE, "topk must be in [1, 65536] (got 65537)"),
                           (dict(ls=st(-256, 256)), STRIDE, "logits_strides must be non-negative and at most 2^40 elements (got -256)"),
                           (dict(Sq=2, os=st(64, 31)), STRIDE,
                            "the rows of indices must not overlap: a row stride of at least topk, a non-zero batch stride (row stride 31)"),
                           (dict(lengths=p + 2), ALIGN, "logits, lengths and indices must be 4-byte aligned (one ends in 2)")]:
        a = dict(logits=p, lengths=None, out=p, B=2, Sq=1, W=256, topk=32, ls=None, os=None)
        a.update(kw)
        assert fa.lib.fa_mla_indexer_select(*[a[k] for k in ARGS], None) == code, (kw, fa.lib.fa_last_error())
        assert fa.lib.fa_last_error().decode() == FN + ": " + text


def test_two_kernels_without_scratch_inside_the_lds():
    ks = [k for k in codeobj.kernels() if "IdxSelect" in k["name"]]
    assert len(ks) == 2 and all("fa_decode_paged_kernel" in k["name"] for k in ks)
    for k in ks:
        assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 160 * 1024, k   # (spill: vector registers to scratch)
