"""CPU tests of mla_sparse_prefill.flash_attention_mla_sparse_prefill (include_mla_sparse_prefill/mi355fa_mla_sparse_prefill.h):
the refusals of the wrapper and of the C call with their messages, the header against the signature table, and the new kernels'
resources from the code objects."""
import ctypes
import os
import re
import sys

import pytest
import torch

from conftest import ROOT
import variantcheck as vck
from test_host_mla import OnDevice

NULL, SHAPE, DTYPE, ALIGN, STRIDE = -1, -2, -4, -5, -6
FN = "fa_fwd_mla_sparse_prefill"
ARGS = ("q", "kv", "idx", "o", "lse", "M", "H", "N", "topk", "dtype", "scale", "qs", "krs", "os", "xrs")
ST = lambda *v: (ctypes.c_longlong * len(v))(*v)


def test_the_wrapper_refuses_malformed_calls_with_their_messages():
    import mla_sparse_prefill as P
    assert P.__all__ == ["flash_attention_mla_sparse_prefill"]
    q, kv = torch.zeros(5, 16, 576, dtype=torch.bfloat16), torch.zeros(40, 576, dtype=torch.bfloat16)
    idx = torch.zeros(5, 8, dtype=torch.int32).as_subclass(OnDevice)

    def refused(msg, *a, **kw):
        with pytest.raises(AssertionError) as e:
            P.flash_attention_mla_sparse_prefill(*a, **kw)
        assert str(e.value) == msg, str(e.value)
    refused("kv must be a tensor", q, None, idx)
    refused("indices must be int32 (got torch.int64)", q, kv, idx.long())
    refused("indices must be a device tensor: the kernel reads it, the host never does", q, kv, torch.zeros(5, 8, dtype=torch.int32))
    refused("softmax_scale must be finite and > 0", q, kv, idx, softmax_scale=float("inf"))
    refused("flash_attention_mla_sparse_prefill has no backward: q must not require grad", q.clone().requires_grad_(True), kv, idx)
    refused("q must be [M, H, 576]: 512 latent dims, then 64 RoPE dims (got 3 dims)", q[..., :512], kv, idx)
    refused("q's dtype must be float16 or bfloat16", q.float(), kv.float(), idx)
    refused("kv must have q's dtype", q, kv.half(), idx)
    refused("indices must be an int32 tensor [M, topk] with 1 <= topk <= 2^24", q, kv, idx[:4])
    refused("indices must have unit stride along topk and a non-negative row stride", q, kv, idx[:, ::2])
    refused("kv must be addressable in place: unit stride along the 576 dims and 16-byte aligned rows (a row stride that is a "
            "multiple of 8 elements and at least 576, got 580)", q, torch.zeros(40, 580, dtype=torch.bfloat16)[:, :576], idx)
    refused("out must be [M, H, 512] in q's dtype", q, kv, idx, out=torch.zeros(5, 16, 576, dtype=torch.bfloat16))
    refused("q, kv, indices and out must be device tensors", q, kv, idx)


REFUSALS = [                                                      # ("p+n": the aligned buffer's address plus n)
    (dict(q=None), NULL, "q is NULL (argument 1)"),
    (dict(kv=None), NULL, "kv is NULL (argument 2)"),
    (dict(idx=None), NULL, "indices is NULL (argument 3)"),
    (dict(dtype=2), DTYPE, "dtype must be 0 (fp16) or 1 (bf16) (got 2)"),
    (dict(scale=0.0), SHAPE, "scale must be finite and > 0 (its bits are 0)"),
    (dict(M=0), SHAPE, "M must be in [1, 2^22] (got 0)"),
    (dict(H=1025), SHAPE, "H must be in [1, 1024] (got 1025)"),
    (dict(N=-1), SHAPE, "N must be >= 0 (got -1)"),
    (dict(topk=0), SHAPE, "topk must be in [1, 2^24] (got 0)"),
    (dict(topk=(1 << 24) + 1), SHAPE, "topk must be in [1, 2^24] (got 16777217)"),
    (dict(qs=ST(9216, 580)), STRIDE, "q_strides must be non-negative multiples of 8 elements (got 580)"),
    (dict(os=ST(8192, 504)), STRIDE, "the head stride of o must be at least 512 elements (got 504)"),
    (dict(os=ST(0, 512)), STRIDE, "the row stride of o must be at least 512 elements (got 0)"),
    (dict(krs=580), STRIDE, "kv_row_stride must be a multiple of 8 in [576, 2^24] elements (got 580)"),
    (dict(xrs=-64), STRIDE, "indices_row_stride must be non-negative and at most 2^40 elements (got -64)"),
    (dict(kv="p+4"), ALIGN, "kv must be 16-byte aligned (ends in 4)"),
    (dict(lse="p+2"), ALIGN, "lse must be 4-byte aligned (ends in 2)"),
    (dict(idx="p+2"), ALIGN, "indices must be 4-byte aligned (ends in 2)"),
]


@pytest.mark.parametrize("kw,code,text", REFUSALS, ids=[t.split(" (")[0][:40] for _, _, t in REFUSALS])
def test_c_refusals_name_the_argument_and_carry_the_value(kw, code, text):
    import _mi355fa as fa
    buf, p = vck.aligned_ptr()
    a = dict(q=p, kv=p, idx=p, o=p, lse=p, M=8, H=16, N=256, topk=64, dtype=fa.BF16, scale=576 ** -0.5, qs=None, krs=576, os=None, xrs=64)
    a.update({k: p + int(v[2:]) if isinstance(v, str) else v for k, v in kw.items()})
    assert fa.lib.fa_fwd_mla_sparse_prefill(*[a[k] for k in ARGS], None) == code, fa.lib.fa_last_error()
    assert fa.lib.fa_last_error().decode() == FN + ": " + text


def test_the_header_lists_the_function_of_the_signature_table():
    import _mi355fa as fa
    hdr = os.path.join(ROOT, "include_mla_sparse_prefill")
    assert os.listdir(hdr) == ["mi355fa_mla_sparse_prefill.h"]
    _, _, names = vck.header_functions(os.path.join(hdr, "mi355fa_mla_sparse_prefill.h"))
    assert names == [FN] and set(fa.MLA_SPARSE_PREFILL_SIGNATURES) == {FN} and FN in fa.ALL_SIGNATURES and fa.lib.fa_abi_version() == 7


def test_two_new_kernels_are_in_the_library_inside_the_decode_budget():
    """the <RowList, T> overload of fa_decode_paged_kernel over RowListParams, fp16 and bf16, and no other kernel with the tag:
    workgroup 256, VGPR + AGPR <= 256, no scratch, no spills, LDS within 80 KiB (the carve is dynamic: the source asserts it)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj
    found = []
    for k in codeobj.kernels():
        if "RowList" not in k["name"]:
            continue
        m = re.match(r"_ZN2fa22fa_decode_paged_kernelINS_7RowListENS_4(BF16|FP16)EEEvNS_13RowListParamsE$", k["name"])
        assert m, "a kernel with the sparse prefill tag outside the expected set: " + k["name"]
        found.append(m.group(1))
        assert k["wg"] == 256 and k["vgpr"] + k["agpr"] <= 256, (k["name"], k["vgpr"], k["agpr"])
        assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 81920, k["name"]
    assert sorted(found) == ["BF16", "FP16"], found
    src = open(os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd", "csrc", "fa_mla_sparse_prefill.hip")).read()
    assert 'static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU")' in src
