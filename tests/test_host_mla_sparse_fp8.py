"""CPU tests of sparse (top-k indexed) MLA decoding over the FP8 latent cache
(include_mla_sparse_fp8/mi355fa_kvcache_mla_sparse_fp8.h, mla_sparse_fp8_kvcache.py): the refusals of the wrapper and of the C
call, the workspace function against the split rule, and the new kernels' resources from the code objects."""
import ctypes
import os
import re
import sys

import pytest
import torch

from conftest import ROOT
import variantcheck as vck
from test_host_mla import OnDevice, splits_formula

NULL, SHAPE, STRIDE, WORKSPACE = -1, -2, -6, -9
FN = "fa_fwd_kvcache_mla_sparse_fp8"
ARGS = ("q", "kv", "new", "idx", "sl", "bt", "o", "lse", "ws", "wsb", "B", "H", "Sq", "topk", "pages", "page", "mp", "bts", "Snew",
        "dtype", "scale", "causal", "qs", "ks", "os", "xs")


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def _call(fa, p, **kw):
    a = dict(q=p, kv=p, new=None, idx=p, sl=p, bt=p, o=p, lse=p, ws=p, wsb=1 << 30, B=2, H=16, Sq=1, topk=64, pages=8, page=64, mp=4,
             bts=4, Snew=0, dtype=fa.BF16, scale=576 ** -0.5, causal=1, qs=None, ks=None, os=None, xs=None)
    a.update(kw)
    return fa.lib.fa_fwd_kvcache_mla_sparse_fp8(*[a[k] for k in ARGS], None)


def test_the_wrapper_refuses_malformed_calls_with_their_messages():
    import mla_sparse_fp8_kvcache as M
    f = M.flash_attention_mla_kvcache_sparse_fp8
    q = torch.randn(2, 4, 2, 576).to(torch.bfloat16)
    kv = torch.zeros(6, 32, 656, dtype=torch.uint8)
    dev = lambda *s: torch.zeros(*s, dtype=torch.int32).as_subclass(OnDevice)
    idx, sl, bt = dev(2, 2, 8), dev(2), dev(2, 3)

    def refused(msg, *a):
        with pytest.raises(AssertionError) as e:
            f(*a)
        assert str(e.value) == msg, str(e.value)
    refused("kv_cache must be torch.uint8 [num_pages, page_size, 656]: rows of 512 e4m3 bytes, 4 fp32 scales and 64 RoPE values "
            "in q's dtype (got torch.bfloat16)", q, torch.zeros(6, 32, 576, dtype=torch.bfloat16), idx, sl, bt)
    refused("kv_cache's last dim must be 656 bytes (got 576)", q, kv[..., :576], idx, sl, bt)
    refused("indices must be int32 (got torch.int64)", q, kv, idx.long(), sl, bt)
    refused("indices must be a device tensor: the kernel reads it, the host never does", q, kv, torch.zeros(2, 2, 8, dtype=torch.int32), sl, bt)
    refused("indices must be an int32 tensor [B, S_q, topk] with 1 <= topk <= 2^24", q, kv, idx[..., :0], sl, bt)
    refused("flash_attention_mla_kvcache_sparse_fp8 has no backward: q must not require grad", q.float().requires_grad_(True), kv, idx, sl, bt)
    refused("q, kv_cache, indices, cache_seqlens and block_table must be device tensors", q, kv, idx, sl, bt)


def test_c_refusals_and_the_workspace_formula():
    """the rule: mla_splits with topk in the place of S_cache over B * S_q * ceil(H / 32) workgroups per split"""
    import _mi355fa as fa
    buf, p = vck.aligned_ptr()
    st = lambda *v: (ctypes.c_longlong * len(v))(*v)
    for kw, code, text in [(dict(idx=None), NULL, "indices is NULL (argument 4)"),
                           (dict(topk=0), SHAPE, "topk must be in [1, 2^24] (got 0)"),
                           (dict(ks=st(41984, 664)), STRIDE, "the row stride of kv_pool must be a multiple of 16 bytes and at least 656 (got 664)"),
                           (dict(xs=st(64, -64)), STRIDE, "indices_strides must be non-negative and at most 2^40 elements (got -64)")]:
        assert _call(fa, p, **kw) == code, (kw, fa.lib.fa_last_error())
        assert fa.lib.fa_last_error().decode() == FN + ": " + text
    ws = fa.lib.fa_fwd_kvcache_mla_sparse_fp8_workspace_bytes
    for B, H, Sq, topk in [(1, 1, 1, 1), (8, 128, 1, 2048), (8, 16, 1, 2048), (3, 40, 3, 160)]:
        n = splits_formula(B * Sq, H, 1, topk)
        assert ws(B, H, Sq, topk, 4, 64, Sq) == (n * B * H * Sq * 514 * 4 if n > 1 else 0), (B, H, Sq, topk, n)
        assert ws(B, H, Sq, topk, 4, 64, 0) == fa.lib.fa_fwd_kvcache_mla_sparse_workspace_bytes(B, H, Sq, topk, 4, 64, 0)
        vck.splits(7)
        assert ws(B, H, Sq, topk, 4, 64, 0) == 7 * B * H * Sq * 514 * 4
        vck.splits(0)
    vck.splits(3)
    need = ws(2, 16, 1, 64, 4, 64, 0)
    assert need == 3 * 2 * 16 * 514 * 4 and _call(fa, p, wsb=need - 1) == WORKSPACE
    assert fa.lib.fa_last_error().decode() == FN + ": workspace smaller than %s_workspace_bytes() (%d bytes)" % (FN, need)


def test_two_new_kernels_are_in_the_library_inside_the_decode_budget():
    """the <GatherF8, T> overload of fa_decode_paged_kernel over GatherF8Params, fp16 and bf16, and no other kernel with the tag:
    workgroup 256, VGPR + AGPR <= 256, no scratch, no spills, LDS within 80 KiB (the carve is dynamic: the source asserts it)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj
    found = []
    for k in codeobj.kernels():
        if "GatherF8" not in k["name"]:
            continue
        m = re.match(r"_ZN2fa22fa_decode_paged_kernelINS_8GatherF8ENS_4(BF16|FP16)EEEvNS_14GatherF8ParamsE$", k["name"])
        assert m, "a kernel with the sparse FP8 tag outside the expected set: " + k["name"]
        found.append(m.group(1))
        assert k["wg"] == 256 and k["vgpr"] + k["agpr"] <= 256, (k["name"], k["vgpr"], k["agpr"])
        assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 81920, k["name"]
    assert sorted(found) == ["BF16", "FP16"], found
    src = open(os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd", "csrc", "fa_decode_mla_sparse_fp8.hip")).read()
    assert 'static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU")' in src
