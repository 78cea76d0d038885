"""CPU tests of MLA decoding over a paged latent cache with packed variable-length queries
(include_mla_ragged/mi355fa_ragged_mla.h, mla_ragged_kvcache.py): the Python and binding signatures, every refusal with its exact
message and the order of the checks (pairs of simultaneous faults), the workspace function against its formula, the ABI version
and the header, the new kernels' resources from the code objects, the packing helper of the GPU tests against mlacheck's truth,
and the reference-only condition of the GPU scale test."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

from conftest import ROOT
import fa_oracle as fo
import mlacheck as mc
import mlaraggedcheck as mr
import variantcheck as vck
from test_host_mla import OnDevice, splits_formula

BF16, F16 = torch.bfloat16, torch.float16
NULL, SHAPE, DTYPE, ALIGN, STRIDE, WORKSPACE, PAGED = -1, -2, -4, -5, -6, -9, -12
FN = "fa_fwd_kvcache_mla_ragged"


def _lib():
    import _mi355fa as fa
    return fa


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


# ---------------------------------------------------------------- surface
def test_python_and_binding_signatures():
    import mla_kvcache
    import mla_ragged_kvcache as M
    import _mi355fa_mla_ragged_torch as ext
    assert M.__all__ == ["flash_attention_mla_kvcache_ragged"]
    assert mla_kvcache.__all__ == ["flash_attention_mla_kvcache", "MLA_D", "MLA_DV"]
    sig = inspect.signature(M.flash_attention_mla_kvcache_ragged)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [
        ("q", inspect.Parameter.empty), ("kv_cache", inspect.Parameter.empty), ("cu_seqlens_q", inspect.Parameter.empty),
        ("cache_seqlens", inspect.Parameter.empty), ("block_table", inspect.Parameter.empty), ("kv_new", None), ("is_causal", False),
        ("softmax_scale", None), ("return_lse", False), ("out", None)]
    doc = M.flash_attention_mla_kvcache_ragged.__doc__
    for words in ("[total_q, H, 576]", "[total_q, H, 512]", "[H, total_q]", "576 ** -0.5", "(128 + 64) ** -0.5", "never read",
                  "never written", "O = 0 and LSE = -inf", "Inference only", "no fallback", "int32 device tensor [B + 1]"):
        assert words in doc, words
    assert [n for n in dir(ext) if not n.startswith("_")] == ["kvcache_mla_ragged_forward"]
    args = re.search(r"kvcache_mla_ragged_forward\((.*?)\) ->", ext.kvcache_mla_ragged_forward.__doc__, re.S).group(1)
    assert re.findall(r"(\w+): ", args) == ["q", "kv_cache", "cu_seqlens_q", "cache_seqlens", "block_table", "kv_new", "is_causal",
                                            "softmax_scale", "out"]


def test_abi_header_and_ctypes_signatures():
    fa = _lib()
    assert fa.lib.fa_abi_version() == 7 and fa.ABI_VERSION == 7
    assert os.listdir(os.path.join(ROOT, "include_mla_ragged")) == ["mi355fa_ragged_mla.h"]
    txt, body, names = vck.header_functions(os.path.join(ROOT, "include_mla_ragged", "mi355fa_ragged_mla.h"))
    assert names == [FN, FN + "_workspace_bytes"]
    assert '#include "../include_mla/mi355fa_kvcache_mla.h"' in body and "#define" not in body.replace("#define MI355FA_RAGGED_MLA_H_", "")
    assert set(fa.KVCACHE_MLA_RAGGED_SIGNATURES) == set(names) and all(n in fa.ALL_SIGNATURES for n in names)
    assert set(fa.KVCACHE_MLA_SIGNATURES) == {"fa_fwd_kvcache_mla", "fa_fwd_kvcache_mla_workspace_bytes"}
    for name, count in ((FN, 25), (FN + "_workspace_bytes", 5)):                 # the declared argument counts
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, body).group(1)
        assert len(decl.split(",")) == len(fa.KVCACHE_MLA_RAGGED_SIGNATURES[name][1]) == count, name


# ---------------------------------------------------------------- the wrapper's and the binding's refusals
def _args(dtype=BF16, Tq=5, H=4, B=2, page=32, pages=6, mp=3):
    g = torch.Generator().manual_seed(0)
    q = torch.randn(Tq, H, 576, generator=g).to(dtype)
    kv = torch.randn(pages, page, 576, generator=g).to(dtype)
    cu = torch.tensor([0, 2, 5][:B + 1], dtype=torch.int32).as_subclass(OnDevice)
    sl = torch.zeros(B, dtype=torch.int32).as_subclass(OnDevice)
    bt = torch.zeros(B, mp, dtype=torch.int32).as_subclass(OnDevice)
    return q, kv, cu, sl, bt


def test_every_malformed_call_is_refused_with_its_message_in_a_fixed_order():
    import mla_ragged_kvcache as M
    f = M.flash_attention_mla_kvcache_ragged
    q, kv, cu, sl, bt = _args()
    z = lambda *s, **kw: torch.zeros(*s, dtype=kw.get("dtype", BF16))

    def refused(msg, *a, **kw):
        with pytest.raises(AssertionError) as e:
            f(*a, **kw)
        assert str(e.value) == msg, str(e.value)
    # ---- the wrapper, in its order
    refused("q must be a tensor", None, kv, cu, sl, bt)
    refused("cu_seqlens_q must be a tensor", q, kv, [0, 2, 5], sl, bt)
    refused("kv_new must be a tensor or None", q, kv, cu, sl, bt, kv_new=3)
    refused("cu_seqlens_q must be int32 (got torch.int64)", q, kv, cu.long(), sl, bt)
    refused("cu_seqlens_q must be a vector of B + 1 entries, B >= 1 (got shape (1,))", q, kv, cu[:1], sl, bt)
    refused("cu_seqlens_q must be a vector of B + 1 entries, B >= 1 (got shape (1, 3))", q, kv, cu[None], sl, bt)
    refused("block_table must be int32 (got torch.int64)", q, kv, cu, sl, bt.long())
    refused("block_table must be [B, max_pages_per_seq] with B = 2, the sequences of cu_seqlens_q", q, kv, cu, sl, bt[:1])
    refused("cache_seqlens must be int32 (got torch.int64)", q, kv, cu, sl.long(), bt)
    refused("cache_seqlens must have B = 2 entries, the sequences of cu_seqlens_q", q, kv, cu, sl[:1], bt)
    host = lambda t: t.as_subclass(torch.Tensor)
    refused("cu_seqlens_q must be a device tensor: the kernels read it, the host never does", q, kv, host(cu), sl, bt)
    refused("cache_seqlens must be a device tensor: the kernels read it, the host never does", q, kv, cu, host(sl), bt)
    refused("block_table must be a device tensor: the kernels read it, the host never does", q, kv, cu, sl, host(bt))
    refused("softmax_scale must be finite and > 0", q, kv, cu, sl, bt, softmax_scale=0.0)
    refused("softmax_scale must be finite and > 0", q, kv, cu, sl, bt, softmax_scale=float("inf"))
    qg, kvg = q.float().requires_grad_(True), kv.float().requires_grad_(True)
    refused("flash_attention_mla_kvcache_ragged has no backward: q must not require grad", qg, kv, cu, sl, bt)
    refused("flash_attention_mla_kvcache_ragged has no backward: kv_cache must not require grad", q, kvg, cu, sl, bt)
    refused("flash_attention_mla_kvcache_ragged has no backward: q, kv_cache, kv_new must not require grad", qg, kvg, cu, sl, bt,
            kv_new=torch.zeros(5, 576, requires_grad=True))
    # the wrapper's order: cu_seqlens_q before block_table before cache_seqlens before the scale before grad
    refused("cu_seqlens_q must be int32 (got torch.int64)", q, kv, cu.long(), sl.long(), bt.long())
    refused("block_table must be int32 (got torch.int64)", q, kv, cu, sl.long(), bt.long())
    refused("cache_seqlens must be int32 (got torch.int64)", qg, kv, cu, sl.long(), bt, softmax_scale=-1.0)
    refused("softmax_scale must be finite and > 0", qg, kv, cu, sl, bt, softmax_scale=-1.0)
    # ---- the binding, in its order
    refused("packed q must be [total_q, H, 576] (got 4 dims)", q[None], kv, cu, sl, bt)
    refused("packed q's last dim must be 576: 512 latent dims, then 64 RoPE dims (got 512)", q[..., :512], kv, cu, sl, bt)
    refused("kv_cache must be [num_pages, page_size, 576]: one latent head, as flash_attention_mla_kvcache takes it (got 4 dims)",
            q, kv[:, None], cu, sl, bt)
    refused("kv_cache's last dim must be 576, as packed q's (got 512)", q, kv[..., :512], cu, sl, bt)
    refused("packed q's dtype must be float16 or bfloat16 (flash_attention_mla_kvcache_ragged)", q.float(), kv.float(), cu, sl, bt)
    refused("kv_cache must have packed q's dtype", q, kv.to(F16), cu, sl, bt)
    refused("packed q and kv_cache must not be empty", q[:0], kv, cu, sl, bt)
    refused("the page size of the latent pool (kv_cache.shape[1] = 48) must be a positive multiple of 32", q, z(4, 48, 576), cu, sl, bt)
    refused("the page size of the latent pool (kv_cache.shape[1] = 16) must be a positive multiple of 32", q, kv[:, :16], cu, sl, bt)
    refused("cu_seqlens_q must be a contiguous int32 vector of B + 1 entries", q, kv,
            torch.zeros(6, dtype=torch.int32)[::2].as_subclass(OnDevice), sl, bt)
    refused("cache_seqlens must be a contiguous int32 vector of B entries (cu_seqlens_q has B + 1)", q, kv, cu,
            torch.zeros(4, dtype=torch.int32)[::2].as_subclass(OnDevice), bt)
    refused("block_table must be an int32 tensor [B, max_pages_per_seq] with unit stride along the pages", q, kv, cu, sl,
            torch.zeros(2, 6, dtype=torch.int32)[:, ::2].as_subclass(OnDevice))
    odd = z(6, 32, 580)[..., :576]
    refused("the latent pool must be addressable in place: unit stride along the 576 dims, 16-byte aligned rows (a row stride that "
            "is a multiple of 8 elements, got 580) and a page stride that is a multiple of 8 elements", q, odd, cu, sl, bt)
    for bad in (z(4, 576), z(5, 512), z(5, 1, 576)):
        refused("kv_new must be [total_q, 576]: one cached row per packed query row", q, kv, cu, sl, bt, kv_new=bad)
    refused("kv_new must have packed q's dtype and must not require grad", q, kv, cu, sl, bt, kv_new=z(5, 576, dtype=F16))
    for bad in (z(5, 4, 576), z(4, 4, 512), z(5, 4, 512, dtype=F16), z(1, 5, 4, 512)):
        refused("out must be [total_q, H, 512] in packed q's dtype", q, kv, cu, sl, bt, out=bad)
    msg = ("out must be addressable in place (unit stride along the 512 dims, row and head strides that are multiples of 8 "
           "elements, at least 512 and below 2^30) and must not require grad")
    refused(msg, q, kv, cu, sl, bt, out=z(5, 4, 1024)[..., ::2])
    refused(msg, q, kv, cu, sl, bt, out=z(5, 1, 512).expand(5, 4, 512))
    refused(msg, q, kv, cu, sl, bt, out=z(5, 4, 516)[..., :512])
    wide = z(6, 32, 640)[..., :576]                                             # 640: fine, the device check is reached
    refused("packed q, kv_cache, cu_seqlens_q, cache_seqlens and block_table must be device tensors", q, wide, cu, sl, bt)
    refused("packed q, kv_cache, cu_seqlens_q, cache_seqlens and block_table must be device tensors", q, kv, cu, sl, bt,
            kv_new=z(5, 576), out=z(7, 4, 640)[:5, :, :512])
    # the binding's order: q before kv_cache, shapes before dtypes before the page size before the vectors before the pool's
    # strides before kv_new before out before the device
    refused("packed q must be [total_q, H, 576] (got 4 dims)", q[None], kv[..., :512], cu, sl, bt)
    refused("kv_cache's last dim must be 576, as packed q's (got 512)", q.float(), kv[..., :512], cu, sl, bt)
    refused("kv_cache must have packed q's dtype", q, z(4, 48, 576, dtype=F16), cu, sl, bt)
    refused("the page size of the latent pool (kv_cache.shape[1] = 48) must be a positive multiple of 32", q, z(4, 48, 580)[..., :576],
            cu, sl, bt, kv_new=z(4, 576))
    refused("the latent pool must be addressable in place: unit stride along the 576 dims, 16-byte aligned rows (a row stride that "
            "is a multiple of 8 elements, got 580) and a page stride that is a multiple of 8 elements", q, odd, cu, sl, bt, kv_new=z(4, 576))
    refused("kv_new must be [total_q, 576]: one cached row per packed query row", q, kv, cu, sl, bt, kv_new=z(4, 576), out=z(5, 4, 576))
    refused("out must be [total_q, H, 512] in packed q's dtype", q, kv, cu, sl, bt, kv_new=z(5, 576), out=z(5, 4, 576))


# ---------------------------------------------------------------- the C entry points
def _call(fa, p, **kw):
    a = dict(q=p, kv=p, new=None, cu=p, sl=p, bt=p, o=p, lse=p, ws=p, wsb=1 << 30, Tq=9, B=2, H=16, pages=8, page=64, mp=4, bts=4,
             has_new=0, dtype=fa.BF16, scale=576 ** -0.5, causal=1, qs=None, ks=None, os=None)
    a.update(kw)
    return fa.lib.fa_fwd_kvcache_mla_ragged(a["q"], a["kv"], a["new"], a["cu"], a["sl"], a["bt"], a["o"], a["lse"], a["ws"], a["wsb"],
                                            a["Tq"], a["B"], a["H"], a["pages"], a["page"], a["mp"], a["bts"], a["has_new"], a["dtype"],
                                            a["scale"], a["causal"], a["qs"], a["ks"], a["os"], None)


def test_c_refusals_name_the_argument_and_carry_the_value():
    fa = _lib()
    buf, p = vck.aligned_ptr()
    st = lambda *v: (ctypes.c_longlong * len(v))(*v)
    cases = [
        (dict(q=None), NULL, "q is NULL (argument 1)"),
        (dict(kv=None), NULL, "kv_pool is NULL (argument 2)"),
        (dict(cu=None), NULL, "cu_seqlens_q is NULL (argument 4)"),
        (dict(sl=None), NULL, "cache_seqlens is NULL (argument 5)"),
        (dict(bt=None), NULL, "block_table is NULL (argument 6)"),
        (dict(o=None), NULL, "o is NULL (argument 7)"),
        (dict(has_new=2), SHAPE, "has_new must be 0 or 1 (got 2)"),
        (dict(has_new=1), NULL, "has_new = 1 needs kv_new (has_new 1)"),
        (dict(new=p), SHAPE, "kv_new given with has_new = 0 (has_new 0)"),
        (dict(dtype=2), DTYPE, "dtype must be 0 (fp16) or 1 (bf16) (got 2)"),
        (dict(causal=2), SHAPE, "causal must be 0 or 1 (got 2)"),
        (dict(scale=0.0), SHAPE, "scale must be finite and > 0 (its bits are 0)"),
        (dict(scale=float("inf")), SHAPE, "scale must be finite and > 0 (its bits are 2139095040)"),
        (dict(Tq=0), SHAPE, "total_q must be >= 1 (got 0)"),
        (dict(B=0), SHAPE, "B must be >= 1 (got 0)"),
        (dict(H=0), SHAPE, "H must be >= 1 (got 0)"),
        (dict(H=1 << 20, Tq=32), SHAPE, "too many query rows for one launch: H * total_q is at most 2^24 (got 33554432)"),
        (dict(B=(1 << 24) + 1), SHAPE, "too many sequences for one launch: B is at most 2^24 (got 16777217)"),
        (dict(page=48), PAGED, "page_size must be a positive multiple of 32 (got 48)"),
        (dict(page=0), PAGED, "page_size must be a positive multiple of 32 (got 0)"),
        (dict(mp=0, bts=0), PAGED, "max_pages_per_seq must be >= 1 (got 0)"),
        (dict(mp=1 << 26, bts=1 << 26), PAGED, "max_pages_per_seq * page_size must stay below 2^31 (got 4294967296)"),
        (dict(pages=0), PAGED, "num_pages must be >= 1 (got 0)"),
        (dict(bts=3), PAGED, "block_table_stride must be at least max_pages_per_seq and below 2^31 (got 3)"),
        (dict(qs=st(9216, 580)), STRIDE, "q_strides must be non-negative multiples of 8 elements below 2^30 (got 580)"),
        (dict(qs=st(1 << 30, 576)), STRIDE, "q_strides must be non-negative multiples of 8 elements below 2^30 (got 1073741824)"),
        (dict(qs=st(512, 576)), STRIDE, "the row stride of q must be at least 576 elements (got 512)"),
        (dict(os=st(-8, 512)), STRIDE, "o_strides must be non-negative multiples of 8 elements below 2^30 (got -8)"),
        (dict(os=st(504, 512)), STRIDE, "the row stride of o must be at least 512 elements (got 504)"),
        (dict(os=st(8192, 0)), STRIDE, "o_strides: an output cannot have a zero head stride (head stride 0)"),
        (dict(ks=st(36868, 576)), STRIDE, "the page stride of kv_pool must be a non-negative multiple of 8 elements (got 36868)"),
        (dict(ks=st(36864, 580)), STRIDE, "the row stride of kv_pool must be a multiple of 8 elements (16-byte rows) and at least 576 (got 580)"),
        (dict(ks=st(36864, 568)), STRIDE, "the row stride of kv_pool must be a multiple of 8 elements (16-byte rows) and at least 576 (got 568)"),
        (dict(ks=st(0, 1 << 25)), STRIDE, "one page of kv_pool exceeds 2^31 bytes (row stride 33554432 elements)"),
        (dict(q=p + 8), ALIGN, "q must be 16-byte aligned (ends in 8)"),
        (dict(kv=p + 4), ALIGN, "kv_pool must be 16-byte aligned (ends in 4)"),
        (dict(new=p + 2, has_new=1), ALIGN, "kv_new must be 16-byte aligned (ends in 2)"),
        (dict(o=p + 8), ALIGN, "o must be 16-byte aligned (ends in 8)"),
        (dict(ws=p + 8), ALIGN, "workspace must be 16-byte aligned (ends in 8)"),
        (dict(lse=p + 2), ALIGN, "lse must be 4-byte aligned (ends in 2)"),
        (dict(cu=p + 2), ALIGN, "cu_seqlens_q must be 4-byte aligned (ends in 2)"),
        (dict(sl=p + 2), ALIGN, "cache_seqlens must be 4-byte aligned (ends in 2)"),
        (dict(bt=p + 1), ALIGN, "block_table must be 4-byte aligned (ends in 1)"),
        # pairs of simultaneous faults: the order of the checks
        (dict(q=None, dtype=2), NULL, "q is NULL (argument 1)"),
        (dict(cu=None, sl=None), NULL, "cu_seqlens_q is NULL (argument 4)"),
        (dict(has_new=1, dtype=2), NULL, "has_new = 1 needs kv_new (has_new 1)"),
        (dict(dtype=2, causal=2), DTYPE, "dtype must be 0 (fp16) or 1 (bf16) (got 2)"),
        (dict(causal=2, scale=0.0), SHAPE, "causal must be 0 or 1 (got 2)"),
        (dict(scale=0.0, Tq=0), SHAPE, "scale must be finite and > 0 (its bits are 0)"),
        (dict(Tq=0, B=0), SHAPE, "total_q must be >= 1 (got 0)"),
        (dict(H=0, page=48), SHAPE, "H must be >= 1 (got 0)"),
        (dict(page=48, pages=0), PAGED, "page_size must be a positive multiple of 32 (got 48)"),
        (dict(pages=0, bts=3), PAGED, "num_pages must be >= 1 (got 0)"),
        (dict(bts=3, qs=st(512, 576)), PAGED, "block_table_stride must be at least max_pages_per_seq and below 2^31 (got 3)"),
        (dict(qs=st(512, 576), os=st(504, 512)), STRIDE, "the row stride of q must be at least 576 elements (got 512)"),
        (dict(os=st(504, 512), ks=st(36864, 568)), STRIDE, "the row stride of o must be at least 512 elements (got 504)"),
        (dict(ks=st(36864, 568), q=p + 8), STRIDE,
         "the row stride of kv_pool must be a multiple of 8 elements (16-byte rows) and at least 576 (got 568)"),
        (dict(q=p + 8, ws=None, wsb=0), ALIGN, "q must be 16-byte aligned (ends in 8)"),
    ]
    for kw, code, text in cases:
        assert _call(fa, p, **kw) == code, (kw, fa.lib.fa_last_error())
        assert fa.lib.fa_last_error().decode() == FN + ": " + text, kw
    vck.splits(3)
    need = fa.lib.fa_fwd_kvcache_mla_ragged_workspace_bytes(9, 2, 16, 4, 64)
    assert need == _plan_bytes(16, 9, 2) + 3 * 16 * 9 * 514 * 4
    assert _call(fa, p, wsb=need - 1) == WORKSPACE
    assert fa.lib.fa_last_error().decode() == FN + ": workspace smaller than fa_fwd_kvcache_mla_ragged_workspace_bytes() (%d bytes)" % need
    vck.splits(1)                                                               # one split: the plan alone, still a workspace
    assert _call(fa, p, ws=None, wsb=0) == WORKSPACE
    assert fa.lib.fa_last_error().decode() == FN + ": workspace smaller than fa_fwd_kvcache_mla_ragged_workspace_bytes() (%d bytes)" % _plan_bytes(16, 9, 2)
    # the workspace function refuses what the call refuses about the shape, under its own name
    ws = fa.lib.fa_fwd_kvcache_mla_ragged_workspace_bytes
    assert ws(9, 2, 16, 4, 48) == PAGED
    assert fa.lib.fa_last_error().decode() == FN + "_workspace_bytes: page_size must be a positive multiple of 32 (got 48)"
    assert ws(0, 2, 16, 4, 64) == SHAPE
    assert fa.lib.fa_last_error().decode() == FN + "_workspace_bytes: total_q must be >= 1 (got 0)"
    assert ws(9, 0, 16, 4, 64) == SHAPE and ws(9, 2, 0, 4, 64) == SHAPE and ws(9, 2, 16, 0, 64) == PAGED


def _nb_max(H, Tq, B):
    return (H * Tq + 31 * B) // 32


def _plan_bytes(H, Tq, B):
    return (16 + 8 * _nb_max(H, Tq, B) + 15) // 16 * 16


def packed_splits_formula(Tq, B, H, S_cache):
    """mla_splits over nb_max workgroups per split: tests/test_host_mla.py splits_formula counts B * ceil(H * S_q / 32), so a
    launch of nb_max sequences with H * S_q = 32 is the same count"""
    return splits_formula(_nb_max(H, Tq, B), 32, 1, S_cache)


def test_workspace_bytes_follow_the_formula_and_the_forced_count():
    fa = _lib()
    ws = fa.lib.fa_fwd_kvcache_mla_ragged_workspace_bytes
    seen = set()
    for Tq, B, H, mp, page in [(1, 1, 1, 1, 32), (8, 8, 128, 256, 64), (8, 8, 16, 256, 64), (20, 8, 128, 256, 64), (80, 32, 16, 64, 64),
                               (1, 1, 16, 2048, 64), (287, 32, 16, 64, 64), (13, 9, 24, 11, 64), (53, 9, 128, 4, 128), (600, 600, 16, 100, 32)]:
        n = packed_splits_formula(Tq, B, H, mp * page)
        seen.add(n)
        assert ws(Tq, B, H, mp, page) == _plan_bytes(H, Tq, B) + (n * H * Tq * 514 * 4 if n > 1 else 0), (Tq, B, H, mp, page, n)
        for forced in (1, 2, 7):
            vck.splits(forced)
            assert ws(Tq, B, H, mp, page) == _plan_bytes(H, Tq, B) + (forced * H * Tq * 514 * 4 if forced > 1 else 0)
        vck.splits(0)
    assert {1, 64} <= seen and len(seen) >= 5, seen


# ---------------------------------------------------------------- the kernels
def test_new_kernels_are_in_the_library_inside_the_decode_budget():
    """The <Latent, T> overloads of fa_decode_ragged_kernel, fa_kvcache_append_ragged_kernel and fa_decode_combine_ragged_kernel
    over LatentRaggedParams -- overloads of stems the race tables already claim (tests/test_host_racecheck.py), lower-case and
    without an `int 512` argument (tests/test_host_mla.py) --, two dtypes each and nothing else new: workgroup 256, VGPR + AGPR <=
    256, no scratch, no spills, LDS within 80 KiB; the three rectangular stems still at two instances each."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj
    new = {"fa_decode_ragged_kernel": 0, "fa_kvcache_append_ragged_kernel": 0, "fa_decode_combine_ragged_kernel": 0}
    old = {"fa_decode_paged_kernel": 0, "fa_kvcache_append_paged_kernel": 0, "fa_decode_combine_kernel": 0}
    for k in codeobj.kernels():
        m = re.match(r"_ZN2fa\d+(fa_\w+?_kernel)INS_6LatentENS_4(?:BF16|FP16)EEEvNS_18LatentRaggedParamsE$", k["name"])
        if m:
            assert m.group(1) in new, k["name"]
            new[m.group(1)] += 1
            assert k["wg"] == 256 and k["vgpr"] + k["agpr"] <= 256, (k["name"], k["vgpr"], k["agpr"])
            assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 81920, k["name"]
            continue
        assert "Latent" not in k["name"], "a packed MLA kernel outside the expected set: " + k["name"]
        m = re.match(r"_ZN2fa\d+(fa_\w+?_kernel)I(NS_3MLAENS_4(?:BF16|FP16)E|Li512ENS_4(?:BF16|FP16)E)EEv", k["name"])
        if m:
            old[m.group(1)] += 1
    assert new == dict.fromkeys(new, 2), new
    assert old == dict.fromkeys(old, 2), old
    src = open(os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd", "csrc", "fa_decode_mla.hip")).read()
    assert 'static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU")' in src
    assert src.count('#include "fa_decode_mla_body.inc"') == 2                  # one body, the rectangular and the packed kernel


# ---------------------------------------------------------------- the packing helper of the GPU tests
@pytest.mark.parametrize("append", [False, True], ids=["noappend", "append"])
def test_packing_helper_agrees_with_mlacheck_truth(append):
    """the per-sequence truths, packed and unpacked again, are mc.truth of a rectangular problem built by hand; a packed result
    made from the truth passes held(), and one with two rows swapped does not"""
    seqs = [(0, 7), (2, 3), (1, 0), (3, 40), (0, 0)]
    step = mr.Step(seqs, 3, F16, append, seed=5, device="cpu", pad=2)
    assert step.cu_list == [0, 0, 2, 3, 6, 6] and step.total_q == 8 and step.Ls == ([7, 5, 1, 43, 0] if append else [7, 3, 0, 40, 0])
    assert torch.isnan(step.qp[6:].float()).all() and torch.isnan(step.new[6:].float()).all()
    for causal in (False, True):
        truths = step.truth(causal)
        assert [t is None for t in truths] == [True, False, False, False, True]
        for b, (s, f) in enumerate(seqs):
            if not s:
                continue
            # by hand: the packed rows of b, head-major, over the first L_b rows of its cache
            qb = step.qp[step.cu_list[b]:step.cu_list[b + 1]].transpose(0, 1)[None]
            assert torch.equal(qb, step.q[b])
            assert torch.equal(step.new[step.cu_list[b]:step.cu_list[b + 1]], step.kv[b, f:f + s])
            O, LSE = mc.truth(qb, step.kv[b:b + 1], [step.Ls[b]], causal)
            assert torch.equal(O, truths[b][0]) and torch.equal(LSE, truths[b][1])
            if step.Ls[b] == 0:
                assert (O == 0).all() and torch.isneginf(LSE).all()
        live = [t for t in truths if t is not None]
        o = mr.pack_rows([t[0].to(F16) for t in live], step.total_q, 7.0)
        lse = mr.pack_lse([t[1].float() for t in live], step.total_q, 7.0)
        assert (o[6:] == 7).all() and (lse[:, 6:] == 7).all()
        for b in (1, 2, 3):
            ob, lb = mr.unpack(o, lse, step.cu_list, b)
            assert torch.equal(ob, truths[b][0].to(F16)) and torch.equal(lb, truths[b][1].float())
            assert mr.same_rows(o, lse, step.cu_list, b, (truths[b][0].to(F16), truths[b][1].float()))
        mr.held("helper", step, o, lse, truths)
        bad = o.clone()
        bad[3], bad[4] = o[4], o[3]
        with pytest.raises(AssertionError):
            mr.held("helper swapped", step, bad, lse, truths)
    before, table, after = step.pools(32, 3, 1, row_stride=640)
    assert before.stride(1) == 640 and before.shape == after.shape
    same = torch.equal(torch.nan_to_num(before.float(), nan=-7.0), torch.nan_to_num(after.float(), nan=-7.0))
    assert same == (not append)


# ---------------------------------------------------------------- the reference-only condition of the GPU scale test
def test_the_scale_of_the_gpu_test_is_far_from_the_default():
    from test_gpu_mla_ragged import SCALE, SCALE_SEQS, SCALE_QMUL
    assert SCALE == 192 ** -0.5
    for dtype in (F16, BF16):
        step = mr.Step(SCALE_SEQS, 16, dtype, True, seed=95, device="cpu")
        step.q = [(x.float() * SCALE_QMUL).to(dtype) for x in step.q]
        for a, b in zip(step.truth(True, SCALE), step.truth(True)):
            if a is not None:
                far = fo.rel_fro(b[0], a[0])
                assert far >= mc.FAR, far
                assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
