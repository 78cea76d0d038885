"""CPU tests of MLA decoding over a paged latent cache (include_mla/mi355fa_kvcache_mla.h, mla_kvcache.py): the Python and
binding signatures, every refusal with its exact message, the workspace function against its formula, the ABI version and
header listings, the new kernels' resources from the code objects, and the reference-only condition of the GPU scale test."""
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
import variantcheck as vck

BF16, F16 = torch.bfloat16, torch.float16
NULL, SHAPE, DTYPE, ALIGN, STRIDE, WORKSPACE, PAGED = -1, -2, -4, -5, -6, -9, -12


def _lib():
    import _mi355fa as fa
    return fa


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


# ---------------------------------------------------------------- surface
def test_python_and_binding_signatures():
    import mla_kvcache as M
    import _mi355fa_mla_torch as ext
    assert M.__all__ == ["flash_attention_mla_kvcache", "MLA_D", "MLA_DV"] and (M.MLA_D, M.MLA_DV) == (576, 512)
    sig = inspect.signature(M.flash_attention_mla_kvcache)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [
        ("q", inspect.Parameter.empty), ("kv_cache", inspect.Parameter.empty), ("cache_seqlens", inspect.Parameter.empty),
        ("block_table", inspect.Parameter.empty), ("kv_new", None), ("is_causal", False), ("softmax_scale", None),
        ("return_lse", False), ("out", None)]
    assert "(128 + 64) ** -0.5" in M.flash_attention_mla_kvcache.__doc__ and "576 ** -0.5" in M.flash_attention_mla_kvcache.__doc__
    assert [n for n in dir(ext) if not n.startswith("_")] == ["kvcache_mla_forward"]
    doc = ext.kvcache_mla_forward.__doc__
    args = re.search(r"kvcache_mla_forward\((.*?)\) ->", doc, re.S).group(1)
    assert re.findall(r"(\w+): ", args) == ["q", "kv_cache", "cache_seqlens", "block_table", "kv_new", "is_causal", "softmax_scale", "out"]


def test_abi_headers_and_ctypes_signatures():
    fa = _lib()
    assert fa.lib.fa_abi_version() == 7 and fa.ABI_VERSION == 7
    assert re.search(r"#define\s+MI355FA_ABI_VERSION\s+7\b", open(os.path.join(ROOT, "include", "mi355fa.h")).read())
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(
        "mi355fa%s.h" % s for s in ("", "_alibi", "_gqa", "_kvcache", "_kvcache_fp4", "_kvcache_fp8", "_kvcache_fp8_token", "_local",
                                    "_paged", "_ragged", "_ragged_fp4", "_sink", "_softcap"))
    assert os.listdir(os.path.join(ROOT, "include_quant")) == ["mi355fa_kvcache_quant_softcap.h"]
    assert os.listdir(os.path.join(ROOT, "include_mla")) == ["mi355fa_kvcache_mla.h"]
    txt, body, names = vck.header_functions(os.path.join(ROOT, "include_mla", "mi355fa_kvcache_mla.h"))
    assert names == ["fa_fwd_kvcache_mla", "fa_fwd_kvcache_mla_workspace_bytes"]
    assert re.search(r"#define\s+MI355FA_MLA_D\s+576\b", body) and re.search(r"#define\s+MI355FA_MLA_DV\s+512\b", body)
    assert "(128 + 64) ** -0.5" in txt
    assert set(fa.KVCACHE_MLA_SIGNATURES) == set(names) and all(n in fa.ALL_SIGNATURES for n in names)
    for name in names:                                                          # the declared argument counts
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, body).group(1)
        assert len(decl.split(",")) == len(fa.KVCACHE_MLA_SIGNATURES[name][1]), name


# ---------------------------------------------------------------- the wrapper's and the binding's refusals
def _args(dtype=BF16, B=2, H=4, Sq=2, page=32, pages=6, mp=3):
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B, H, Sq, 576, generator=g).to(dtype)
    kv = torch.randn(pages, page, 576, generator=g).to(dtype)
    sl = torch.zeros(B, dtype=torch.int32).as_subclass(OnDevice)
    bt = torch.zeros(B, mp, dtype=torch.int32).as_subclass(OnDevice)
    return q, kv, sl, bt


class OnDevice(torch.Tensor):
    """a host tensor that tells the Python wrapper it lives on the device: the checks behind the wrapper's device check are
    reached without a GPU (the binding sees the host tensor it is, and refuses it last)"""
    is_cuda = property(lambda self: True)


def test_every_malformed_call_is_refused_with_its_message():
    import mla_kvcache as M
    f = M.flash_attention_mla_kvcache
    q, kv, sl, bt = _args()

    def refused(msg, *a, **kw):
        with pytest.raises(AssertionError) as e:
            f(*a, **kw)
        assert str(e.value) == msg, str(e.value)
    refused("q's last dim must be 576: 512 latent dims, then 64 RoPE dims (got 512)", q[..., :512], kv, sl, bt)
    refused("q must be [B, H, S_q, 576] (got 3 dims)", q[0], kv, sl, bt)
    refused("kv_cache's last dim must be 576 (got 512)", q, kv[..., :512], sl, bt)
    refused("kv_cache must be [num_pages, page_size, 576]: one latent head (got 4 dims)", q, kv[:, None], sl, bt)
    refused("kv_cache must have q's dtype", q, kv.to(F16), sl, bt)
    refused("q's dtype must be float16 or bfloat16", q.float(), kv.float(), sl, bt)
    refused("the page size (kv_cache.shape[1] = 48) must be a positive multiple of 32", q, torch.zeros(4, 48, 576, dtype=BF16), sl, bt)
    refused("the page size (kv_cache.shape[1] = 16) must be a positive multiple of 32", q, kv[:, :16], sl, bt)
    refused("cache_seqlens must be int32 (got torch.int64)", q, kv, sl.long(), bt)
    refused("block_table must be int32 (got torch.int64)", q, kv, sl, bt.long())
    refused("cache_seqlens must be a contiguous int32 vector of B entries", q, kv, sl[:1], bt)
    refused("block_table must be an int32 tensor [B, max_pages_per_seq] with unit stride along the pages", q, kv, sl, bt[:1])
    refused("kv_new must be [B, S_q, 576]: one cached row per query row", q, kv, sl, bt, kv_new=torch.zeros(2, 3, 576, dtype=BF16))
    refused("kv_new must be [B, S_q, 576]: one cached row per query row", q, kv, sl, bt, kv_new=torch.zeros(2, 2, 512, dtype=BF16))
    refused("kv_new must be [B, S_q, 576]: one cached row per query row", q, kv, sl, bt, kv_new=torch.zeros(2, 1, 2, 576, dtype=BF16))
    refused("kv_new must have q's dtype and must not require grad", q, kv, sl, bt, kv_new=torch.zeros(2, 2, 576, dtype=F16))
    refused("out must be [B, H, S_q, 512] in q's dtype", q, kv, sl, bt, out=torch.zeros(2, 4, 2, 576, dtype=BF16))
    refused("softmax_scale must be finite and > 0", q, kv, sl, bt, softmax_scale=0.0)
    refused("softmax_scale must be finite and > 0", q, kv, sl, bt, softmax_scale=float("inf"))
    refused("q must be a tensor", None, kv, sl, bt)
    # inference only: by argument name, as paged_kvcache._check_no_grad words it
    qg, kvg = q.float().requires_grad_(True), kv.float().requires_grad_(True)
    refused("flash_attention_mla_kvcache has no backward: q must not require grad", qg, kv, sl, bt)
    refused("flash_attention_mla_kvcache has no backward: kv_cache must not require grad", q, kvg, sl, bt)
    refused("flash_attention_mla_kvcache has no backward: q, kv_cache, kv_new must not require grad", qg, kvg, sl, bt,
            kv_new=torch.zeros(2, 2, 576, requires_grad=True))
    # a row stride the kernels cannot address: rows must stay 16-byte aligned
    odd = torch.zeros(6, 32, 580, dtype=BF16)[..., :576]
    refused("kv_cache must be addressable in place: unit stride along the 576 dims, 16-byte aligned rows (a row stride that is a "
            "multiple of 8 elements, got 580) and a page stride that is a multiple of 8 elements", q, odd, sl, bt)
    wide = torch.zeros(6, 32, 640, dtype=BF16)[..., :576]                       # 640: fine, the next refusal is reached
    # host-resident cache_seqlens / block_table: the kernels read them, the host never does
    host = lambda t: t.as_subclass(torch.Tensor)
    refused("cache_seqlens must be a device tensor: the kernels read it, the host never does", q, kv, host(sl), bt)
    refused("block_table must be a device tensor: the kernels read it, the host never does", q, kv, sl, host(bt))
    refused("q, kv_cache, cache_seqlens and block_table must be device tensors", q, wide, sl, bt)


# ---------------------------------------------------------------- the C entry points
def _call(fa, p, **kw):
    a = dict(q=p, kv=p, new=None, sl=p, bt=p, o=p, lse=p, ws=p, wsb=1 << 30, B=2, H=16, Sq=1, pages=8, page=64, mp=4, bts=4, Snew=0,
             dtype=fa.BF16, scale=576 ** -0.5, causal=1, qs=None, ks=None, os=None)
    a.update(kw)
    return fa.lib.fa_fwd_kvcache_mla(a["q"], a["kv"], a["new"], a["sl"], a["bt"], a["o"], a["lse"], a["ws"], a["wsb"], a["B"], a["H"],
                                     a["Sq"], a["pages"], a["page"], a["mp"], a["bts"], a["Snew"], a["dtype"], a["scale"], a["causal"],
                                     a["qs"], a["ks"], a["os"], None)


def test_c_refusals_name_the_argument_and_carry_the_value():
    fa = _lib()
    buf, p = vck.aligned_ptr()
    st = lambda *v: (ctypes.c_longlong * len(v))(*v)
    cases = [
        (dict(q=None), NULL, "fa_fwd_kvcache_mla: q is NULL (argument 1)"),
        (dict(kv=None), NULL, "fa_fwd_kvcache_mla: kv_pool is NULL (argument 2)"),
        (dict(sl=None), NULL, "fa_fwd_kvcache_mla: cache_seqlens is NULL (argument 4)"),
        (dict(bt=None), NULL, "fa_fwd_kvcache_mla: block_table is NULL (argument 5)"),
        (dict(o=None), NULL, "fa_fwd_kvcache_mla: o is NULL (argument 6)"),
        (dict(Snew=2), NULL, "fa_fwd_kvcache_mla: S_new > 0 needs kv_new (S_new 2)"),
        (dict(new=p), SHAPE, "fa_fwd_kvcache_mla: kv_new given with S_new < 1 (S_new 0)"),
        (dict(dtype=2), DTYPE, "fa_fwd_kvcache_mla: dtype must be 0 (fp16) or 1 (bf16) (got 2)"),
        (dict(causal=2), SHAPE, "fa_fwd_kvcache_mla: causal must be 0 or 1 (got 2)"),
        (dict(scale=0.0), SHAPE, "fa_fwd_kvcache_mla: scale must be finite and > 0 (its bits are 0)"),
        (dict(scale=float("inf")), SHAPE, "fa_fwd_kvcache_mla: scale must be finite and > 0 (its bits are 2139095040)"),
        (dict(B=0), SHAPE, "fa_fwd_kvcache_mla: B must be >= 1 (got 0)"),
        (dict(H=0), SHAPE, "fa_fwd_kvcache_mla: H must be >= 1 (got 0)"),
        (dict(Sq=0), SHAPE, "fa_fwd_kvcache_mla: S_q must be >= 1 (got 0)"),
        (dict(Snew=-1), SHAPE, "fa_fwd_kvcache_mla: S_new must be >= 0 (got -1)"),
        (dict(H=1 << 20, Sq=32), SHAPE, "fa_fwd_kvcache_mla: too many query rows for one launch: H * S_q is at most 2^24 (got 33554432)"),
        (dict(page=48), PAGED, "fa_fwd_kvcache_mla: page_size must be a positive multiple of 32 (got 48)"),
        (dict(page=0), PAGED, "fa_fwd_kvcache_mla: page_size must be a positive multiple of 32 (got 0)"),
        (dict(mp=0, bts=0), PAGED, "fa_fwd_kvcache_mla: max_pages_per_seq must be >= 1 (got 0)"),
        (dict(mp=1 << 26, bts=1 << 26), PAGED, "fa_fwd_kvcache_mla: max_pages_per_seq * page_size must stay below 2^31 (got 4294967296)"),
        (dict(pages=0), PAGED, "fa_fwd_kvcache_mla: num_pages must be >= 1 (got 0)"),
        (dict(bts=3), PAGED, "fa_fwd_kvcache_mla: block_table_stride must be at least max_pages_per_seq and below 2^31 (got 3)"),
        (dict(qs=st(0, 580, 576)), STRIDE, "fa_fwd_kvcache_mla: q_strides must be non-negative multiples of 8 elements (got 580)"),
        (dict(qs=st(0, 0, 512)), STRIDE,
         "fa_fwd_kvcache_mla: the row stride of q must be at least 576 elements, one (batch, head) slice below 2^31 bytes (got 512)"),
        (dict(os=st(8192, 512, -8)), STRIDE, "fa_fwd_kvcache_mla: o_strides must be non-negative multiples of 8 elements (got -8)"),
        (dict(os=st(8192, 512, 504)), STRIDE,
         "fa_fwd_kvcache_mla: the row stride of o must be at least 512 elements, one (batch, head) slice below 2^31 bytes (got 504)"),
        (dict(os=st(8192, 0, 512)), STRIDE, "fa_fwd_kvcache_mla: o_strides: an output cannot have a zero batch / head stride (head stride 0)"),
        (dict(ks=st(36868, 576)), STRIDE, "fa_fwd_kvcache_mla: the page stride of kv_pool must be a non-negative multiple of 8 elements (got 36868)"),
        (dict(ks=st(36864, 580)), STRIDE,
         "fa_fwd_kvcache_mla: the row stride of kv_pool must be a multiple of 8 elements (16-byte rows) and at least 576 (got 580)"),
        (dict(ks=st(36864, 568)), STRIDE,
         "fa_fwd_kvcache_mla: the row stride of kv_pool must be a multiple of 8 elements (16-byte rows) and at least 576 (got 568)"),
        (dict(ks=st(0, 1 << 25)), STRIDE, "fa_fwd_kvcache_mla: one page of kv_pool exceeds 2^31 bytes (row stride 33554432 elements)"),
        (dict(q=p + 8), ALIGN, "fa_fwd_kvcache_mla: q must be 16-byte aligned (ends in 8)"),
        (dict(kv=p + 4), ALIGN, "fa_fwd_kvcache_mla: kv_pool must be 16-byte aligned (ends in 4)"),
        (dict(new=p + 2, Snew=1), ALIGN, "fa_fwd_kvcache_mla: kv_new must be 16-byte aligned (ends in 2)"),
        (dict(o=p + 8), ALIGN, "fa_fwd_kvcache_mla: o must be 16-byte aligned (ends in 8)"),
        (dict(ws=p + 8), ALIGN, "fa_fwd_kvcache_mla: workspace must be 16-byte aligned (ends in 8)"),
        (dict(lse=p + 2), ALIGN, "fa_fwd_kvcache_mla: lse must be 4-byte aligned (ends in 2)"),
        (dict(sl=p + 2), ALIGN, "fa_fwd_kvcache_mla: cache_seqlens must be 4-byte aligned (ends in 2)"),
        (dict(bt=p + 1), ALIGN, "fa_fwd_kvcache_mla: block_table must be 4-byte aligned (ends in 1)"),
    ]
    for kw, code, text in cases:
        assert _call(fa, p, **kw) == code, (kw, fa.lib.fa_last_error())
        assert fa.lib.fa_last_error().decode() == text, kw
    vck.splits(3)
    need = fa.lib.fa_fwd_kvcache_mla_workspace_bytes(2, 16, 1, 4, 64, 0)
    assert need == 3 * 2 * 16 * 1 * 514 * 4
    assert _call(fa, p, wsb=need - 1) == WORKSPACE
    assert fa.lib.fa_last_error().decode() == "fa_fwd_kvcache_mla: workspace smaller than fa_fwd_kvcache_mla_workspace_bytes() (%d bytes)" % need
    assert _call(fa, p, ws=None, wsb=0) == WORKSPACE
    # the workspace function refuses what the call refuses about the shape, under its own name
    assert fa.lib.fa_fwd_kvcache_mla_workspace_bytes(2, 16, 1, 4, 48, 0) == PAGED
    assert fa.lib.fa_last_error().decode() == "fa_fwd_kvcache_mla_workspace_bytes: page_size must be a positive multiple of 32 (got 48)"
    assert fa.lib.fa_fwd_kvcache_mla_workspace_bytes(0, 16, 1, 4, 64, 0) == SHAPE


def splits_formula(B, H, Sq, S_cache):
    """csrc/fa_decode_mla.hip mla_splits: at most two workgroups per CU over (sequence, 32-row block, split), splits of at
    least sqrt(16 * S_cache) keys, at most 64"""
    wgs = max(1, B * ((H * Sq + 31) // 32))
    n = (512 + wgs - 1) // wgs
    by_len = 1
    while (by_len + 1) ** 2 * 16 <= S_cache:
        by_len += 1
    return max(1, min(n, by_len, 64))


def test_workspace_bytes_follow_the_formula_and_the_forced_count():
    fa = _lib()
    ws = fa.lib.fa_fwd_kvcache_mla_workspace_bytes
    seen = set()
    for B, H, Sq, mp, page in [(1, 1, 1, 1, 32), (8, 128, 1, 256, 64), (8, 16, 1, 256, 64), (8, 128, 2, 256, 64), (32, 16, 1, 64, 64),
                               (1, 16, 1, 2048, 64), (64, 128, 3, 8, 128), (3, 24, 3, 11, 64), (1, 128, 1, 1, 32), (600, 16, 1, 100, 32)]:
        n = splits_formula(B, H, Sq, mp * page)
        seen.add(n)
        for S_new in (0, Sq):
            assert ws(B, H, Sq, mp, page, S_new) == (n * B * H * Sq * (512 + 2) * 4 if n > 1 else 0), (B, H, Sq, mp, page, n)
        for forced in (1, 2, 7):
            vck.splits(forced)
            assert ws(B, H, Sq, mp, page, 0) == (forced * B * H * Sq * 514 * 4 if forced > 1 else 0)
        vck.splits(0)
    assert {1, 64} <= seen and len(seen) >= 5


# ---------------------------------------------------------------- the kernels
def test_new_kernels_are_in_the_library_inside_the_decode_budget():
    """<MLA, T> overloads of fa_decode_paged_kernel and fa_kvcache_append_paged_kernel and the <512, T> instances of the shared
    combine kernel, two dtypes each and nothing else new: workgroup 256, VGPR + AGPR <= 256, no scratch, no spills, LDS within
    80 KiB (the attention kernel's carve is dynamic: csrc/fa_decode_mla.hip static_asserts it)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj
    found = {}
    for k in codeobj.kernels():
        m = re.match(r"_ZN2fa\d+(fa_\w+?_kernel)I(NS_3MLAENS_4(?:BF16|FP16)E|Li512ENS_4(?:BF16|FP16)E)EEv", k["name"])
        if not m and ("MLA" in k["name"] or "Mla" in k["name"] or "Li512E" in k["name"]):
            raise AssertionError("an MLA kernel outside the expected set: " + k["name"])
        if m:
            found[m.group(1)] = found.get(m.group(1), 0) + 1
            assert k["wg"] == 256 and k["vgpr"] + k["agpr"] <= 256, (k["name"], k["vgpr"], k["agpr"])
            assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 81920, k["name"]
            assert k["name"].endswith("NS_9MlaParamsE") or k["name"].endswith("NS_12DecodeParamsE"), k["name"]
    assert found == {"fa_decode_paged_kernel": 2, "fa_kvcache_append_paged_kernel": 2, "fa_decode_combine_kernel": 2}, found
    src = open(os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd", "csrc", "fa_decode_mla.hip")).read()
    assert 'static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU")' in src


# ---------------------------------------------------------------- the reference-only condition of the GPU scale test
@pytest.mark.parametrize("scale,qmul", [(192 ** -0.5, 1.0), (1.0, 0.125)], ids=["deepseek", "one"])
def test_the_scales_of_the_gpu_test_are_far_from_the_default(scale, qmul):
    lens = [33, 129, 300]
    for dtype in (F16, BF16):
        q, kv = mc.make(len(lens), 16, 2, 320, dtype, seed=95, device="cpu")
        q = (q.float() * qmul).to(dtype)
        O, LSE = mc.truth(q, kv, lens, True, scale)
        far = fo.rel_fro(mc.truth(q, kv, lens, True)[0], O)
        assert far > mc.FAR, far
        assert torch.isfinite(O).all() and torch.isfinite(LSE).all() and O.shape == (3, 16, 2, 512)
