"""CPU tests of MLA decoding over a paged FP8 latent cache (include_mla_fp8/mi355fa_kvcache_mla_fp8.h, mla_fp8_kvcache.py): the
656-byte row of the helpers against a plain fp32 reference, the Python and binding signatures, the refusals with their exact
messages, the workspace function, the header and the signature table, the new kernels' resources from the code objects, and
the reference-only condition of the GPU scale test."""
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
import mlafp8check as f8
import variantcheck as vck
from test_host_mla import OnDevice, splits_formula

BF16, F16 = torch.bfloat16, torch.float16
NULL, SHAPE, DTYPE, ALIGN, STRIDE, WORKSPACE, PAGED = -1, -2, -4, -5, -6, -9, -12


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


# ---------------------------------------------------------------- the row format
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_helpers_write_and_read_the_656_byte_row(dtype):
    F = f8.F()
    kv = torch.randn(3, 5, 576, generator=torch.Generator().manual_seed(1)).to(dtype)
    kv[0, 0, 128:256] = 0                                             # an all-zero block: scale 1.0
    kv[0, 1, :4] = -0.0
    kv[1, 2, 300] = 900.0                                             # one outlier sets its block's scale alone
    kv[2, 4, 384:512] *= 1e-37 if dtype == BF16 else 1e-7             # bf16: amax / 448 is subnormal -> scale 1.0, bytes 0
    rows = F.quantize_mla_latent_fp8(kv)
    assert rows.shape == (3, 5, 656) and rows.dtype == torch.uint8 and (f8.ROW, f8.SCALE_OFF, f8.ROPE_OFF) == (656, 512, 528)
    x = kv[..., :512].float().view(3, 5, 4, 128)
    s = x.abs().amax(-1) / 448.0                                      # the plain fp32 reference of the rule
    s = torch.where((s >= 2.0 ** -126) & (s < float("inf")), s, torch.ones_like(s))
    b = (x / s[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).view(3, 5, 512)
    assert torch.equal(rows[..., :512], b)
    assert torch.equal(rows[..., 512:528].contiguous().view(torch.float32), s)
    assert torch.equal(rows[..., 528:].contiguous().view(dtype), kv[..., 512:])
    assert s[0, 0, 1] == 1.0 and (rows[0, 0, 128:256] == 0).all() and (rows[0, 1, :4] == 0x80).all()
    assert s[1, 2, 2] == 900.0 / 448.0 and rows[1, 2, 300] == 0x7E and (s[1, 2, [0, 1, 3]] < 0.02).all()
    assert dtype == F16 or (s[2, 4, 3] == 1.0 and (rows[2, 4, 384:512] & 0x7F == 0).all())
    back = F.dequantize_mla_latent_fp8(rows, dtype)
    assert back.shape == (3, 5, 576) and back.dtype == torch.float32
    want = torch.cat([(b.view(torch.float8_e4m3fn).float().view(3, 5, 4, 128) * s[..., None]).view(3, 5, 512), kv[..., 512:].float()], -1)
    assert torch.equal(back, want)


# ---------------------------------------------------------------- surface
def test_python_binding_header_and_ctypes_signatures():
    import _mi355fa as fa
    import _mi355fa_mla_fp8_torch as ext
    import mla_kvcache
    M = f8.F()
    assert M.__all__ == ["quantize_mla_latent_fp8", "dequantize_mla_latent_fp8", "flash_attention_mla_kvcache_fp8", "MLA_FP8_ROW_BYTES"]
    sig = inspect.signature(M.flash_attention_mla_kvcache_fp8)
    assert sig == inspect.signature(mla_kvcache.flash_attention_mla_kvcache)
    assert [n for n in dir(ext) if not n.startswith("_")] == ["kvcache_mla_fp8_forward"]
    args = re.search(r"kvcache_mla_fp8_forward\((.*?)\) ->", ext.kvcache_mla_fp8_forward.__doc__, re.S).group(1)
    assert re.findall(r"(\w+): ", args) == ["q", "kv_cache", "cache_seqlens", "block_table", "kv_new", "is_causal", "softmax_scale", "out"]
    assert fa.lib.fa_abi_version() == 7
    assert os.listdir(os.path.join(ROOT, "include_mla_fp8")) == ["mi355fa_kvcache_mla_fp8.h"]
    txt, body, names = vck.header_functions(os.path.join(ROOT, "include_mla_fp8", "mi355fa_kvcache_mla_fp8.h"))
    assert names == ["fa_fwd_kvcache_mla_fp8", "fa_fwd_kvcache_mla_fp8_workspace_bytes"]
    for macro, v in (("ROW_BYTES", 656), ("SCALE_OFFSET", 512), ("ROPE_OFFSET", 528)):
        assert re.search(r"#define\s+MI355FA_MLA_FP8_%s\s+%d\b" % (macro, v), body)
    assert set(fa.KVCACHE_MLA_FP8_SIGNATURES) == set(names) and all(n in fa.ALL_SIGNATURES for n in names)
    for name in names:                                                          # the declared argument counts
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, body).group(1)
        assert len(decl.split(",")) == len(fa.KVCACHE_MLA_FP8_SIGNATURES[name][1]), name


# ---------------------------------------------------------------- the wrapper's and the binding's refusals
def test_every_malformed_call_is_refused_with_its_message():
    f = f8.F().flash_attention_mla_kvcache_fp8
    q = torch.randn(2, 4, 2, 576).to(BF16)
    kv = torch.zeros(6, 32, 656, dtype=torch.uint8)
    sl = torch.zeros(2, dtype=torch.int32).as_subclass(OnDevice)
    bt = torch.zeros(2, 3, dtype=torch.int32).as_subclass(OnDevice)

    def refused(msg, *a, **kw):
        with pytest.raises(AssertionError) as e:
            f(*a, **kw)
        assert str(e.value) == msg, str(e.value)
    refused("kv_cache must be torch.uint8 [num_pages, page_size, 656]: rows of 512 e4m3 bytes, 4 fp32 scales and 64 RoPE values "
            "in q's dtype (got torch.bfloat16)", q, torch.zeros(6, 32, 576, dtype=BF16), sl, bt)
    refused("kv_cache's last dim must be 656 bytes (got 576)", q, kv[..., :576], sl, bt)
    refused("kv_cache must be [num_pages, page_size, 656]: one latent head (got 4 dims)", q, kv[:, None], sl, bt)
    refused("q's last dim must be 576: 512 latent dims, then 64 RoPE dims (got 512)", q[..., :512], kv, sl, bt)
    refused("the page size (kv_cache.shape[1] = 48) must be a positive multiple of 32", q, torch.zeros(4, 48, 656, dtype=torch.uint8), sl, bt)
    refused("kv_new must be [B, S_q, 576]: one unquantised row per query row", q, kv, sl, bt, kv_new=torch.zeros(2, 2, 656, dtype=BF16))
    refused("flash_attention_mla_kvcache_fp8 has no backward: q must not require grad", q.float().requires_grad_(True), kv, sl, bt)
    # strides the kernels cannot address: rows a multiple of 16 bytes apart
    refused("kv_cache must be addressable in place: unit stride along the 656 bytes, a row stride that is a multiple of 16 bytes "
            "(got 664) and a page stride that is a multiple of 16 bytes", q, torch.zeros(6, 32, 664, dtype=torch.uint8)[..., :656], sl, bt)
    wide = torch.zeros(6, 32, 672, dtype=torch.uint8)[..., :656]               # 672: fine, the next refusal is reached
    refused("q, kv_cache, cache_seqlens and block_table must be device tensors", q, wide, sl, bt)


def _call(fa, p, **kw):
    a = dict(q=p, kv=p, new=None, sl=p, bt=p, o=p, lse=p, ws=p, wsb=1 << 30, B=2, H=16, Sq=1, pages=8, page=64, mp=4, bts=4, Snew=0,
             dtype=fa.BF16, scale=576 ** -0.5, causal=1, qs=None, ks=None, os=None)
    a.update(kw)
    return fa.lib.fa_fwd_kvcache_mla_fp8(a["q"], a["kv"], a["new"], a["sl"], a["bt"], a["o"], a["lse"], a["ws"], a["wsb"], a["B"],
                                         a["H"], a["Sq"], a["pages"], a["page"], a["mp"], a["bts"], a["Snew"], a["dtype"], a["scale"],
                                         a["causal"], a["qs"], a["ks"], a["os"], None)


def test_c_refusals_and_the_workspace_formula():
    import _mi355fa as fa
    buf, p = vck.aligned_ptr()
    st = lambda *v: (ctypes.c_longlong * len(v))(*v)
    fn = "fa_fwd_kvcache_mla_fp8: "
    cases = [
        (dict(kv=None), NULL, "kv_pool is NULL (argument 2)"),
        (dict(dtype=2), DTYPE, "dtype must be 0 (fp16) or 1 (bf16), the type of q, o, kv_new and the RoPE values (got 2)"),
        (dict(page=48), PAGED, "page_size must be a positive multiple of 32 (got 48)"),
        (dict(ks=st(41992, 656)), STRIDE, "the page stride of kv_pool must be a non-negative multiple of 16 bytes (got 41992)"),
        (dict(ks=st(41984, 664)), STRIDE, "the row stride of kv_pool must be a multiple of 16 bytes and at least 656 (got 664)"),
        (dict(ks=st(0, 1 << 26)), STRIDE, "one page of kv_pool exceeds 2^31 bytes (row stride 67108864 bytes)"),
        (dict(kv=p + 4), ALIGN, "kv_pool must be 16-byte aligned (ends in 4)"),
    ]
    for kw, code, text in cases:
        assert _call(fa, p, **kw) == code, (kw, fa.lib.fa_last_error())
        assert fa.lib.fa_last_error().decode() == fn + text, kw
    ws = fa.lib.fa_fwd_kvcache_mla_fp8_workspace_bytes
    vck.splits(3)
    need = ws(2, 16, 1, 4, 64, 0)
    assert need == 3 * 2 * 16 * 1 * 514 * 4
    assert _call(fa, p, wsb=need - 1) == WORKSPACE
    assert fa.lib.fa_last_error().decode() == fn + "workspace smaller than fa_fwd_kvcache_mla_fp8_workspace_bytes() (%d bytes)" % need
    assert ws(2, 16, 1, 4, 48, 0) == PAGED
    assert fa.lib.fa_last_error().decode() == "fa_fwd_kvcache_mla_fp8_workspace_bytes: page_size must be a positive multiple of 32 (got 48)"
    vck.splits(0)
    # the split rule is the 16-bit call's (mla_splits), and the forced count of the test hook is honoured
    for B, H, Sq, mp, page in [(1, 1, 1, 1, 32), (8, 128, 1, 256, 64), (8, 16, 1, 256, 64), (3, 24, 3, 11, 64), (600, 16, 1, 100, 32)]:
        n = splits_formula(B, H, Sq, mp * page)
        assert ws(B, H, Sq, mp, page, Sq) == (n * B * H * Sq * 514 * 4 if n > 1 else 0), (B, H, Sq, mp, page, n)
        assert ws(B, H, Sq, mp, page, 0) == fa.lib.fa_fwd_kvcache_mla_workspace_bytes(B, H, Sq, mp, page, 0)
        vck.splits(7)
        assert ws(B, H, Sq, mp, page, 0) == 7 * B * H * Sq * 514 * 4
        vck.splits(0)


# ---------------------------------------------------------------- the kernels
def test_new_kernels_are_in_the_library_inside_the_decode_budget():
    """<Fp8Row, T> overloads of fa_decode_paged_kernel, fa_kvcache_append_paged_kernel and fa_decode_combine_kernel over
    Fp8RowParams, two dtypes each: workgroup 256, VGPR + AGPR <= 256, no scratch, no spills, LDS within 80 KiB (the attention
    kernel's carve is dynamic: csrc/fa_decode_mla_fp8.hip static_asserts it)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj
    found = {}
    for k in codeobj.kernels():
        m = re.match(r"_ZN2fa\d+(fa_\w+?_kernel)INS_6Fp8RowENS_4(?:BF16|FP16)EEEvNS_12Fp8RowParamsE$", k["name"])
        assert m or "Fp8Row" not in k["name"], "an FP8 latent kernel outside the expected set: " + k["name"]
        if m:
            found[m.group(1)] = found.get(m.group(1), 0) + 1
            assert k["wg"] == 256 and k["vgpr"] + k["agpr"] <= 256, (k["name"], k["vgpr"], k["agpr"])
            assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] <= 81920, k["name"]
    assert found == {"fa_decode_paged_kernel": 2, "fa_kvcache_append_paged_kernel": 2, "fa_decode_combine_kernel": 2}, found
    src = open(os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd", "csrc", "fa_decode_mla_fp8.hip")).read()
    assert 'static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU")' in src


# ---------------------------------------------------------------- the reference-only condition of the GPU scale test
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_the_scaled_truth_of_the_gpu_test_is_far_from_the_all_ones_truth(dtype):
    lens = [65, 300]
    q, kv = mc.make(2, 16, 2, 320, dtype, seed=41, device="cpu")
    rows = f8.with_scales(kv, 42)
    s = rows[..., f8.SCALE_OFF:f8.ROPE_OFF].contiguous().view(torch.float32)
    assert s.min() >= 2.0 ** -6 and s.max() < 2.0 ** 6 and s.max() / s.min() > 1000 and (s[:, :, 0] != s[:, :, 1]).all()
    _, O, LSE, _ = f8.reference(q, rows, lens, True, 1 / 128)
    _, O1, _, _ = f8.reference(q, f8.ones(rows), lens, True, 1 / 128)
    far = fo.rel_fro(O1, O)
    assert far > mc.FAR, far
    assert torch.isfinite(O).all() and torch.isfinite(LSE).all() and O.shape == (2, 16, 2, 512)


# ---------------------------------------------------------------- the reference-only conditions of tests/test_gpu_mla_fp8_deep.py
DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])


@DTYPES
@pytest.mark.parametrize("w", range(4))
def test_column_problems_are_what_the_gpu_tests_take_them_for(w, dtype):
    """the helper's rows: zero bytes where the test says so under scales that are never all 1.0, a RoPE slice that moves LSE by
    more than 0.05, a V-side scale change that leaves the scores alone"""
    L = f8.COL_LENS
    q, rows = f8.column_problem("latent", w, dtype, "cpu")
    rest = torch.ones(512, dtype=torch.bool)
    rest[128 * w:128 * w + 128] = False
    s = f8.scales_of(rows)
    assert (rows[..., :512][..., rest] == 0).all() and (rows[..., :512][..., ~rest] != 0).any() and (rows[..., 528:] == 0).all()
    assert (s != 1.0).all() and s.min() >= 2.0 ** f8.COL_E[0] and s.max() < 2.0 ** (f8.COL_E[1] + 1) and (s[..., 0] != s[..., 1]).all()
    q, rows = f8.column_problem("rope", w, dtype, "cpu")
    assert (rows[..., :512] == 0).all() and (f8.scales_of(rows) != 1.0).all()
    _, O, LSE, _ = f8.reference(q, rows, L, True)
    _, _, flat, _ = f8.reference(torch.zeros_like(q), rows, L, True)
    assert (O == 0).all() and ((LSE - flat).abs() > 0.05).float().mean() > 0.9                 # the slice matters to LSE
    q, rows = f8.column_problem("zero", w, dtype, "cpu")
    assert (rows[..., 128 * w:128 * w + 128] == 0).all() and (f8.scales_of(rows)[..., w] == 2.0 ** 20).all()
    q, rows = f8.column_problem("vscale", w, dtype, "cpu")
    _, O, LSE, _ = f8.reference(q, rows, L, True)
    _, O2, LSE2, _ = f8.reference(q, f8.scaled_block(rows, w, 0.125), L, True)
    assert torch.equal(LSE, LSE2) and torch.equal(O[..., rest], O2[..., rest]) and torch.equal(O[..., ~rest] * 0.125, O2[..., ~rest])
    assert (O[..., ~rest] != 0).any()


def tile_share(q, kvd, scale, keep):
    """fp64 O [H, 512] of the one non-causal query of a ramp problem with the softmax of the whole row and the values of the
    keys outside `keep` (bool [L, 512]) zeroed"""
    P = torch.softmax(q[0, :, 0].double() @ kvd[0].t() * scale, dim=-1)
    return P @ (kvd[0, :, :512] * keep)


@DTYPES
@pytest.mark.parametrize("case", f8.RAMP_CASES)
def test_every_ramp_needs_its_scales_and_no_single_tile_carries_it(case, dtype):
    L = f8.RAMP_L
    q, rows = f8.ramp_problem(case, dtype, "cpu")
    s, e = f8.scales_of(rows)[0], f8.ramp_exponents(case)
    assert rows.shape == (1, 288, 656) and torch.equal(s, torch.exp2(e.float()).repeat_interleave(32, 0))
    assert case.endswith("-q") == bool((q[..., :512] != 0).any())
    kvd, O, LSE, level = f8.reference(q, rows, [L], False)
    _, O1, _, _ = f8.reference(q, f8.ones(rows), [L], False)
    assert fo.rel_fro(O1, O) > mc.FAR
    # the tile with the largest scale, per block (the first of them where several tie), alone under the row's softmax
    top = e.argmax(0)
    keep = (torch.arange(L)[:, None] // 32 == top[None, :]).repeat_interleave(128, 1)
    alone = tile_share(q, kvd[:, :L], mc.DEFAULT_SCALE, keep)
    assert fo.rel_fro(O[0, :, 0], tile_share(q, kvd[:, :L], mc.DEFAULT_SCALE, torch.ones_like(keep))) < 1e-12
    bound = mc.FP16_BOUND if dtype == F16 else max(2 * level[0], mc.BF16_FLOOR)
    assert fo.rel_fro(O[0, :, 0], alone) > 10 * bound, (fo.rel_fro(O[0, :, 0], alone), bound)
    assert f8.fits(O, dtype) and torch.isfinite(LSE).all()


@DTYPES
def test_a_spike_of_two_to_the_twelfth_would_carry_its_row_alone(dtype):
    """why the 'spike' ramp is flattened: with one tile at 2^6 among tiles at 2^-6 that tile alone is the truth to within the
    bound, and a wrong rescale of the other tiles could not show"""
    L = f8.RAMP_L
    q, rows = f8.ramp_problem("spike", dtype, "cpu")
    e = torch.full((9, 4), -6)
    e[4] = 6
    f8.set_scales(rows, torch.exp2(e.float()).repeat_interleave(32, 0)[None])
    kvd, O, _, _ = f8.reference(q, rows, [L], False)
    keep = (torch.arange(L)[:, None] // 32 == 4).expand(L, 512)
    assert fo.rel_fro(O[0, :, 0], tile_share(q, kvd[:, :L], mc.DEFAULT_SCALE, keep)) < 10 * mc.FP16_BOUND


@DTYPES
def test_the_scale_range_of_the_gpu_test_is_the_widest_that_fits_the_dtype(dtype):
    """e uniform in [-E, E]: at E the dequantised cache and the truth's O are finite and non-zero in the call's dtype; at E + 1
    the largest e4m3 value, 448, times 2^(E + 1) is not (fp16: 448 * 2^8 > 65504; bf16: 448 * 2^120 > 2^128)"""
    E = f8.RANGE_E[dtype]
    q, rows = f8.range_problem(dtype, E, "cpu")
    s = f8.scales_of(rows)
    assert s.min() == 2.0 ** -E and s.max() == 2.0 ** E and not (rows[..., :512] & 0x7F == 0x7F).any() and (rows[..., :512] == 0x7E).any()
    kvd, O, LSE, _ = f8.reference(q, rows, f8.RANGE_LENS, True)
    assert f8.fits(kvd[..., :512], dtype) and f8.fits(O, dtype) and (O != 0).all() and torch.isfinite(LSE).all()
    assert not f8.fits(torch.tensor([448.0 * 2.0 ** (E + 1)], dtype=torch.float64), dtype)
    q, rows = f8.range_problem(dtype, E + 1, "cpu")
    assert not f8.fits(f8.F().dequantize_mla_latent_fp8(rows, dtype, torch.float64)[..., :512], dtype)


@DTYPES
def test_the_deepseek_scale_of_the_gpu_test_is_far_from_the_default(dtype):
    lens = [33, 129, 300]
    q, kv = mc.make(len(lens), 16, 2, 320, dtype, seed=95, device="cpu")
    rows = f8.F().quantize_mla_latent_fp8(kv)
    _, O, LSE, _ = f8.reference(q, rows, lens, True, 192 ** -0.5)
    assert fo.rel_fro(f8.reference(q, rows, lens, True)[1], O) > mc.FAR
    assert torch.isfinite(O).all() and torch.isfinite(LSE).all()
