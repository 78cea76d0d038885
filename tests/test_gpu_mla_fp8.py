"""MLA decoding over a paged FP8 latent cache (mla_fp8_kvcache.flash_attention_mla_kvcache_fp8) against the fp64 truth of
tests/mlacheck.py on the DEQUANTISED cache, with the project's bounds (mlacheck.held: fp16 relFro < 1e-3, bf16 < max(2 x PyTorch
bf16 SDPA, 4e-3), LSE rtol 1e-3 / atol 2e-3, -inf exact).  Every pool is poisoned outside its live rows (tests/mlafp8check.py):
a read at or past L, of an unused page or of the row padding shows as NaN."""
import pytest
import torch

import mlacheck as mc
import mlafp8check as f8
import variantcheck as vck
from mlacheck import BF16, DT, IDS

pytestmark = pytest.mark.gpu

LENS = [0, 1, 31, 32, 33, 65, 129, 300]
S = 320


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def call(q, pool, lens, table, n=0, **kw):
    vck.splits(n)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    return f8.F().flash_attention_mla_kvcache_fp8(q, pool, sl, table, return_lse=True, **kw)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("Sq", [1, 3])
@pytest.mark.parametrize("H", [1, 16, 24])
def test_parity_over_fill_levels_pages_and_splits(H, Sq, dtype, causal):
    q, kv = mc.make(len(LENS), H, Sq, S, dtype, seed=H + Sq)
    rows = f8.F().quantize_mla_latent_fp8(kv)
    _, O, LSE, level = f8.reference(q, rows, LENS, causal)
    for page in (32, 64):
        pool, table = f8.scatter(rows, dtype, LENS, page, S // page, seed=page)
        for n in (0, 1, 3):
            tag = "fp8-parity/H%d/Sq%d/%s/page%d/n%d" % (H, Sq, "causal" if causal else "full", page, n)
            got = call(q, pool, LENS, table, n, is_causal=causal)
            mc.held(tag, q, got[0], got[1], O, LSE, LENS, level)
            assert mc.same(got, call(q, pool, LENS, table, n, is_causal=causal)), (tag, "a repeated call gives other bits")


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_scales_are_applied_per_quarter_to_k_and_v(dtype, n):
    """scales 2^-6 .. 2^5 with random mantissas per (key, 128-dim block): a swapped, dropped or key-misaligned scale is far off
    (tests/test_host_mla_fp8.py shows on the CPU how far the all-ones truth lies)"""
    lens = [65, 300]
    q, kv = mc.make(2, 16, 2, S, dtype, seed=41)
    rows = f8.with_scales(kv, 42)
    _, O, LSE, level = f8.reference(q, rows, lens, True, 1 / 128)
    pool, table = f8.scatter(rows, dtype, lens, 64, 5, seed=3)
    o, lse = call(q, pool, lens, table, n, is_causal=True, softmax_scale=1 / 128)
    mc.held("fp8-scales/n%d" % n, q, o, lse, O, LSE, lens, level)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_append_quantises_bit_exactly_and_only_its_rows(dtype):
    """kv_new across page boundaries, an all-zero block (scale 1.0), a block with one large outlier, -0.0, and a sequence whose
    last row falls past the table (dropped): afterwards the pool is the pool of the quantised full cache, byte for byte."""
    F, page, new = f8.F(), 32, 3
    fills = [30, 31, 63, 0, 318]                                    # 318 + 3 rows: the third is past the 320-row table
    Ls = [min(x + new, S) for x in fills]
    q, kv = mc.make(len(fills), 16, new, S, dtype, seed=7)
    kv_new = torch.randn(len(fills), new, mc.D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8)).to(dtype)
    kv_new[0, 0, 128:256] = 0
    kv_new[1, 1, 300] = 900.0
    kv_new[2, 2, :8] = -0.0
    kv_new[3, 0] *= 1e-3
    full = kv.clone()
    for b, x in enumerate(fills):
        full[b, x:Ls[b]] = kv_new[b, :Ls[b] - x]
    quant = lambda x: F.quantize_mla_latent_fp8(x.cpu()).cuda()     # on the CPU: the correctly rounded amax / 448
    rows, rows_full = quant(kv), quant(full)
    for b, x in enumerate(fills):                                   # the helper on kv_new itself: what the append must write
        assert torch.equal(rows_full[b, x:Ls[b]], quant(kv_new[b, :Ls[b] - x]))
    assert rows_full[0, 30, f8.SCALE_OFF + 4:f8.SCALE_OFF + 8].view(torch.float32).item() == 1.0
    pool, table = f8.scatter(rows, dtype, fills, page, S // page, seed=5, alloc=Ls)
    expect, _ = f8.scatter(rows_full, dtype, Ls, page, S // page, seed=5)
    _, O, LSE, level = f8.reference(q, rows_full, Ls, True)
    for n in (1, 3):
        mine = pool.clone()
        o, lse = call(q, mine, fills, table, n, kv_new=kv_new, is_causal=True)
        assert torch.equal(mine, expect), ("bytes differ at", (mine != expect).nonzero()[:4].tolist())
        mc.held("fp8-append/n%d" % n, q, o, lse, O, LSE, Ls, level)


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_layouts_give_the_bits_of_the_contiguous_call(dtype):
    lens = [33, 129, 300]
    q, kv = mc.make(len(lens), 24, 3, S, dtype, seed=11)
    rows = f8.F().quantize_mla_latent_fp8(kv)
    pool, table = f8.scatter(rows, dtype, lens, 64, 5, seed=2)
    wide, table_w = f8.scatter(rows, dtype, lens, 64, 5, seed=2, row_stride=672)
    assert torch.equal(table, table_w) and wide.stride(1) == 672
    for n in (1, 3):
        want = call(q, pool, lens, table, n, is_causal=True)
        qt = q.transpose(1, 2).contiguous().transpose(1, 2)          # a [B, S_q, H, 576] tensor seen as [B, H, S_q, 576]
        out = torch.empty(len(lens), 3, 24, 640, dtype=dtype, device="cuda")[..., :512].transpose(1, 2)
        got = call(qt, wide, lens, table, n, is_causal=True, out=out)
        assert got[0].data_ptr() == out.data_ptr() and not qt.is_contiguous()
        assert mc.same(want, got)
