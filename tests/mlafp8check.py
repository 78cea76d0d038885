"""The byte pool of the FP8 MLA decode tests (tests/test_gpu_mla_fp8.py, tests/test_gpu_race_mla_fp8.py,
tests/test_host_mla_fp8.py; not a test module).  Everything else -- the problem, the table, the fp64 truth, the bounds -- is
tests/mlacheck.py's, applied to the DEQUANTISED cache (mla_fp8_kvcache.dequantize_mla_latent_fp8 in fp64): quantisation error
is no part of any bound."""
import torch

import mlacheck as mc

ROW, SCALE_OFF, ROPE_OFF = 656, 512, 528


def F():
    import mla_fp8_kvcache
    return mla_fp8_kvcache


def poison_rows(shape, row_stride, dtype, device):
    """uint8 [*shape, row_stride] of rows nothing may read: latent bytes 0x7F (e4m3 NaN), NaN scales, NaN RoPE values, 0xFF padding"""
    row = torch.full((row_stride,), 0xFF, dtype=torch.uint8)
    row[:SCALE_OFF] = 0x7F
    row[SCALE_OFF:ROPE_OFF] = torch.full((4,), float("nan")).view(torch.uint8)
    row[ROPE_OFF:ROW] = torch.full((64,), float("nan"), dtype=dtype).view(torch.uint8)
    return row.to(device).repeat(*shape, 1)


def scatter(rows, dtype, lens, page, max_pages, seed, alloc=None, row_stride=ROW):
    """mlacheck.scatter for quantised rows [B, S, 656]: the pool [num_pages, page, 656] (rows row_stride bytes apart) under
    mlacheck's permuted table with out-of-range entries past each sequence's pages; every row at or past lens[b], every unused
    page and the padding between rows are poison_rows."""
    B, S, _ = rows.shape
    _, table = mc.scatter(torch.zeros(B, S, mc.D, dtype=dtype), lens, page, max_pages, seed, alloc=alloc)
    num_pages = sum(mc.pages_of(L, page) for L in (alloc or lens)) + 3
    pool = poison_rows((num_pages, page), row_stride, dtype, rows.device)[..., :ROW]
    for b, L in enumerate(lens):
        for i in range(mc.pages_of(L, page)):
            n = min(page, L - i * page)
            pool[int(table[b, i]), :n] = rows[b, i * page:i * page + n]
    return pool, table.to(rows.device)


def with_scales(kv, seed):
    """Rows whose four scale blocks differ by large factors per key: the latent values of kv as e4m3 bytes as they are, and a
    scale 2^e * (1 + f), e in [-6, 5], f in [0, 1), drawn per (key, block)."""
    rows = F().quantize_mla_latent_fp8(kv)
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-6, 6, (*kv.shape[:-1], 4), generator=g)
    s = (torch.exp2(e.float()) * (1 + torch.rand(e.shape, generator=g))).to(kv.device)
    rows[..., :SCALE_OFF] = kv[..., :mc.DV].float().to(torch.float8_e4m3fn).view(torch.uint8)
    rows[..., SCALE_OFF:ROPE_OFF] = s.contiguous().view(torch.uint8).reshape(*kv.shape[:-1], 16)
    return rows


def ones(rows):
    """the same rows with every scale 1.0"""
    r = rows.clone()
    r[..., SCALE_OFF:ROPE_OFF] = torch.ones(4).view(torch.uint8).to(rows.device)
    return r


def reference(q, rows, lens, causal, scale=None):
    """(the dequantised cache in fp64, O, LSE, PyTorch's SDPA level for bf16 or None) of the problem (q, rows)"""
    kvd = F().dequantize_mla_latent_fp8(rows, q.dtype, torch.float64)
    O, LSE = mc.truth(q, kvd, lens, causal, scale)
    level = mc.sdpa_level(q, kvd.to(q.dtype), lens, causal, scale, O) if q.dtype == mc.BF16 else None
    return kvd, O, LSE, level
