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


def with_scales(kv, seed, lo=-6, hi=5):
    """Rows whose four scale blocks differ by large factors per key: the latent values of kv as e4m3 bytes as they are, and a
    scale 2^e * (1 + f), e in [lo, hi] = [-6, 5], f in [0, 1), drawn per (key, block)."""
    rows = F().quantize_mla_latent_fp8(kv)
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(lo, hi + 1, (*kv.shape[:-1], 4), generator=g)
    s = (torch.exp2(e.float()) * (1 + torch.rand(e.shape, generator=g))).to(kv.device)
    rows[..., :SCALE_OFF] = kv[..., :mc.DV].float().to(torch.float8_e4m3fn).view(torch.uint8)
    rows[..., SCALE_OFF:ROPE_OFF] = s.contiguous().view(torch.uint8).reshape(*kv.shape[:-1], 16)
    return rows


def scales_of(rows):
    """the fp32 scales [..., 4] of rows (a copy)"""
    return rows[..., SCALE_OFF:ROPE_OFF].contiguous().view(torch.float32)


def set_scales(rows, s):
    """rows with the scales s (fp32, broadcast to [..., 4]) in place; returns rows"""
    s = s.to(torch.float32).to(rows.device).expand(*rows.shape[:-1], 4).contiguous()
    rows[..., SCALE_OFF:ROPE_OFF] = s.view(torch.uint8).reshape(*rows.shape[:-1], 16)
    return rows


# ---- tests/test_gpu_mla_fp8_deep.py: one column group at a time ------------------------------------------------------------
COL_LENS, COL_H, COL_SQ, COL_PAGE, COL_S = [65, 300], 16, 2, 64, 320
COL_E = (-3, 1)                    # the exponents of the column tests' scales: 2^-3 (1 + f) .. 2^1 (1 + f), never all 1.0


def column_rows(kv, seed):
    """with_scales at the column tests' exponents: the softmax of a default-scale problem stays broad, and the four blocks of
    a key still differ by factors up to 32"""
    return with_scales(kv, seed, *COL_E)


def column_problem(kind, w, dtype, device="cuda"):
    """(q, rows) of the column test `kind` at column group w (mlacheck.make's problem [2, 16, 2, 576] / [2, 320, 576]):
    'latent'  q (x 2) and the cache bytes are zero outside latent columns [128 w, + 128); every scale stays random
    'rope'    q (x 8) and the cache are zero outside RoPE columns [512 + 16 w, + 16): all 512 bytes 0x00, every scale random
    'zero'    the full problem with quarter w of the cache zeroed: bytes 0x00 under the scale 2^20
    'ropev'   the full problem with q zero on the RoPE columns
    'vscale'  the full problem with q zero on the latent columns: the scores come from the RoPE columns alone"""
    seed = {"latent": 140, "rope": 150, "zero": 160, "ropev": 170, "vscale": 180}[kind] + w
    q0, kv0 = mc.make(len(COL_LENS), COL_H, COL_SQ, COL_S, dtype, seed=seed, device=device)
    if kind in ("latent", "rope"):
        cols = slice(128 * w, 128 * w + 128) if kind == "latent" else slice(mc.DV + 16 * w, mc.DV + 16 * w + 16)
        q, kv = torch.zeros_like(q0), torch.zeros_like(kv0)
        q[..., cols], kv[..., cols] = q0[..., cols] * (2 if kind == "latent" else 8), kv0[..., cols]
        return q, column_rows(kv, seed + 1)
    rows = column_rows(kv0, seed + 1)
    if kind == "zero":
        rows[..., 128 * w:128 * w + 128] = 0
        s = scales_of(rows)
        s[..., w] = 2.0 ** 20
        set_scales(rows, s)
    elif kind == "ropev":
        q0[..., mc.DV:] = 0
    elif kind == "vscale":
        q0[..., :mc.DV] = 0
    return q0, rows


def scaled_block(rows, w, factor):
    """a copy of rows with the scales of block w times factor in every key"""
    s = scales_of(rows)
    s[..., w] *= factor
    return set_scales(rows.clone(), s)


# ---- tests/test_gpu_mla_fp8_deep.py: scale ramps over the tiles, and the scale range ------------------------------------------
RAMP_TILES, RAMP_L, RAMP_H = 9, 8 * 32 + 5, 16                       # eight full tiles and one of five keys
RAMPS = {                                                            # log2 of the scale of tile t = 0 .. 8
    "ascending": [2 * (t - 4) for t in range(9)],                    # x 4 per tile: 2^-8 .. 2^8
    "descending": [2 * (4 - t) for t in range(9)],
    "sawtooth": [2 if t & 1 else -2 for t in range(9)],              # x 16 up, / 16 down
    "spike": [6 - 2 * abs(t - 4) for t in range(9)],                 # 2^6 in the middle; see ramp_problem
}
RAMP_CASES = ["ascending", "descending", "sawtooth", "spike", "mixed0", "mixed1", "ascending-q", "descending-q"]
Q_LATENT = 2.0 ** -8               # the -q cases: q's latent columns times this, so that the scores stay of order 1


def ramp_exponents(case):
    """int [9 tiles, 4 blocks]: 'mixedk' puts block j on ramp (j + k) mod 4"""
    names = list(RAMPS)
    if case.startswith("mixed"):
        k = int(case[5:])
        return torch.tensor([RAMPS[names[(j + k) % 4]] for j in range(4)]).t().contiguous()
    return torch.tensor(RAMPS[case.split("-")[0]])[:, None].expand(9, 4).contiguous()


def ramp_problem(case, dtype, device="cuda"):
    """(q [1, 16, 1, 576], rows [1, 288, 656]) of one ramp: block scales constant within a 32-key tile.  q is zero on the latent
    columns -- the scores are independent of the scales and the softmax stays broad -- but in the '-q' cases.
    'spike': one tile at 2^6 in the middle of tiles at 2^-6 leaves that tile carrying the result alone (the rest of the row
    weighs 2^-12: tests/test_host_mla_fp8.py has the figure), so it is flattened to x 2 per tile on either side of the 2^6."""
    q, kv = mc.make(1, RAMP_H, 1, RAMP_TILES * 32, dtype, seed=200 + RAMP_CASES.index(case), device=device)
    if case.endswith("-q"):
        q[..., :mc.DV] = (q[..., :mc.DV].float() * Q_LATENT).to(dtype)
    else:
        q[..., :mc.DV] = 0
    rows = F().quantize_mla_latent_fp8(kv)
    rows[..., :SCALE_OFF] = kv[..., :mc.DV].float().to(torch.float8_e4m3fn).view(torch.uint8)
    s = torch.exp2(ramp_exponents(case).float()).repeat_interleave(32, 0)[None]
    return q, set_scales(rows, s)


RANGE_LENS, RANGE_SQ = [33, 300], 2
RANGE_E = {mc.F16: 7, mc.BF16: 119}          # tests/test_host_mla_fp8.py: the widest e for which cache and truth fit the dtype


def range_problem(dtype, E, device="cuda"):
    """(q [2, 16, 2, 576] zero on the latent columns, rows [2, 320, 656]): uniformly random e4m3 bytes (the two NaN codes
    replaced by +-448) under scales 2^e, e uniform in [-E, E] per (key, block)"""
    q, kv = mc.make(len(RANGE_LENS), 16, RANGE_SQ, COL_S, dtype, seed=230, device=device)
    q[..., :mc.DV] = 0
    rows = F().quantize_mla_latent_fp8(kv)
    g = torch.Generator().manual_seed(231)
    b = torch.randint(0, 256, (*kv.shape[:-1], mc.DV), generator=g, dtype=torch.uint8)
    b = torch.where(b & 0x7F == 0x7F, b - 1, b)
    e = torch.randint(-E, E + 1, (*kv.shape[:-1], 4), generator=g)
    rows[..., :SCALE_OFF] = b.to(device)
    return q, set_scales(rows, torch.exp2(e.double()).float())


def fits(x, dtype):
    """every value of the fp64 tensor x is finite and, where x is non-zero, non-zero in dtype"""
    y = x.to(dtype)
    return bool(torch.isfinite(y.float()).all() and ((y != 0) | (x == 0)).all())


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
