"""CPU tests of the paged-KV-cache decoding boundary: include/mi355fa_paged.h declares exactly two entry points, the
mi355fa_paged_mods struct and MI355FA_ERR_PAGED (-12); libmi355fa.so and the ctypes tables export them (a table of their
own, PAGED_SIGNATURES, as every companion header has: SIGNATURES is the table tests/test_host_scale.py enumerates); the ABI
version and mi355fa_kvcache.h are untouched; every new refusal is reported before anything is launched; the workspace is
the padded call's at S_cache = max_pages_per_seq * page_size; the Python function refuses what it must; and the tests' own
scatter / gather helpers (tests/pagedcheck.py) agree with a hand-written loop, their strided-table and guarded-pool forms
gather the same bytes, and the shapes of tests/test_gpu_paged_deep.py reach what that module is there for: a CPU model of the
decode body's tile and split arithmetic over its constants; and the two Python functions and the two binding functions
refuse every malformed call of tests/paged_surface.py's CPU table at the check, with the exception type and the exact
message of tests/golden/paged_errors.json, recorded before the two bindings became one module.  No compute is launched here
(no GPU)."""
import ctypes
import functools
import json
import os
import re

import pytest
import torch

from conftest import ROOT
import paged_surface as ps
import pagedcheck as pc
import variantcheck as vck

HDR = os.path.join(ROOT, "include", "mi355fa_paged.h")
NAMES = ["fa_fwd_kvcache_paged", "fa_fwd_kvcache_paged_workspace_bytes"]


def _lib():
    import _mi355fa as fa
    return fa


def test_header_declares_the_paged_entry_points():
    txt, body, functions = vck.header_functions(HDR)
    assert functions == NAMES
    assert re.search(r"#define\s+MI355FA_ERR_PAGED\s+\(-12\)", body)
    m = re.search(r"typedef struct mi355fa_paged_mods \{(.*?)\} mi355fa_paged_mods;", body, flags=re.S)
    assert m, "the mods struct"
    members = re.findall(r"(\w+);", m.group(1))
    assert members == ["softcap", "alibi_slopes", "slopes_batch_stride", "sinks", "k_descale", "v_descale", "descale_bstride"]
    assert "fa_debug" not in txt
    # the older headers are as they were: ABI 7, and the padded header still declares exactly its two functions
    assert vck.header_functions(os.path.join(ROOT, "include", "mi355fa_kvcache.h"))[2] == \
        ["fa_fwd_kvcache", "fa_fwd_kvcache_workspace_bytes"]
    assert re.search(r"#define\s+MI355FA_ABI_VERSION\s+7\b", open(os.path.join(ROOT, "include", "mi355fa.h")).read())
    for older in ("mi355fa.h", "mi355fa_kvcache.h", "mi355fa_kvcache_fp8.h", "mi355fa_sink.h"):
        assert "paged" not in open(os.path.join(ROOT, "include", older)).read().lower(), older


def test_library_and_ctypes_export_the_paged_entry_points():
    fa = _lib()
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in fa.PAGED_SIGNATURES and name in fa.ALL_SIGNATURES, name
        assert name not in fa.SIGNATURES, name
    assert len(fa.PAGED_SIGNATURES["fa_fwd_kvcache_paged"][1]) == 29
    assert len(fa.PAGED_SIGNATURES["fa_fwd_kvcache_paged_workspace_bytes"][1]) == 9
    assert fa.ERR_PAGED == -12 and (fa.PAGED_CACHE_16BIT, fa.PAGED_CACHE_FP8_E4M3) == (0, 1)
    # the struct as the C compiler lays it out on this ABI: float, 4 bytes of padding, then 8-byte members
    assert ctypes.sizeof(fa.PagedMods) == 56 and fa.PagedMods.alibi_slopes.offset == 8 and fa.PagedMods.descale_bstride.offset == 48
    assert fa.lib.fa_abi_version() == 7 and fa.ABI_VERSION == 7


def _call(fa, p, **over):
    """One otherwise well-formed paged call (B 2, H 8, H_kv 2, S_q 1, 6 pages of 64 keys per sequence, D 64, bf16, every
    pointer p) with the arguments of `over` replaced; mods: a dict of mi355fa_paged_mods members."""
    a = dict(q=p, kp=p, vp=p, kn=None, vn=None, sl=p, bt=p, o=p, ws=p, wsb=1 << 20, B=2, H=8, Hkv=2, Sq=1, NP=100, page=64,
             MP=6, bts=6, Sn=0, D=64, dt=fa.BF16, cdt=fa.PAGED_CACHE_16BIT, scale=0.125, wl=-1, wr=-1, mods=None, opts=None)
    a.update(over)
    mods = None
    if a["mods"] is not None:
        mods = ctypes.byref(fa.PagedMods(**a["mods"]))
    return fa.lib.fa_fwd_kvcache_paged(a["q"], a["kp"], a["vp"], a["kn"], a["vn"], a["sl"], a["bt"], a["o"], None, a["ws"],
                                       a["wsb"], a["B"], a["H"], a["Hkv"], a["Sq"], a["NP"], a["page"], a["MP"], a["bts"],
                                       a["Sn"], a["D"], a["dt"], a["cdt"], a["scale"], a["wl"], a["wr"], mods, a["opts"], None)


def test_new_refusals_come_before_launch():
    fa = _lib()
    L = fa.lib
    _buf, p = vck.aligned_ptr()
    vck.splits(4)      # a split count that needs a workspace at any shape
    try:
        assert _call(fa, p, bt=None) == -1 and b"block_table" in L.fa_last_error()          # MI355FA_ERR_NULL
        for page in (16, 48, 0, -32, 33, 31):
            assert _call(fa, p, page=page) == fa.ERR_PAGED, page
            assert b"page_size" in L.fa_last_error()
        for kw in ({"NP": 0}, {"NP": -1}, {"MP": 0}, {"MP": -3}):
            assert _call(fa, p, **kw) == fa.ERR_PAGED, kw
        for bts in (5, 0, -6):
            assert _call(fa, p, bts=bts) == fa.ERR_PAGED, bts
            assert b"block_table_stride" in L.fa_last_error()
        for off in (1, 2, 3):
            assert _call(fa, p, bt=p + off) == -5, off                                       # MI355FA_ERR_ALIGN
            assert b"block_table" in L.fa_last_error()
        for mods in ({"k_descale": p}, {"v_descale": p}, {"descale_bstride": 2}):
            assert _call(fa, p, mods=mods) == fa.ERR_PAGED, mods
            assert b"fp8" in L.fa_last_error()
        assert _call(fa, p, cdt=2) == -4 and b"cache_dtype" in L.fa_last_error()             # MI355FA_ERR_DTYPE
        # the combinations the padded entry points do not offer
        for mods in ({"softcap": 30.0, "sinks": p}, {"softcap": 30.0, "alibi_slopes": p}, {"alibi_slopes": p, "sinks": p}):
            assert _call(fa, p, mods=mods) == fa.ERR_PAGED, mods
        for mods in ({"softcap": 30.0}, {"alibi_slopes": p}):
            assert _call(fa, p, cdt=fa.PAGED_CACHE_FP8_E4M3, mods=mods) == fa.ERR_PAGED, mods
        # each variant's own checks, with the padded entry points' codes
        for cap in (-1.0, float("nan"), float("inf"), -0.0):
            assert _call(fa, p, mods={"softcap": cap}) == fa.ERR_SOFTCAP, cap
        assert _call(fa, p, mods={"sinks": p + 2}) == -5
        assert _call(fa, p, mods={"alibi_slopes": p + 2}) == -5
        assert _call(fa, p, mods={"alibi_slopes": p, "slopes_batch_stride": 3}) == fa.ERR_ALIBI
        assert _call(fa, p, cdt=fa.PAGED_CACHE_FP8_E4M3, mods={"k_descale": p, "descale_bstride": 1}) == -2
        assert _call(fa, p, cdt=fa.PAGED_CACHE_FP8_E4M3, mods={"k_descale": p + 2}) == -5
        # and kvcache_impl's, unchanged
        for kw in ({"q": None}, {"kp": None}, {"vp": None}, {"sl": None}, {"o": None}, {"kn": p}, {"Sn": 3}):
            assert _call(fa, p, **kw) == -1, kw
        for kw in ({"B": 0}, {"Sq": 0}, {"scale": 0.0}, {"scale": float("nan")}, {"Sn": -1}):
            assert _call(fa, p, **kw) == -2, kw
        assert _call(fa, p, D=96) == -3 and _call(fa, p, dt=2) == -4
        assert _call(fa, p, Hkv=3) == fa.ERR_GROUP and _call(fa, p, wl=-2) == fa.ERR_WINDOW
        assert _call(fa, p, q=p + 8) == -5 and _call(fa, p, kp=p + 8) == -5
        need = L.fa_fwd_kvcache_paged_workspace_bytes(2, 8, 2, 1, 6, 64, 0, 64, fa.PAGED_CACHE_16BIT)
        assert need == 4 * 2 * 8 * 1 * (64 + 2) * 4
        assert _call(fa, p, wsb=need - 1) == fa.ERR_WORKSPACE and _call(fa, p, ws=None) == fa.ERR_WORKSPACE
        S3 = lambda *s: ctypes.cast((ctypes.c_longlong * 3)(*s), ctypes.POINTER(ctypes.c_longlong))
        keep = S3(64 * 2 * 64, 64, 2 * 64 + 4)                                               # a row stride off 16 bytes
        st = fa.Opts.make(k_strides=keep, v_strides=keep)
        assert _call(fa, p, opts=ctypes.byref(st)) == -6                                     # MI355FA_ERR_STRIDE
        # the workspace function refuses the same page geometry
        for page in (16, 48, 0):
            assert L.fa_fwd_kvcache_paged_workspace_bytes(2, 8, 2, 1, 6, page, 0, 64, 0) == fa.ERR_PAGED
        assert L.fa_fwd_kvcache_paged_workspace_bytes(2, 8, 2, 1, 0, 64, 0, 64, 0) == fa.ERR_PAGED
        assert L.fa_fwd_kvcache_paged_workspace_bytes(2, 8, 2, 1, 6, 64, 0, 64, 2) == -4
    finally:
        vck.splits(0)


def test_workspace_is_the_padded_one_at_the_tables_reach():
    fa = _lib()
    L = fa.lib
    shapes = ((1, 32, 8, 1, 128, 32, 128), (8, 32, 8, 1, 128, 128, 128), (8, 32, 8, 1, 64, 256, 64), (3, 4, 4, 130, 7, 96, 64),
              (2, 8, 1, 3, 1, 32, 128), (1, 8, 2, 1, 4096, 32, 64))
    try:
        for n in (0, 1, 2, 7, 64):
            vck.splits(n)
            for (B, H, Hkv, Sq, MP, page, D) in shapes:
                for Sn in (0, 5):
                    padded = L.fa_fwd_kvcache_workspace_bytes(B, H, Hkv, Sq, MP * page, Sn, D)
                    padded8 = L.fa_fwd_kvcache_fp8_workspace_bytes(B, H, Hkv, Sq, MP * page, Sn, D)
                    assert L.fa_fwd_kvcache_paged_workspace_bytes(B, H, Hkv, Sq, MP, page, Sn, D, fa.PAGED_CACHE_16BIT) == padded
                    assert L.fa_fwd_kvcache_paged_workspace_bytes(B, H, Hkv, Sq, MP, page, Sn, D, fa.PAGED_CACHE_FP8_E4M3) == padded8
                    if n > 1:
                        assert padded == padded8 == n * B * H * Sq * (D + 2) * 4
        vck.splits(0)
        # the two cache formats really follow different rules somewhere in the table above
        assert any(L.fa_fwd_kvcache_workspace_bytes(B, H, Hkv, Sq, MP * page, 0, D) !=
                   L.fa_fwd_kvcache_fp8_workspace_bytes(B, H, Hkv, Sq, MP * page, 0, D) for (B, H, Hkv, Sq, MP, page, D) in shapes)
    finally:
        vck.splits(0)


def _args(page=64, dtype=torch.bfloat16, cache_dtype=None):
    B, H, Hkv, D, NP, MP = 2, 4, 2, 64, 8, 3
    q = torch.zeros(B, H, 1, D, dtype=dtype)
    kc = torch.zeros(NP, Hkv, page, D, dtype=cache_dtype or dtype)
    return dict(q=q, k_cache=kc, v_cache=kc.clone(), cache_seqlens=torch.zeros(B, dtype=torch.int32),
                block_table=torch.zeros(B, MP, dtype=torch.int32))


def test_python_wrapper_refuses_what_it_must():
    """Every refusal below is reached on the CPU: the wrapper checks the table's dtype and rank, the page size, the
    combinations and the gradients before the first device check, which is the table's own."""
    import paged_kvcache as P
    f = P.flash_attention_kvcache_paged
    one = torch.ones(4)

    def refused(what, **over):
        kw = _args(**{k: over.pop(k) for k in ("page", "cache_dtype") if k in over})
        kw.update(over)
        with pytest.raises(AssertionError, match=what):
            f(**kw)

    a = _args()
    refused("block_table must be int32", block_table=a["block_table"].to(torch.int64))
    refused("block_table must be a device tensor")               # everything else in order: the host table is what is left
    refused("block_table must be \\[B, max_pages_per_seq\\]", block_table=torch.zeros(6, dtype=torch.int32))
    refused("multiple of 32", page=16)
    refused("multiple of 32", page=48)
    refused("at most one of softcap, alibi_slopes and sinks", softcap=30.0, sinks=one)
    refused("at most one of softcap, alibi_slopes and sinks", softcap=30.0, alibi_slopes=one)
    refused("at most one of softcap, alibi_slopes and sinks", alibi_slopes=one, sinks=one)
    refused("an fp8 cache takes sinks only: softcap", cache_dtype=torch.float8_e4m3fn, softcap=30.0)
    refused("an fp8 cache takes sinks only: alibi_slopes", cache_dtype=torch.float8_e4m3fn, alibi_slopes=one)
    refused("k_descale / v_descale belong to a torch.float8_e4m3fn cache", k_descale=torch.ones(2))
    refused("k_descale / v_descale belong to a torch.float8_e4m3fn cache", v_descale=torch.ones(2))
    refused("softcap must be finite and > 0", softcap=0.0)
    refused("softcap must be finite and > 0", softcap=float("nan"))
    refused("softmax_scale must be finite and > 0", softmax_scale=-1.0)
    refused("is_causal=True with window_right > 0", is_causal=True, window_size=(-1, 3))
    refused("k_new and v_new must be given together", k_new=torch.zeros(2, 2, 1, 64, dtype=torch.bfloat16))
    refused("has no backward: q must not require grad", q=a["q"].clone().requires_grad_(True))
    refused("has no backward: k_cache must not require grad", k_cache=a["k_cache"].clone().requires_grad_(True))
    kn = torch.zeros(2, 2, 1, 64, dtype=torch.bfloat16)
    refused("has no backward: k_new must not require grad", k_new=kn.clone().requires_grad_(True), v_new=kn)
    refused("has no backward: sinks must not require grad", sinks=one.clone().requires_grad_(True))
    # the public surface of the module is the one function
    assert P.__all__ == ["flash_attention_kvcache_paged"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float8_e4m3fn], ids=["bf16", "fp16", "e4m3"])
def test_scatter_and_gather_agree_with_a_hand_written_loop(dtype):
    B, Hkv, D, page, NP, MP = 4, 2, 8, 32, 12, 3
    lens = [0, 1, 33, 96]
    g = torch.Generator().manual_seed(3)
    cache = torch.randn(B, Hkv, MP * page, D, generator=g).clamp(-4, 4).to(dtype)
    (pool,), table = pc.scatter([cache], lens, page, NP, MP, seed=1)
    assert pool.shape == (NP, Hkv, page, D) and table.shape == (B, MP) and table.dtype == torch.int32
    assert int(table.min()) >= 0 and int(table.max()) < NP              # never an out-of-range entry
    used = [int(table[b, i]) for b in range(B) for i in range(pc.pages_of(lens[b], page))]
    assert len(set(used)) == len(used) == 0 + 1 + 2 + 3
    isnan = lambda t: torch.isnan(t.float())
    for n in range(NP):
        if n not in used:
            assert isnan(pool[n]).all(), n                               # an unused page is NaN throughout
    for b in range(B):
        for i in range(pc.pages_of(lens[b], page), MP):
            assert int(table[b, i]) not in used                          # an unused entry names a NaN page
    # key j of sequence b is row j % page of page table[b][j // page]; rows past L_b in the last page are NaN
    for b, L in enumerate(lens):
        for j in range(MP * page):
            row = pool[int(table[b, j // page]), :, j % page]
            if j < L:
                assert pc.same_bytes(row, cache[b, :, j]), (b, j)
            else:
                assert isnan(row).all(), (b, j)
    back = pc.gather(pool, table)
    zeroed = pc.gather(pool, table, lens)
    assert back.shape == cache.shape and back.dtype == dtype
    for b, L in enumerate(lens):
        assert pc.same_bytes(back[b, :, :L], cache[b, :, :L]) and isnan(back[b, :, L:]).all()
        assert pc.same_bytes(zeroed[b, :, :L], cache[b, :, :L]) and (zeroed[b, :, L:].float() == 0).all()
    # a table given by the caller: two sequences sharing their first page
    shared = torch.tensor([[5, 7, 0], [5, 9, 0]], dtype=torch.int32)
    two = cache[2:4].clone()
    two[1, :, :page] = two[0, :, :page]
    (pool2,), t2 = pc.scatter([two], [40, 64], page, NP, MP, seed=0, table=shared)
    assert torch.equal(t2, shared)
    assert pc.same_bytes(pc.gather(pool2, t2, [40, 64])[:, :, :40], two[:, :, :40])
    assert isnan(pool2[0]).all() and isnan(pool2[7][:, 8:]).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float8_e4m3fn], ids=["bf16", "e4m3"])
def test_wide_table_and_guarded_pool_gather_the_same_bytes(dtype):
    B, Hkv, D, page, NP, MP, G = 4, 2, 8, 32, 14, 5, 4
    lens = [0, 1, 33, 160]
    g = torch.Generator().manual_seed(5)
    cache = torch.randn(B, Hkv, MP * page, D, generator=g).clamp(-4, 4).to(dtype)
    (pool,), table = pc.scatter([cache], lens, page, NP, MP, seed=2)
    plain = pc.gather(pool, table)
    isnan = lambda t: torch.isnan(t.float())
    # the pages no sequence names: NaN throughout, and the complement of the used ones
    spare = pc.unused_pages(table, lens, page, NP)
    used = {int(table[b, i]) for b in range(B) for i in range(pc.pages_of(lens[b], page))}
    assert sorted(used | set(spare)) == list(range(NP)) and not used & set(spare) and len(spare) == NP - 8
    assert all(isnan(pool[n]).all() for n in spare)
    # the table as columns [3, 3 + MP) of a [B, MP + 7] tensor whose other columns name those pages
    wide = pc.wide_table(table, spare)
    assert wide.shape == (B, MP) and wide.dtype == torch.int32 and wide.stride() == (MP + 7, 1) and not wide.is_contiguous()
    assert wide.storage_offset() == 3 and wide.data_ptr() % 4 == 0 and (wide.data_ptr() - 12) % 16 == 0
    whole = torch.as_strided(wide, (B, MP + 7), (MP + 7, 1), 0)
    assert torch.equal(whole[:, 3:3 + MP], table)
    outside = torch.cat([whole[:, :3], whole[:, 3 + MP:]], dim=1)
    assert set(outside.flatten().tolist()) <= set(spare) and outside.shape == (B, 7)
    assert torch.equal(wide, table) and pc.same_bytes(pc.gather(pool, wide), plain)
    assert pc.same_bytes(pc.gather(pool, wide, lens), pc.gather(pool, table, lens))
    # the pool as pages [G, G + NP) of a NaN-filled allocation of NP + 2 G pages
    big, view = pc.guarded(pool, G)
    assert big.shape == (NP + 2 * G, Hkv, page, D) and view.shape == pool.shape and view.dtype == dtype and view.is_contiguous()
    assert view.data_ptr() == big[G].data_ptr() and pc.same_bytes(view, pool)
    assert isnan(big[:G]).all() and isnan(big[G + NP:]).all() and pc.guards_intact(big, G)
    assert pc.same_bytes(pc.gather(view, table), plain) and pc.same_bytes(pc.gather(view, wide), plain)
    # the entries the deep tests plant (-1, -G, NP, NP + G - 1) name guard pages of `big`, never anything outside it
    for e in (-1, -G, NP, NP + G - 1):
        assert 0 <= e + G < big.shape[0] and not 0 <= e < NP and isnan(big[e + G]).all()
    # a changed guard byte is seen, on either side
    for n in (0, G - 1, G + NP, NP + 2 * G - 1):
        pc._bytes(big)[n, 1, 3, 2] = 0
        assert not pc.guards_intact(big, G), n
        pc.fill_nan(big[n])
        assert pc.guards_intact(big, G)
    assert pc.same_bytes(view, pool)


def _work_items(L, Sq, g, wl, wr, n, ng=4):
    """fa_decode_body.inc's arithmetic for one (sequence, K/V head): (tb, s_beg, [loop steps of wave 0..3]) per (row block,
    split) at n splits.  wl / wr < 0: unbounded.  ng: the tiles a workgroup takes per loop step, 4 but 2 at D = 256, where
    the two waves of a pair share a tile and every pair's steps are counted from s_beg, as the body counts them."""
    M = g * Sq
    big = 1 << 30
    wl, wr = (big if wl < 0 else wl), (big if wr < 0 else wr)
    for rb in range(-(-M // 32)):
        r0, rlast = rb * 32, min(M, rb * 32 + 32) - 1
        pos0, pos1 = L - Sq + r0 // g, L - Sq + rlast // g
        lo, hi = max(0, pos0 - wl), min(L, pos1 + wr + 1)
        tb = lo // 32
        te = -(-hi // 32) if hi > lo else tb
        nt = te - tb
        for split in range(n):
            s_beg, s_end = tb + nt * split // n, tb + nt * (split + 1) // n
            yield tb, s_beg, [len(range(s_beg + (w if ng == 4 else 0), s_end, ng)) for w in range(ng)]


def deep_reach(geoms, lengths, groups, sqs, masks, splits, ng=4):
    """per (page, max_pages): the longest wave over all cases, the longest wave at 3 splits, whether a split with a wave of
    >= 4 steps begins mid-page, and whether some case's first tile lies in the last third of the table"""
    import test_gpu_kvcache as tk
    out = {}
    for page, mp in geoms:
        tpp, tiles = page // 32, page * mp // 32
        longest = longest3 = 0
        midpage = last_third = False
        for L in lengths(page, mp):
            for H, Hkv in groups:
                for Sq in sqs:
                    for is_causal, window in masks:
                        wl, wr = tk.window_of(is_causal, window)
                        for n in splits:
                            for tb, s_beg, steps in _work_items(L, Sq, H // Hkv, wl, wr, n, ng):
                                longest = max(longest, max(steps))
                                if n == 3:
                                    longest3 = max(longest3, max(steps))
                                midpage |= max(steps) >= 4 and s_beg % tpp != 0
                                last_third |= max(steps) >= 1 and 3 * tb >= 2 * tiles
        out[(page, mp)] = (longest, longest3, midpage, last_third)
    return out


def packed_reach(page, mp, S, lens, ng, groups, masks, splits):
    """deep_reach's four figures for one packed step: sequence b has S[b] queries over lens[b] keys (the pins of the quantised
    formats' deep modules, tests/test_host_fp4_deep.py and tests/test_host_fp8_token_deep.py, pass their module's lists)"""
    import test_gpu_kvcache as tk
    tpp, tiles = page // 32, page * mp // 32
    longest = longest3 = 0
    midpage = last_third = False
    for L, Sq in zip(lens, S):
        if Sq == 0:
            continue
        for H, Hkv in groups:
            for is_causal, window in masks:
                wl, wr = tk.window_of(is_causal, window)
                for n in splits:
                    for tb, s_beg, steps in _work_items(L, Sq, H // Hkv, wl, wr, n, ng):
                        longest = max(longest, max(steps))
                        if n == 3:
                            longest3 = max(longest3, max(steps))
                        midpage |= max(steps) >= 4 and s_beg % tpp != 0
                        last_third |= max(steps) >= 1 and 3 * tb >= 2 * tiles
    return longest, longest3, midpage, last_third


def shares(L, n):
    """(loop steps, tiles) of each split of L keys under the full mask at two tiles per step"""
    nt = -(-L // 32)
    for split in range(n):
        s_beg, s_end = nt * split // n, nt * (split + 1) // n
        yield len(range(s_beg, s_end, 2)), s_end - s_beg


def test_deep_shapes_reach_the_steady_state_of_the_lookup_pipeline():
    """The body looks a table entry up three steps ahead, builds the descriptors two ahead and loads one ahead: an entry
    looked up inside the loop feeds a load only in a wave that runs at least 4 loop steps, and the pipeline is in steady
    state from about 8.  These are conditions on the shapes of tests/test_gpu_paged_deep.py, not measurements: whoever
    shrinks them below the reach that module exists for fails here, on the CPU.  (Forced split counts only: the formula's
    count is one of them.)"""
    import test_gpu_paged_deep as deep
    assert deep.GEOMS == [(32, 44), (64, 22), (96, 15), (128, 11), (160, 9), (224, 7), (256, 6)]
    assert [p // 32 for p, _ in deep.GEOMS] == [1, 2, 3, 4, 5, 7, 8]                # FastDiv's m != 1 at 3, 5, 7
    forced = [n for n in deep.SPLITS if n > 0]
    assert forced == [1, 2, 3, 5, 11] and 0 in deep.SPLITS
    reach = deep_reach(deep.GEOMS, deep.lengths, deep.GROUPS, deep.SQS, deep.MASKS, forced)
    for (page, mp), (longest, longest3, midpage, last_third) in reach.items():
        assert 44 <= page * mp // 32 <= 49, (page, mp)
        assert longest >= 8, (page, mp, longest)                                    # 1. some wave runs at least 8 steps
        assert longest3 >= 4, (page, mp, longest3)                                  # 2. and at least 4 at three splits
        assert midpage or page == 32, (page, mp)                                    # 3. a split of >= 4 steps begins mid-page
        assert last_third, (page, mp)                                               # 4. a first tile in the table's last third
    # the condition has teeth: the same lists over the three pages of tests/test_gpu_paged.py reach none of it
    shallow = deep_reach([(p, 3) for p, _ in deep.GEOMS], deep.lengths, deep.GROUPS, deep.SQS, deep.MASKS, forced)
    for (page, mp), (longest, longest3, _, _) in shallow.items():
        assert longest < 8 and longest3 < 4, (page, longest, longest3)
    # the packed steps run over the same lengths plus the prefill chunk's own
    for page, mp, _, _ in deep.PACKED_GEOMS:
        assert (page, mp) in deep.GEOMS and len(deep.packed_lens(page, mp)) == len(deep.S_PACKED)


# ---- the refusals of the wrappers and of the binding, replayed against the fixture -------------------------------------------
with open(os.path.join(ps.GOLDEN, "paged_errors.json")) as _fh:
    PAGED_ERRORS = json.load(_fh)
ERROR_FUNCTIONS = sorted({cid.split("/")[0] for cid in PAGED_ERRORS["cpu"]})


@functools.lru_cache(maxsize=None)
def _cpu_cases():
    return dict(ps.cpu_cases())


def test_binding_signatures_are_the_recorded_ones():
    assert ps.signatures() == PAGED_ERRORS["signatures"]
    import paged_kvcache, ragged_kvcache
    assert paged_kvcache._ext is ragged_kvcache._ext and paged_kvcache._ext.__name__ == "_mi355fa_paged_torch"


def test_the_error_table_and_the_fixture_list_the_same_cases():
    want = PAGED_ERRORS["cpu"]
    assert sorted(_cpu_cases()) == sorted(want)
    assert ERROR_FUNCTIONS == ["P.flash_attention_kvcache_paged", "R.flash_attention_kvcache_ragged",
                               "ext.kvcache_paged_forward", "ext.kvcache_ragged_forward"]
    for fn in ERROR_FUNCTIONS:     # per function: >= 3 cases that violate two checks at once
        assert sum(1 for cid in want if cid.startswith(fn + "/") and "+" in cid) >= 3, fn
    assert all(v[0] == "AssertionError" for v in want.values())     # refused, every one: nothing returned


@pytest.mark.parametrize("function", ERROR_FUNCTIONS)
def test_malformed_calls_raise_what_they_raised(function):
    cases = _cpu_cases()
    wrong = {}
    for cid, want in PAGED_ERRORS["cpu"].items():
        if cid.startswith(function + "/"):
            got = ps.outcome(cases[cid])
            if got != want:
                wrong[cid] = (got, want)
    assert not wrong, wrong
