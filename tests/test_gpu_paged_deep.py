"""GPU tests of paged and packed decoding over DEEP block tables and page sizes that are not a power of two
(fa_decode_paged_kernel, fa_decode_ragged_kernel and the paged appends; include/mi355fa_paged.h, mi355fa_ragged.h).

tests/test_gpu_paged.py and tests/test_gpu_ragged.py stop at three pages of 32, 64 or 256 keys.  There the kernel's lookup
pipeline (table entry three steps ahead, descriptors two, loads one) runs its prologue only, the division by tiles per page
is a shift, the table is contiguous and no entry is out of range.  The geometries below reach 44 to 49 tiles with 1 to 8
tiles per page, so that waves run up to 13 loop steps and change page on every step or every other one, the multiply path
of FastDiv runs (3, 5, 7 tiles per page), and windows and splits begin many pages into a table and mid-page.
tests/test_host_paged.py holds a CPU model of the body's tb / te / s_beg / s_end arithmetic over THIS module's constants
and fails if the shapes are shrunk below that reach.

  1. the bits of the padded call on the gathered cache, all six variants, every geometry, head group, S_q, mask and split
  2. fp64 on its own per (sequence, head): a whole-tensor norm hides one wrong page of one head
  3. the block table as a slice of a wider tensor: stride(0) > max_pages, a base 12 bytes off 16-byte alignment
  4. packed queries over deep tables against the paged call on each sequence alone, and fp64 per (sequence, head)
  5. the append across page boundaries deep in the table, 16-bit and fp8 pools, paged and packed
  6. table entries outside [0, num_pages): an empty page, a dropped row, nothing touched outside the pool.  The pool is
     the middle of a larger NaN-filled allocation and the bad entries stay within its guard pages, so even a kernel
     without the range check would read or write a guard page: a stray access is a NaN or a changed guard byte
  7. a launch that poisons LDS and registers between the reference call and the paged call

Per-head bounds (test 2, 4, 5) are the project's own: 1e-3 for fp16 and 8e-3 for bf16 per (batch, head), as in
test_gpu_kvcache.test_per_head_against_fp64_at_long_ragged_fill_levels, and LSE by check_lse (plain, fp8) or by the
variants' LSE_BOUND.  Measured on an MI355X (profiles/paged_deep_errors.jsonl, written by this module when
MI355FA_PAGED_DEEP_ERRORS names a file), the worst (sequence, head) of every case:
  fp16: plain 3.9e-4, softcap 3.8e-4, alibi 3.7e-4, sink 4.2e-4, fp8 3.7e-4, fp8_sink 4.9e-4   (bound 1e-3)
  bf16: plain 3.1e-3, softcap 2.9e-3, alibi 2.9e-3, sink 3.0e-3, fp8 2.9e-3, fp8_sink 3.0e-3   (bound 8e-3)
The whole module takes about 40 s on an MI355X (214 cases, the slowest 1.5 s).  Shapes are the smallest that reach each
path."""
import copy
import ctypes
import json
import os

import pytest
import torch

import attn_ref as ar
import blockcheck as bc
import fa_oracle as fo
import pagedcheck as pc
import raggedcheck as rc
import test_gpu_kvcache as tk
import test_gpu_kvcache_fp8 as t8
import test_gpu_paged as tpg
import test_gpu_ragged as trg
import test_gpu_softcap as tsc
import variantcheck as vck

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
GEOMS = [(32, 44), (64, 22), (96, 15), (128, 11), (160, 9), (224, 7), (256, 6)]   # (page_size, max_pages): 44 to 49 tiles
SPLITS = (0, 1, 2, 3, 5, 11)             # 0: the formula
MASKS = tk.MASKS + [(False, (300, 8)), (True, (700, -1))]   # + two that begin mid-table (mid-page at 3, 5, 7 tiles a page)
GROUPS = [(4, 4), (8, 2), (8, 1)]
SQS = (1, 3, 40)
VARIANTS = tpg.VARIANTS
# (D, dtype) per geometry: crossed where the FastDiv multiply path (96) and the benchmarked page (128) run, one pair each
# elsewhere; every variant meets both head dims and both dtypes
_ALL = [(64, F16), (64, BF16), (128, F16), (128, BF16)]
FORMATS = {32: [(64, F16)], 64: [(128, BF16)], 96: _ALL, 128: _ALL, 160: [(64, BF16)], 224: [(128, F16)], 256: [(64, F16)]}
CONFIGS = [(page, mp, D, dt) for page, mp in GEOMS for D, dt in FORMATS[page]]
_name = {F16: "fp16", BF16: "bf16"}
IDS = ["p%dx%d-d%d-%s" % (page, mp, D, _name[dt]) for page, mp, D, dt in CONFIGS]
PER_HEAD = {F16: 1e-3, BF16: 8e-3}       # test_gpu_kvcache.test_per_head_against_fp64_at_long_ragged_fill_levels
LSE_BOUND = tsc.BOUNDS["LSE_BOUND"]      # |LSE - fp64| <= a + u * max |logit|: the same pair in the three variants' files
SOFTCAP = 15.0                           # Case's cap
# packed steps (test 3, 4): S_b per sequence and which of the geometry's lengths (or 130 = S_b) it runs over
S_PACKED = [1, 3, 0, 40, 130, 1, 9]
PACKED_GEOMS = [(32, 44, 64, F16), (96, 15, 128, BF16), (128, 11, 64, BF16), (160, 9, 128, F16)]
GUARD = 4                                # guard pages on each side of the pool in test 6


def lengths(page, mp):
    """the empty sequence, the first tiles, both sides of the middle of the table, its last page and its end"""
    S, h = page * mp, mp // 2
    return [0, 1, 33, h * page - 1, h * page + 33, (mp - 1) * page, (mp - 1) * page + 1, S - 1, S]


def packed_lens(page, mp):
    """key lengths of S_PACKED's sequences: the geometry's own, but L_b = S_b = 130 for the prefill chunk (its early row
    blocks see few tiles); one sequence fills the table"""
    S, h = page * mp, mp // 2
    lens = [h * page + 33, 33, (mp - 1) * page + 1, S - 1, 130, S, h * page - 1]
    assert set(lens) - {130} <= set(lengths(page, mp)) and lens[4] == S_PACKED[4] and S in lens
    return lens


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def case(variant, dtype, D, H, Hkv, Sq, page, mp, seed, lens=None, **kw):
    return tpg.Case(variant, dtype, D, H, Hkv, Sq, page, lengths(page, mp) if lens is None else lens, seed, max_pages=mp, **kw)


def with_table(c, table):
    """the Case or Step `c` over another table (a shallow copy: the pools and every other tensor are shared)"""
    w = copy.copy(c)
    w.table = table
    return w


def record(test, variant, dtype, D, page, mp, worst):
    """one line of profiles/paged_deep_errors.jsonl: appended to the file MI355FA_PAGED_DEEP_ERRORS names, if any"""
    path = os.environ.get("MI355FA_PAGED_DEEP_ERRORS")
    line = dict(test=test, variant=variant, dtype=_name[dtype], D=D, page_size=page, max_pages=mp,
                worst_per_head_rel=worst, bound=PER_HEAD[dtype])
    print(json.dumps(line))
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


# ---- the fp64 truth of one variant ---------------------------------------------------------------------------------------
def truth(variant, mods, q, kc, vc, lens, wl, wr):
    """O [B, H, S_q, D], LSE [B, H, S_q] and SABS (None for plain / fp8) in fp64, per sequence on K / V sliced to L_b (the
    gathered caches carry NaN past it).  plain and fp8: test_gpu_kvcache.ref_fp64, fp8 on the dequantised cache as
    test_gpu_kvcache_fp8.check does; soft cap, ALiBi and sinks: attn_ref.attention_fp64 with the keywords their decode tests
    pass to variantcheck.decode_case."""
    B, H, Sq, D = q.shape
    if variant.startswith("fp8"):
        kc, vc = t8.deq(kc, mods["k_descale"]), t8.deq(vc, mods["v_descale"])
    if variant in ("plain", "fp8"):
        O, LSE = tk.ref_fp64(q, kc, vc, lens, wl, wr)
        return O, LSE, None
    f = dict(dtype=torch.float64, device=q.device)
    O = torch.zeros(B, H, Sq, D, **f)
    LSE = torch.full((B, H, Sq), float("-inf"), **f)
    SABS = torch.zeros(B, H, Sq, **f)
    sinks = mods.get("sinks")
    for b, L in enumerate(lens):
        if L == 0:                                        # no key: O = 0 and LSE = z_h (-inf without sinks)
            if sinks is not None:
                LSE[b] = sinks.double()[:, None].expand(H, Sq)
                SABS[b] = LSE[b].abs()
            continue
        kw = {}
        if variant == "softcap":
            kw = dict(cap=mods["softcap"])
        elif variant == "alibi":
            sl = mods["alibi_slopes"]
            kw = dict(slopes=sl if sl.dim() == 1 else sl[b:b + 1], dist=ar.distance(Sq, L, q.device, L=L))
        else:
            kw = dict(sinks=sinks)
        r = ar.attention_fp64(q[b:b + 1], kc[b:b + 1, :, :L], vc[b:b + 1, :, :L], None, D ** -0.5,
                              ar.visible(Sq, L, wl, wr, q.device, L=L), **kw)
        O[b], LSE[b], SABS[b] = r["O"][0], r["LSE"][0], r["SABS"][0]
    return O, LSE, SABS


def check_against(ref, o, lse, dtype, what):
    """every (sequence, head) of O within PER_HEAD of fp64, LSE row by row, rows without a key exactly 0.  Returns the
    worst (sequence, head) error."""
    O_ref, LSE_ref, SABS = ref
    err = fo.block_errors(O_ref, o, block=o.shape[2])[..., 0]                   # [B, H]
    at = tuple(int(x) for x in torch.unravel_index(err.argmax(), err.shape))
    worst = err[at].item()
    print(what, "worst (b, h)", at, "%.3e" % worst)
    assert (err < PER_HEAD[dtype]).all(), ("(b, h)", at, worst, what)
    if SABS is None:
        tk.check_lse(lse, LSE_ref)
        assert (o[torch.isinf(LSE_ref)] == 0).all(), what
    else:
        fin = torch.isfinite(LSE_ref)
        assert torch.equal(torch.isneginf(lse), ~fin), what
        a, u = LSE_BOUND[dtype]
        assert ((lse.double() - LSE_ref).abs()[fin] <= a + u * SABS[fin]).all(), what
    assert (o[(O_ref == 0).all(-1)] == 0).all(), what
    return worst


# ---- 1. the bits of the padded kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("page,mp,D,dtype", CONFIGS, ids=IDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_deep_paged_call_has_the_bits_of_the_padded_call(variant, page, mp, D, dtype):
    for H, Hkv in GROUPS:
        for Sq in SQS:
            c = case(variant, dtype, D, H, Hkv, Sq, page, mp, seed=D + Sq + H + page)
            for is_causal, window in MASKS:
                kw = dict(is_causal=is_causal, window_size=window)
                for n in SPLITS:
                    vck.splits(n)
                    what = (H, Hkv, Sq, is_causal, window, n)
                    ref = c.padded(**kw)
                    got = c.paged(**kw)
                    assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), what
                    tpg.assert_same(got, ref, what)
                    tpg.assert_same(c.paged(**kw), got, what)             # and its own bits again


# ---- 2. fp64 on its own, per (sequence, head) ------------------------------------------------------------------------------
@pytest.mark.parametrize("page,mp,D,dtype", CONFIGS, ids=IDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_sequence_and_head_matches_fp64(variant, page, mp, D, dtype):
    amp = tsc._amp(SOFTCAP, D ** -0.5, D) if variant == "softcap" else 1.0     # as the soft cap's own decode test
    worst = 0.0
    for H, Hkv in GROUPS:
        for Sq in SQS:
            c = case(variant, dtype, D, H, Hkv, Sq, page, mp, seed=7 + D + Sq + H + page, amp=amp)
            assert c.mods.get("softcap", SOFTCAP) == SOFTCAP
            for is_causal, window in MASKS:
                wl, wr = tk.window_of(is_causal, window)
                ref = truth(variant, c.mods, c.q, c.kc, c.vc, c.lens, wl, wr)   # once per mask, shared by the split counts
                for n in SPLITS:
                    vck.splits(n)
                    o, lse = c.paged(is_causal=is_causal, window_size=window)
                    worst = max(worst, check_against(ref, o, lse, dtype, (H, Hkv, Sq, is_causal, window, n)))
    record("paged", variant, dtype, D, page, mp, worst)


# ---- 3. a strided table ----------------------------------------------------------------------------------------------------
def _wide(c, alloc):
    spare = pc.unused_pages(c.table, alloc, c.page, c.kp.shape[0])
    assert len(spare) >= 5 and all(torch.isnan(c.kp[n].float()).all() for n in spare)
    wide = pc.wide_table(c.table, spare)
    mp = c.table.shape[1]
    assert wide.stride(0) == mp + 7 > wide.shape[1] and wide.stride(1) == 1 and torch.equal(wide, c.table)
    assert wide.data_ptr() % 16 == 12 and not wide.is_contiguous()
    return wide


@pytest.mark.parametrize("page,mp", [(32, 44), (96, 15)])
@pytest.mark.parametrize("variant", ["plain", "fp8"])
def test_table_as_a_slice_of_a_wider_tensor(variant, page, mp):
    D, H, Hkv, Snew, dtype = 128, 8, 2, 3, BF16
    lens = [min(L, page * mp - Snew) for L in lengths(page, mp)]          # room for the append
    full = [L + Snew for L in lens]
    c = case(variant, dtype, D, H, Hkv, 3, page, mp, seed=33 + page, lens=lens, alloc=full)
    w = with_table(c, _wide(c, full))
    g = torch.Generator(device="cuda").manual_seed(34)
    kn, vn = (torch.randn(len(lens), Hkv, Snew, D, generator=g, device="cuda").to(dtype) for _ in range(2))
    for n in (1, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            got = w.paged(**kw)
            assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), (n, is_causal, window)
            tpg.assert_same(got, c.paged(**kw), (n, is_causal, window))
        k1, v1, k2, v2 = c.kp.clone(), c.vp.clone(), c.kp.clone(), c.vp.clone()
        a = c.paged(k1, v1, k_new=kn, v_new=vn, is_causal=True)
        b = w.paged(k2, v2, k_new=kn, v_new=vn, is_causal=True)
        tpg.assert_same(b, a, ("append", n))
        assert torch.isfinite(b[0]).all()
        assert pc.same_bytes(k2, k1) and pc.same_bytes(v2, v1) and not pc.same_bytes(k1, c.kp), n
        # one sequence alone (B = 1: the call passes max_pages as the stride), the base still 12 bytes off
        for s in (4, 8):
            one, ref = copy.copy(c), copy.copy(c)
            mods = {k: (v[s:s + 1] if isinstance(v, torch.Tensor) and v.dim() == 2 else v) for k, v in c.mods.items()}
            one.__dict__.update(q=c.q[s:s + 1], sl=c.sl[s:s + 1], table=w.table[s:s + 1], mods=mods)
            ref.__dict__.update(q=c.q[s:s + 1], sl=c.sl[s:s + 1], table=c.table[s:s + 1].contiguous(), mods=mods)
            assert one.table.data_ptr() % 16 != 0
            tpg.assert_same(one.paged(is_causal=True), ref.paged(is_causal=True), ("B = 1", n, s))
    # the packed call
    plens = [min(L, page * mp - s) for L, s in zip(packed_lens(page, mp), S_PACKED)]
    pfull = [L + s for L, s in zip(plens, S_PACKED)]
    st = trg.Step(variant, dtype, D, H, Hkv, S_PACKED, page, plens, seed=35 + page, alloc=pfull, max_pages=mp)
    sw = with_table(st, _wide(st, pfull))
    tail = sum(st.S)
    new = [[torch.randn(1, Hkv, s, D, generator=g, device="cuda").to(dtype) for s in st.S] for _ in range(2)]
    kn, vn = (rc.pack(x, st.total).contiguous() for x in new)
    for n in (1, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            a, b = st.ragged(**kw), sw.ragged(**kw)
            assert torch.isfinite(b[0][:tail]).all() and not torch.isnan(b[1][:, :tail]).any(), (n, is_causal, window)
            assert bc.same_bits(b[0], a[0]) and bc.same_bits(b[1][:, :tail], a[1][:, :tail]), (n, is_causal, window)
        k1, v1, k2, v2 = st.kp.clone(), st.vp.clone(), st.kp.clone(), st.vp.clone()
        a = st.ragged(k1, v1, k_new=kn, v_new=vn, is_causal=True)
        b = sw.ragged(k2, v2, k_new=kn, v_new=vn, is_causal=True)
        assert bc.same_bits(b[0], a[0]) and bc.same_bits(b[1][:, :tail], a[1][:, :tail]) and torch.isfinite(b[0][:tail]).all(), n
        assert pc.same_bytes(k2, k1) and pc.same_bytes(v2, v1) and not pc.same_bytes(k1, st.kp), n


# ---- 4. packed queries over deep tables ------------------------------------------------------------------------------------
@pytest.mark.parametrize("page,mp,D,dtype", PACKED_GEOMS, ids=["p%dx%d-d%d-%s" % (p, m, D, _name[dt]) for p, m, D, dt in PACKED_GEOMS])
@pytest.mark.parametrize("variant", VARIANTS)
def test_deep_packed_rows_have_the_bits_of_the_paged_call_on_each_sequence(variant, page, mp, D, dtype):
    worst = 0.0
    for H, Hkv in GROUPS:
        st = trg.Step(variant, dtype, D, H, Hkv, S_PACKED, page, packed_lens(page, mp), seed=D + H + page, max_pages=mp)
        tail = sum(st.S)
        kc, vc = pc.gather(st.kp, st.table), pc.gather(st.vp, st.table)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            refs64 = None
            if variant in ("plain", "fp8"):               # fp64 per sequence, once per mask
                wl, wr = tk.window_of(is_causal, window)
                refs64 = [None if s == 0 else truth(variant, st.mods_of(b), st.qs[b], kc[b:b + 1], vc[b:b + 1], [st.lens[b]], wl, wr)
                          for b, s in enumerate(st.S)]
            for n in (1, 3, 11):
                vck.splits(n)
                what = (H, Hkv, is_causal, window, n)
                refs = st.per_sequence(**kw)
                got = st.ragged(**kw)
                assert torch.isfinite(got[0][:tail]).all() and not torch.isnan(got[1][:, :tail]).any(), what
                trg.assert_rows(st, got, refs, what)
                if refs64 is not None:
                    os_, ls = rc.unpack(got[0], st.S), rc.unpack_lse(got[1], st.S)
                    for b, r in enumerate(refs64):
                        if r is not None:
                            worst = max(worst, check_against(r, os_[b], ls[b], dtype, what + (b,)))
    if variant in ("plain", "fp8"):
        record("packed", variant, dtype, D, page, mp, worst)


# ---- 5. the append deep in the table ---------------------------------------------------------------------------------------
APPEND_FORMATS = [("plain", F16), ("plain", BF16), ("fp8", BF16), ("fp8_sink", F16)]


def append_starts(page, mp):
    """the rows before, at and across a page boundary in the middle of the table and at its last page"""
    h = mp // 2
    return [h * page - 1, h * page - 2, h * page, (mp - 1) * page - 1, (mp - 1) * page - 2, (mp - 1) * page]


@pytest.mark.parametrize("page,mp", [(96, 15), (128, 11), (160, 9)])
@pytest.mark.parametrize("variant,dtype", APPEND_FORMATS)
def test_append_deep_in_the_table_is_the_padded_append(variant, dtype, page, mp):
    D, H, Hkv, Sq, Snew = 64, 8, 2, 3, 3
    lens = append_starts(page, mp)
    full = [L + Snew for L in lens]
    c = case(variant, dtype, D, H, Hkv, Sq, page, mp, seed=17 + page, lens=lens, alloc=full)
    g = torch.Generator(device="cuda").manual_seed(18)
    kn, vn = (torch.randn(len(lens), Hkv, Snew, D, generator=g, device="cuda").to(dtype) for _ in range(2))
    after = copy.copy(c)                                                              # the step after: L_b + S_new keys, no append
    after.sl = torch.tensor(full, dtype=torch.int32, device="cuda")
    for n in (0, 3):
        vck.splits(n)
        kc, vc, kp, vp = c.kc.clone(), c.vc.clone(), c.kp.clone(), c.vp.clone()
        ref = c.padded(kc, vc, k_new=kn, v_new=vn, is_causal=True)
        got = c.paged(kp, vp, k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        assert torch.equal(c.sl.cpu(), torch.tensor(lens, dtype=torch.int32))        # cache_seqlens is not modified
        assert not pc.same_bytes(kc, c.kc)                                            # the padded append wrote something
        # the whole pool: the new rows where the table sends them, every other page and row untouched
        (kx, vx), _ = pc.scatter([kc, vc], full, page, kp.shape[0], mp, 0, table=c.table.cpu())
        assert pc.same_bytes(kp, kx) and pc.same_bytes(vp, vx), n
        tpg.assert_same(got, ref, n)
        assert torch.isfinite(got[0]).all()
        # attention sees the new keys: the bits of the next step's call over the pool as the append left it, which is
        # held to fp64 over all L_b + S_new keys per (sequence, head) -- without the new keys the last queries would be
        # some 5e-2 off -- and other bits than the step before
        tpg.assert_same(after.paged(kp, vp, is_causal=True), got, n)
        check_against(truth(variant, c.mods, c.q, pc.gather(kp, c.table), pc.gather(vp, c.table), full, -1, 0),
                      got[0], got[1], dtype, ("append", n))
        assert not bc.same_bits(c.paged(is_causal=True)[0], got[0]), n


@pytest.mark.parametrize("page,mp", [(96, 15), (128, 11), (160, 9)])
@pytest.mark.parametrize("variant,dtype", APPEND_FORMATS)
def test_packed_append_deep_in_the_table_is_the_per_sequence_append(variant, dtype, page, mp):
    D, H, Hkv = 64, 8, 2
    S = [3, 0, 40, 1]
    h = mp // 2
    for lens in ([h * page - 1, h * page, h * page - 2, (mp - 1) * page],
                 [(mp - 1) * page - 2, (mp - 1) * page - 1, (mp - 1) * page - 1, page * mp - 1]):
        full = [L + s for L, s in zip(lens, S)]
        st = trg.Step(variant, dtype, D, H, Hkv, S, page, lens, seed=71 + page, alloc=full, max_pages=mp)
        g = torch.Generator(device="cuda").manual_seed(72)
        new = [[torch.randn(1, Hkv, s, D, generator=g, device="cuda").to(dtype) for s in S] for _ in range(2)]
        kn, vn = (rc.pack(x, st.total).contiguous() for x in new)
        for n in (1, 3):
            vck.splits(n)
            kr, vr, kp, vp = st.kp.clone(), st.vp.clone(), st.kp.clone(), st.vp.clone()
            refs = st.per_sequence(kr, vr, k_new=new[0], v_new=new[1], is_causal=True)
            got = st.ragged(kp, vp, k_new=kn, v_new=vn, is_causal=True)
            torch.cuda.synchronize()
            assert torch.equal(st.sl.cpu(), torch.tensor(lens, dtype=torch.int32))       # cache_seqlens is not modified
            assert not pc.same_bytes(kr, st.kp)                                           # the appends wrote something
            assert pc.same_bytes(kp, kr) and pc.same_bytes(vp, vr), n                     # the whole pool, byte for byte
            trg.assert_rows(st, got, refs, n)
            assert torch.isfinite(got[0][:sum(S)]).all()
            # attention sees the new keys: fp64 over the pool as the append left it, per (sequence, head)
            kc, vc = pc.gather(kp, st.table), pc.gather(vp, st.table)
            os_, ls = rc.unpack(got[0], S), rc.unpack_lse(got[1], S)
            for b, s in enumerate(S):
                if s:
                    r = truth(variant, st.mods_of(b), st.qs[b], kc[b:b + 1], vc[b:b + 1], [full[b]], -1, 0)
                    check_against(r, os_[b], ls[b], dtype, ("packed append", n, b))


# ---- 6. table entries outside the pool, guarded ----------------------------------------------------------------------------
def _plant(table, num_pages, where):
    """a copy of `table` with the entries `where` = [(b, i)] replaced by -1, -GUARD, num_pages, num_pages + GUARD - 1 in
    turn: the only bad entries this module uses, all within GUARD pages of the pool.  Returns it and the pages replaced."""
    bad = [-1, -GUARD, num_pages, num_pages + GUARD - 1]
    t = table.clone()
    lost = []
    for k, (b, i) in enumerate(where):
        lost.append(int(t[b, i]))
        t[b, i] = bad[k % 4]
    assert all(-GUARD <= int(t[b, i]) < num_pages + GUARD and not 0 <= int(t[b, i]) < num_pages for b, i in where)
    return t, lost


@pytest.mark.parametrize("form", ["paged", "packed"])
@pytest.mark.parametrize("variant", ["plain", "fp8_sink"])
def test_out_of_range_entries_read_as_empty_pages_and_drop_their_rows(variant, form):
    """Why this cannot fault: page_desc gives an entry outside [0, num_pages) a descriptor of 0 bytes at the pool's own
    base (every buffer load through it returns 0), paged_dst returns false before any store, and neither binding reads the
    table.  Were either check missing, page * stride for these entries still lands in a guard page of the allocation."""
    page, mp, D, H, Hkv, dtype = 96, 15, 64, 8, 2, F16
    h = mp // 2
    packed = form == "packed"
    S = [1, 3, 40, 3, 9] if packed else [3] * 5
    # sequences 1 and 3 get the bad entries; their appends start one row before the boundary of the pages h and mp - 1
    lens = [h * page + 33, h * page - 1, 33, (mp - 1) * page - 1, page * mp - 40]
    full = [L + s for L, s in zip(lens, S)]
    where = [(1, 0), (1, h), (3, 1), (3, mp - 1), (3, h)]                  # below ceil(L_b / page), with or without the append
    assert all(i < pc.pages_of(lens[b], page) or i == pc.pages_of(full[b], page) - 1 for b, i in where)
    if packed:
        c = trg.Step(variant, dtype, D, H, Hkv, S, page, lens, seed=91, alloc=full, max_pages=mp)
    else:
        c = case(variant, dtype, D, H, Hkv, 3, page, mp, seed=91, lens=lens, alloc=full)
    NP = c.kp.shape[0]
    (bigk, c.kp), (bigv, c.vp) = pc.guarded(c.kp, GUARD), pc.guarded(c.vp, GUARD)
    assert c.kp.data_ptr() == bigk[GUARD].data_ptr() and c.kp.is_contiguous() and c.kp.shape[0] == NP
    table, lost = _plant(c.table, NP, where)
    bad = with_table(c, table)
    run = (lambda x, *a, **kw: x.ragged(*a, **kw)) if packed else (lambda x, *a, **kw: x.paged(*a, **kw))

    def split_rows(res):
        """[(O, LSE) of sequence b]"""
        if packed:
            return list(zip(rc.unpack(res[0], S), rc.unpack_lse(res[1], S)))
        return [(res[0][b], res[1][b]) for b in range(len(S))]

    def compare(got, clean, what):
        for b, ((o, lse), (ro, rl)) in enumerate(zip(split_rows(got), split_rows(clean))):
            if b in (1, 3):                                                # an empty page reads as zeros: no guard NaN
                assert torch.isfinite(o).all() and not torch.isnan(lse).any(), (what, b)
            else:
                assert bc.same_bits(o, ro) and bc.same_bits(lse, rl), (what, b)

    g = torch.Generator(device="cuda").manual_seed(92)
    if packed:
        new = [[torch.randn(1, Hkv, s, D, generator=g, device="cuda").to(dtype) for s in S] for _ in range(2)]
        kn, vn = (rc.pack(x, c.total).contiguous() for x in new)
    else:
        kn, vn = (torch.randn(len(S), Hkv, 3, D, generator=g, device="cuda").to(dtype) for _ in range(2))
    for n in (1, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            compare(run(bad, **kw), run(c, **kw), (n, is_causal, window))
        assert pc.guards_intact(bigk, GUARD) and pc.guards_intact(bigv, GUARD)
        # the append: through the clean table, then through the bad one into a second guarded copy
        (ck, k1), (cv, v1) = pc.guarded(c.kp, GUARD), pc.guarded(c.vp, GUARD)
        (bk, k2), (bv, v2) = pc.guarded(c.kp, GUARD), pc.guarded(c.vp, GUARD)
        clean = run(c, k1, v1, k_new=kn, v_new=vn, is_causal=True)
        got = run(bad, k2, v2, k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        compare(got, clean, ("append", n))
        for big in (ck, cv, bk, bv):
            assert pc.guards_intact(big, GUARD), n
        # the rows bound for a replaced page are dropped -- that page keeps every byte -- and every other row is where the
        # clean append put it; every page no sequence names keeps every byte (the whole pool is compared)
        kx, vx = k1.clone(), v1.clone()
        for pgn in lost:
            pc._bytes(kx)[pgn], pc._bytes(vx)[pgn] = pc._bytes(c.kp)[pgn], pc._bytes(c.vp)[pgn]
        assert not pc.same_bytes(kx, k1) and not pc.same_bytes(k1, c.kp), n               # rows were dropped, rows were written
        assert pc.same_bytes(k2, kx) and pc.same_bytes(v2, vx), n


# ---- 7. a poisoned launch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "fp8"])
def test_poisoned_lds_and_registers_do_not_reach_the_result(variant):
    """fa_debug_poison (NaN patterns in every CU's LDS and registers, as in tests/test_gpu_race.py) between the reference
    call and the paged call: the V tile, the merge stage and the carried descriptors take nothing from the launch before."""
    import _mi355fa as fa
    poison = fa.lib.fa_debug_poison
    poison.argtypes = [ctypes.c_void_p]
    poison.restype = ctypes.c_int
    page, mp = 96, 15
    c = case(variant, BF16, 128, 8, 1, 40, page, mp, seed=101)
    for n in (1, 3, 5):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            ref = c.padded(**kw)
            assert poison(torch.cuda.current_stream().cuda_stream) == 0
            got = c.paged(**kw)
            assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), (n, is_causal, window)
            tpg.assert_same(got, ref, (n, is_causal, window))
