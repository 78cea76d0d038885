"""GPU tests of per-token-scaled e4m3 decoding over DEEP block tables and strided scale pools (the KVT forms of
csrc/fa_decode_body.inc, padded, paged and packed, plain and soft-capped, and the quantising appends;
include/mi355fa_kvcache_fp8_token.h, fp8_token_kvcache.py, quant_softcap_kvcache.py).

tests/test_gpu_kvcache_fp8_token.py and tests/test_gpu_ragged_fp8_token.py stop at 9 tiles: there a wave runs at most 3 loop
steps, so the lookup pipeline of the body (table entry three steps ahead, descriptors two, loads one) runs its prologue only --
and with KVT that pipeline also carries the two descriptors of the page's rows of the fp32 scale pools (rksp, rvsp) and two scale
offsets (sbkp, sbvp) over the loop's back edge.  The geometries below are those of tests/test_gpu_fp4_deep.py, 44 to 49 tiles
with 1, 3, 4, 5 and 7 tiles per page: waves of up to 12 steps (22 at D = 256, where a workgroup takes two tiles a step), the
multiply path of FastDiv, windows and splits that begin many pages into a table and mid-page, and padded caches of 1408 to 1568
rows.  tests/test_host_fp8_token_deep.py holds the CPU model of the body's arithmetic over THIS module's constants and fails if
the shapes are shrunk below that reach.

  1. the bits of the padded call on the padded cache and scales: every geometry, head group, S_q, mask, split count, sinks or not
  2. fp64 (fp8tokencheck.truth on the fp64 dequantised cache) per (sequence, head), the padded and the paged call; the empty
     sequence is O = 0 and LSE = -inf, or the sink's logit
  3. strided storage, deep: the block table as a slice of a wider tensor, the scale pools and the cache pools stored
     [num_pages, page_size, H_kv(, D)], the scale pools with a page stride above H_kv * page_size (NaN slack) -- each the bits
     of the contiguous call, paged and packed, with the append
  4. packed queries at D = 64 and 128: the rows of a sequence have the bits of the paged call on it alone; fp64 per (sequence, head)
  5. packed queries at D = 256 (no rectangular sibling): the bits of the packed call on the sequence alone; fp64 likewise
  6. appends deep in the table, paged and packed: the four pools afterwards are the old bits with quantize_kv_fp8_per_token's
     CPU bytes and scale bits in exactly the appended rows
  7. table entries outside [0, num_pages) at positions a wave looks up inside its loop.  The four pools are the middle of larger
     allocations whose guard pages are 0xFF (bytes) or NaN (scales) and the bad entries name guard pages of the same allocation
     only, so this is defined behaviour, never a fault: page_desc gives such an entry four descriptors of 0 bytes at the pools'
     own bases and the append drops the row before any store
  8. the soft-capped per-token kernels (quant_softcap_kvcache, format "token") over the same tables, with
     tests/quantcapcheck.py's inputs, truth and bounds

Inputs are fp8tokencheck.make's recipe: rows whose amax is 2^e, e uniform and no integer (the scales are no powers of two), K rows
over 2^-6 .. 2^1, V rows over 2^-6 .. 2^6, quantised by quantize_kv_fp8_per_token, q ~ N(0, 1); one sequence of every cache has V
rows of amax 2^-6 throughout (v_scale ~ 2^-14.8: the split of v_scale into exponent and mantissa stays under test many pages
deep).  Every cache byte no sequence owns is 0xFF and every such scale NaN.  The softmax is broad by construction, so that a
wrong page moves the result: every cache asserts that no unmasked row of a sequence with at least 256 keys gives a key a
probability of 0.05 (BROAD; fp64, before any kernel runs).  The bounds are the project's own per (sequence, head): relative
Frobenius 1e-3 (fp16) / 8e-3 (bf16), LSE by check_lse.  Measured on an MI355X (profiles/fp8_token_deep_errors.jsonl, written by
this module when MI355FA_FP8_TOKEN_DEEP_ERRORS names a file), the worst (sequence, head) over every case:
  fp16: padded 5.7e-4, paged 5.7e-4, packed 4.8e-4   (bound 1e-3)
  bf16: padded 4.8e-3, paged 4.8e-3, packed 3.5e-3   (bound 8e-3)
Run on its own the module takes about 25 s on an MI355X (105 cases; the slowest 1.7 s, the first fp64 case, which warms the
device up, every other below 0.4 s).  Shapes are the smallest that reach each path.

Teeth, on a scratch build whose in-loop page_desc (the call at t + 2 NG) leaves rksp, rvsp, sbkp and sbvp as they were: 70 of
these 105 cases fail -- every one that compares numbers of a paged or packed call; the 22 padded fp64 cases, the 8 strided-storage
cases and the 5 out-of-range cases compare that build with itself or do not run the paged loop -- against 10 of 37 in
tests/test_gpu_kvcache_fp8_token.py and 6 of 19 in tests/test_gpu_ragged_fp8_token.py.  With the same change taking effect only
from a wave's second in-loop page_desc on (waves of 4 steps and more), the two older modules pass every case and this module
fails the same 70."""
import gc
import json
import os

import pytest
import torch

import fa_oracle as fo
import fp8tokencheck as tk
import pagedcheck as pc
import quantcapcheck as qc
import raggedcheck as rg
import variantcheck as vck
import test_gpu_kvcache_fp8_token as tt
import test_gpu_paged_deep as deep
from fp8tokencheck import BF16, BOUND, F16

pytestmark = pytest.mark.gpu

GEOMS = [(32, 44), (96, 15), (128, 11), (160, 9), (224, 7)]    # (page_size, max_pages): 44 to 49 tiles; 1, 3, 4, 5, 7 a page
SPLITS = (0, 1, 2, 3, 5, 11)                # 0: the formula
MASKS = tt.MASKS + [(False, (300, 8)), (True, (700, -1))]      # + two that begin mid-table (mid-page at 3, 5, 7 tiles a page)
GROUPS = [(4, 4), (8, 2), (8, 1)]
SQS = (1, 3, 40)
lengths, packed_lens, S_PACKED = deep.lengths, deep.packed_lens, deep.S_PACKED
# (D, dtype) per geometry: crossed where the FastDiv multiply path (96) and the benchmarked page (128) run, one pair elsewhere
_ALL = [(64, F16), (64, BF16), (128, F16), (128, BF16)]
FORMATS = {32: [(64, F16)], 96: _ALL, 128: _ALL, 160: [(128, BF16)], 224: [(64, BF16)]}
CONFIGS = [(page, mp, D, dt) for page, mp in GEOMS for D, dt in FORMATS[page]]
_name = {F16: "fp16", BF16: "bf16"}
_id = lambda rows: ["p%dx%d-d%d-%s" % (page, mp, D, _name[dt]) for page, mp, D, dt in rows]
PACKED_GEOMS = [(32, 44, 64, F16), (96, 15, 128, BF16), (128, 11, 128, F16), (224, 7, 64, BF16)]
PACKED_256 = [(32, 44, 256, F16), (96, 15, 256, BF16), (224, 7, 256, F16)]
PACKED_SPLITS = (1, 3, 11)
PAD = 2                                     # total_q is two rows larger than cu[B]
GUARD = 4                                   # guard pages on each side of the pools in test 7
SINKS = [False, True]
SINK_IDS = ["nosink", "sinks"]
K_SPAN, V_SPAN, SMALL_V = (-6.0, 1.0), (-6.0, 6.0), (-6.0, -6.0)   # log2 of the rows' amax
BROAD, BROAD_FROM = 0.05, 256               # no key of an unmasked row gets this probability, in sequences of >= 256 keys
FF = 0xFF                                   # the poison byte (an e4m3 NaN, like 0x7f, which pagedcheck fills with)
CAP = 30.0                                  # test 8
U8, I32 = torch.uint8, torch.int32


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def record(test, dtype, D, page, mp, sink, worst):
    """one line of profiles/fp8_token_deep_errors.jsonl: appended to the file MI355FA_FP8_TOKEN_DEEP_ERRORS names, if any"""
    path = os.environ.get("MI355FA_FP8_TOKEN_DEEP_ERRORS")
    line = dict(test=test, dtype=_name[dtype], D=D, page_size=page, max_pages=mp, sinks=sink, worst_per_head_rel=worst,
                bound=BOUND[dtype])
    print(json.dumps(line))
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def bits(t):
    """e4m3 bytes as uint8, fp32 scales as int32: comparing and indexing without NaN semantics (views, strided ones too)"""
    return t.view({1: U8, 4: I32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def queries(B, H, Sq, D, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(B, H, Sq, D, generator=g, device="cuda").to(dtype)


def sinks_of(H):
    return torch.linspace(-1.0, 3.0, H, device="cuda", dtype=torch.float32)


def new_rows(B, Hkv, Snew, D, dtype, seed):
    """k_new / v_new [B, H_kv, S_new, D] by the caches' recipe, with one all-zero row each"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    kn, vn = (tk.rows((B, Hkv, Snew, D), *V_SPAN, g).to(dtype) for _ in range(2))
    kn[1, 0, 0] = 0
    vn[2, Hkv - 1, -1] = 0
    return kn, vn


# ---- the caches: built once per (geometry, format, H_kv, fill levels), shared by the tests and never written ----------------
class Cache:
    """pad: the padded k_cache, v_cache [B, H_kv, page * mp, D] and k_scale, v_scale [B, H_kv, page * mp], 0xFF / NaN at and past
    L_b; pools / table: the same rows under a permuted table with pages for owned[b] >= L_b rows, every byte no sequence owns
    0xFF and every such scale NaN; K, V: the dequantised cache in fp64 (NaN past L_b).  Sequence `small`, the longest, has V rows
    of amax 2^-6."""

    def __init__(self, page, mp, D, dtype, Hkv, lens, owned, seed):
        B = len(lens)
        self.lens, self.owned, self.page, self.mp = list(lens), list(owned), page, mp
        self.small = max(range(B), key=lambda b: lens[b])
        _, k8, v8, ks, vs = tk.make(B, Hkv, Hkv, 1, page * mp, D, dtype, seed=seed, span=V_SPAN, k_span=K_SPAN,
                                    v_span={self.small: SMALL_V})
        assert float(vs[self.small].max()) < 2.0 ** -14 and float(ks.max()) < 2.001 / 448 and float(vs.max()) > 16.0 / 448
        assert not (bits(k8) == 0x7F).any() and not (bits(v8) == 0x7F).any()       # the quantiser writes no NaN byte
        self.NP = sum(pc.pages_of(L, page) for L in owned) + 4
        *pools, self.table = tk.scatter(k8, v8, ks, vs, self.lens, page, self.NP, mp, seed + 1, alloc=self.owned)
        for t in pools[:2]:                                                        # pagedcheck's NaN byte -> 0xFF
            b = bits(t)
            b[b == 0x7F] = FF
        for b, L in enumerate(lens):
            bits(k8)[b, :, L:] = FF
            bits(v8)[b, :, L:] = FF
            ks[b, :, L:] = float("nan")
            vs[b, :, L:] = float("nan")
        self.pad, self.pools = [k8, v8, ks, vs], pools
        self.spare = pc.unused_pages(self.table, self.owned, page, self.NP)
        assert len(self.spare) == 4 and all(bool((bits(t)[self.spare] == FF).all()) for t in pools[:2]) and \
            all(bool(torch.isnan(t[self.spare]).all()) for t in pools[2:])
        self.K, self.V = tk.deq64(k8, ks), tk.deq64(v8, vs)
        self.sl = torch.tensor(self.lens, dtype=I32, device="cuda")
        # the condition on the inputs: a broad softmax, from the fp64 cache alone
        q = queries(B, Hkv, 3, D, dtype, seed + 2).double()
        long = [b for b, L in enumerate(lens) if L >= BROAD_FROM]
        self.peak = max(float(torch.softmax(q[b] @ self.K[b, :, :lens[b]].transpose(-1, -2) * D ** -0.5, -1).max()) for b in long)
        assert long and self.peak < BROAD, (self.peak, page, mp, D)


_CACHES = {}                                # the last few, so that a case's loops and its neighbours share one


@pytest.fixture(scope="module", autouse=True)
def _caches_end_with_the_module():
    """The caches are dropped after the module's last test.  Left alive, their blocks stay scattered over the caching
    allocator's segments for the rest of the session, and a later test that accounts for its allocations to the byte
    (test_bshd_views_are_read_in_place of tests/test_gpu_gqa.py) is handed an unsplittable larger block between them."""
    yield
    _CACHES.clear()
    gc.collect()


def cache(page, mp, D, dtype, Hkv, lens=None, owned=None, seed=0):
    lens = tuple(lengths(page, mp) if lens is None else lens)
    owned = lens if owned is None else tuple(owned)
    key = (page, mp, D, dtype, Hkv, lens, owned, seed)
    if key not in _CACHES:
        while len(_CACHES) >= 8:
            del _CACHES[next(iter(_CACHES))]
        _CACHES[key] = Cache(page, mp, D, dtype, Hkv, lens, owned, seed + page + D + Hkv)
    return _CACHES[key]


def gathered64(pools, table):
    """K, V in fp64 of the padded cache the four pools and the table describe"""
    return (tk.deq64(pc.gather(pools[0], table), tk.gather_scales(pools[2], table)),
            tk.deq64(pc.gather(pools[1], table), tk.gather_scales(pools[3], table)))


def held(tag, q, o, lse, ref, lens):
    """fp8tokencheck.held, rows without a key exactly 0; returns the worst (sequence, head) error"""
    tk.held(tag, q, o, lse, *ref, lens)
    assert (o[(ref[0] == 0).all(-1)] == 0).all(), tag
    return float(fo.block_errors(ref[0], o, block=q.shape[2]).max())


def finite(res):
    return bool(torch.isfinite(res[0]).all()) and not bool(torch.isnan(res[1]).any())


# ---- 1. the bits of the padded call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sink", SINKS, ids=SINK_IDS)
@pytest.mark.parametrize("page,mp,D,dtype", CONFIGS, ids=_id(CONFIGS))
def test_deep_paged_call_has_the_bits_of_the_padded_call(page, mp, D, dtype, sink):
    for H, Hkv in GROUPS:
        c = cache(page, mp, D, dtype, Hkv)
        sk = sinks_of(H) if sink else None
        table = pc.wide_table(c.table, c.spare) if Hkv == 2 else c.table
        for Sq in SQS:
            q = queries(len(c.lens), H, Sq, D, dtype, seed=D + Sq + H + page)
            for is_causal, window in MASKS:
                kw = dict(is_causal=is_causal, window_size=window, sinks=sk)
                for n in SPLITS:
                    vck.splits(n)
                    what = (H, Hkv, Sq, is_causal, window, n)
                    ref = tk.padded(q, *c.pad, c.sl, **kw)
                    got = tk.paged(q, *c.pools, c.sl, table, **kw)
                    assert finite(got), what
                    assert tk.same(got, ref), what


# ---- 2. fp64 on its own, per (sequence, head) --------------------------------------------------------------------------------
@pytest.mark.parametrize("sink", SINKS, ids=SINK_IDS)
@pytest.mark.parametrize("call", ["padded", "paged"])
@pytest.mark.parametrize("page,mp,D,dtype", CONFIGS, ids=_id(CONFIGS))
def test_every_sequence_and_head_matches_fp64(page, mp, D, dtype, call, sink):
    worst = 0.0
    for H, Hkv in GROUPS:
        c = cache(page, mp, D, dtype, Hkv)
        assert 0 in c.lens                                                         # the empty sequence
        sk = sinks_of(H) if sink else None
        for Sq in SQS:
            q = queries(len(c.lens), H, Sq, D, dtype, seed=7 + D + Sq + H + page)
            for is_causal, window in MASKS:
                kw = dict(is_causal=is_causal, window_size=window, sinks=sk)
                ref = tk.truth(q, c.K, c.V, c.lens, is_causal, window, sinks=sk)   # once per mask, shared by the splits
                e = c.lens.index(0)
                assert (ref[0][e] == 0).all() and (torch.equal(ref[1][e], sk.double()[:, None].expand(H, Sq)) if sink
                                                   else torch.isneginf(ref[1][e]).all())
                for n in SPLITS:
                    vck.splits(n)
                    if call == "padded":
                        o, lse = tk.padded(q, *c.pad, c.sl, **kw)
                    else:
                        o, lse = tk.paged(q, *c.pools, c.sl, c.table, **kw)
                    worst = max(worst, held("%s %s" % (call, (H, Hkv, Sq, is_causal, window, n)), q, o, lse, ref, c.lens))
    record(call, dtype, D, page, mp, sink, worst)


# ---- 4, 5 (and the packed halves of 3, 6, 7). packed queries over deep tables ------------------------------------------------
class Step:
    """one packed step over a deep table: S_PACKED's query counts (or `S`) over packed_lens' fill levels (or `lens`)"""

    def __init__(self, page, mp, D, dtype, H, Hkv, seed, S=None, lens=None, owned=None):
        self.S = list(S_PACKED if S is None else S)
        self.c = cache(page, mp, D, dtype, Hkv, packed_lens(page, mp) if lens is None else lens, owned, seed=seed)
        assert len(self.c.lens) == len(self.S)
        self.rows, self.tq = sum(self.S), sum(self.S) + PAD
        qb = queries(len(self.S), H, max(self.S), D, dtype, seed=seed + 3)
        self.q_seq = [qb[b:b + 1, :, :s].contiguous() for b, s in enumerate(self.S)]

    def ragged(self, table, pools=None, **kw):
        """per sequence (O [1, H, S_b, D], LSE [1, H, S_b]) of the packed call; k_new / v_new: per sequence"""
        return tk.packed(self.q_seq, *(self.c.pools if pools is None else pools), self.c.sl, table, total_q=self.tq, **kw)

    def alone(self, b, pools=None, k_new=None, v_new=None, **kw):
        """(O [1, H, S_b, D], LSE [1, H, S_b]) of sequence b on its own: the paged call at D <= 128, the packed call with
        B = 1 at D = 256, which has no rectangular sibling"""
        c, pools = self.c, self.c.pools if pools is None else pools
        if self.q_seq[b].shape[-1] == 256:
            one = lambda t: None if t is None else [t]
            return tk.packed([self.q_seq[b]], *pools, c.sl[b:b + 1], c.table[b:b + 1], k_new=one(k_new), v_new=one(v_new), **kw)[0]
        return tk.paged(self.q_seq[b], *pools, c.sl[b:b + 1], c.table[b:b + 1], k_new=k_new, v_new=v_new, **kw)


# ---- 3. strided storage, deep ------------------------------------------------------------------------------------------------
STORAGE = ["table", "scales-by-row", "caches-by-row", "scales-page-stride"]
SLACK = 24                                  # floats between the pages of the scale pools in "scales-page-stride"


def stored(form, pools, table, spare):
    """(pools, table, bigs): copies of the pools and the table in the storage `form`; bigs: the allocations that hold slack"""
    kp, vp, ksp, vsp = (t.clone() for t in pools)
    by_row = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)              # [num_pages, page, H_kv, ..] storage
    bigs = []
    if form == "table":
        w = pc.wide_table(table, spare)
        assert w.stride(0) == table.shape[1] + 7 > w.shape[1] and w.stride(1) == 1 and torch.equal(w, table)
        assert not w.is_contiguous() and w.data_ptr() % 16 == 12
        table = w
    elif form == "scales-by-row":
        ksp, vsp = by_row(ksp), by_row(vsp)
        assert ksp.stride(2) == vsp.stride(2) == ksp.shape[1] and ksp.stride(1) == 1 and not ksp.is_contiguous()
    elif form == "caches-by-row":
        kp, vp = by_row(kp), by_row(vp)
        assert kp.stride(2) == kp.shape[1] * kp.shape[3] and kp.stride(1) == kp.shape[3] and not kp.is_contiguous()
    else:
        NP, Hkv, page = ksp.shape
        views = []
        for t in (ksp, vsp):
            big = torch.full((NP, Hkv * page + SLACK), float("nan"), dtype=torch.float32, device=t.device)
            big[:, :Hkv * page] = t.reshape(NP, -1)
            views.append(big[:, :Hkv * page].unflatten(1, (Hkv, page)))
            bigs.append(big)
        ksp, vsp = views
        assert ksp.stride() == (Hkv * page + SLACK, page, 1) and ksp.data_ptr() == bigs[0].data_ptr() and not ksp.is_contiguous()
    assert all(same_bits(a, b) for a, b in zip((kp, vp, ksp, vsp), pools))
    return [kp, vp, ksp, vsp], table, bigs


def slack_intact(bigs):
    return all(bool(torch.isnan(big[:, big.shape[1] - SLACK:]).all()) for big in bigs)


@pytest.mark.parametrize("form", STORAGE)
@pytest.mark.parametrize("page,mp", [(32, 44), (96, 15)])
def test_strided_tables_scales_and_caches_give_the_bits_of_the_contiguous_call(page, mp, form):
    D, H, Hkv, Sq, Snew, dtype = 128, 8, 2, 3, 3, BF16
    lens = [min(L, page * mp - Snew) for L in lengths(page, mp)]                  # room for the append
    c = cache(page, mp, D, dtype, Hkv, lens, [L + Snew for L in lens], seed=33)
    P, T, bigs = stored(form, c.pools, c.table, c.spare)
    q = queries(len(lens), H, Sq, D, dtype, seed=34)
    kn, vn = new_rows(len(lens), Hkv, Snew, D, dtype, 35)
    for n in (1, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            got = tk.paged(q, *P, c.sl, T, **kw)
            assert finite(got), (n, is_causal, window)
            assert tk.same(got, tk.paged(q, *c.pools, c.sl, c.table, **kw)), (n, is_causal, window)
        p1 = [t.clone() for t in c.pools]
        p2, T2, bigs2 = stored(form, c.pools, c.table, c.spare)
        a = tk.paged(q, *p1, c.sl, c.table, k_new=kn, v_new=vn, is_causal=True)
        b = tk.paged(q, *p2, c.sl, T2, k_new=kn, v_new=vn, is_causal=True)
        assert tk.same(b, a) and finite(b), ("append", n)
        assert all(same_bits(x, y) for x, y in zip(p1, p2)) and not same_bits(p1[2], c.pools[2]) and slack_intact(bigs2), n
        if form == "table":   # one sequence alone (B = 1: the call passes max_pages as the stride), the base still 12 bytes off
            for s in (4, 8):
                one = tk.paged(q[s:s + 1], *c.pools, c.sl[s:s + 1], T[s:s + 1], is_causal=True)
                ref = tk.paged(q[s:s + 1], *c.pools, c.sl[s:s + 1], c.table[s:s + 1].contiguous(), is_causal=True)
                assert T[s:s + 1].data_ptr() % 16 != 0 and tk.same(one, ref), ("B = 1", n, s)
    assert slack_intact(bigs) and all(same_bits(x, y) for x, y in zip(P, c.pools))
    # the packed call, and its append
    lens = [min(L, page * mp - s) for L, s in zip(packed_lens(page, mp), S_PACKED)]
    st = Step(page, mp, D, dtype, H, Hkv, seed=36, lens=lens, owned=[L + s for L, s in zip(lens, S_PACKED)])
    c = st.c
    P, T, bigs = stored(form, c.pools, c.table, c.spare)
    kn_b, vn_b = new_rows(len(lens), Hkv, max(S_PACKED), D, dtype, 37)
    kn, vn = ([x[b:b + 1, :, :s].contiguous() for b, s in enumerate(S_PACKED)] for x in (kn_b, vn_b))
    agree = lambda a, b: all(tk.same(x, y) for x, y in zip(a, b))
    for n in (1, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            a, b = st.ragged(c.table, **kw), st.ragged(T, P, **kw)
            assert all(finite(x) for x in b) and agree(a, b), (n, is_causal, window)
        p1 = [t.clone() for t in c.pools]
        p2, T2, bigs2 = stored(form, c.pools, c.table, c.spare)
        a = st.ragged(c.table, p1, k_new=kn, v_new=vn, is_causal=True)
        b = st.ragged(T2, p2, k_new=kn, v_new=vn, is_causal=True)
        assert all(finite(x) for x in b) and agree(a, b), ("packed append", n)
        assert all(same_bits(x, y) for x, y in zip(p1, p2)) and not same_bits(p1[2], c.pools[2]) and slack_intact(bigs2), n
    assert slack_intact(bigs) and all(same_bits(x, y) for x, y in zip(P, c.pools))


# ---- 4, 5. packed queries ----------------------------------------------------------------------------------------------------
def _packed(page, mp, D, dtype, sink):
    worst = 0.0
    for H, Hkv in GROUPS:
        st = Step(page, mp, D, dtype, H, Hkv, seed=D + H)
        c = st.c
        sk = sinks_of(H) if sink else None
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window, sinks=sk)
            refs64 = [None if s == 0 else tk.truth(st.q_seq[b], c.K[b:b + 1], c.V[b:b + 1], [c.lens[b]], is_causal, window, sinks=sk)
                      for b, s in enumerate(st.S)]                          # fp64 per sequence, once per mask
            for n in PACKED_SPLITS:
                vck.splits(n)
                what = (H, Hkv, is_causal, window, n)
                for b, (got, s) in enumerate(zip(st.ragged(c.table, **kw), st.S)):
                    if s:
                        assert finite(got), what + (b,)
                        assert tk.same(got, st.alone(b, **kw)), what + (b,)
                        worst = max(worst, held("packed %s b=%d" % (what, b), st.q_seq[b], *got, refs64[b], [c.lens[b]]))
    record("packed", dtype, D, page, mp, sink, worst)


@pytest.mark.parametrize("sink", SINKS, ids=SINK_IDS)
@pytest.mark.parametrize("page,mp,D,dtype", PACKED_GEOMS, ids=_id(PACKED_GEOMS))
def test_deep_packed_rows_have_the_bits_of_the_paged_call_on_each_sequence(page, mp, D, dtype, sink):
    _packed(page, mp, D, dtype, sink)


@pytest.mark.parametrize("sink", SINKS, ids=SINK_IDS)
@pytest.mark.parametrize("page,mp,D,dtype", PACKED_256, ids=_id(PACKED_256))
def test_deep_d256_rows_have_the_bits_of_the_sequence_alone(page, mp, D, dtype, sink):
    """NG is 2 here: the odd and empty shares of a wave pair, which only join the barrier, occur many pages deep, and both
    waves of a pair read the same row scales"""
    _packed(page, mp, D, dtype, sink)


# ---- 6. appends deep in the table --------------------------------------------------------------------------------------------
_APPEND = [(96, 15, 64, F16), (128, 11, 128, BF16), (160, 9, 64, BF16)]
APPEND_CONFIGS = [(form,) + c for form in ("paged", "packed") for c in _APPEND] + [("packed", 96, 15, 256, F16)]   # D = 256: packed only


def appended(pools, table, page, fills, new):
    """the pools with quantize_kv_fp8_per_token's CPU bytes and scale bits of new[b] = (k_new, v_new) [1, H_kv, S_b, D] in the
    rows [fills[b], fills[b] + S_b) of sequence b, through the table; every other bit as it was"""
    want = [t.clone() for t in pools]
    tab = table.cpu()
    for b, (kn, vn) in enumerate(new):
        if kn.shape[2] == 0:
            continue
        (kq, kqs), (vq, vqs) = tk.T().quantize_kv_fp8_per_token(kn.cpu()), tk.T().quantize_kv_fp8_per_token(vn.cpu())
        for i in range(kn.shape[2]):
            row = fills[b] + i
            pg, r = int(tab[b, row // page]), row % page
            for t, x in zip(want, (kq, vq, kqs, vqs)):
                bits(t)[pg, :, r] = bits(x)[0, :, i].cuda()
    return want


@pytest.mark.parametrize("form,page,mp,D,dtype", APPEND_CONFIGS, ids=[c[0] + "-" + i for c, i in zip(APPEND_CONFIGS, _id(c[1:] for c in APPEND_CONFIGS))])
def test_append_deep_in_the_table_writes_exactly_the_quantised_rows(form, page, mp, D, dtype):
    """rows [L, L + S_new) that cross a page boundary in the table's second half, and that end at its reach"""
    H, Hkv = 8, 2
    h, reach = mp // 2 + 1, page * mp
    assert 2 * h > mp
    if form == "paged":
        S = [3] * 6
        fills = [h * page - 1, h * page - 2, h * page, (mp - 1) * page - 1, (mp - 1) * page - 2, reach - 3]
    else:
        S = [3, 0, 40, 1, 5]
        fills = [h * page - 1, h * page, (mp - 1) * page - 20, (mp - 1) * page - 1, reach - 5]
    after = [f + s for f, s in zip(fills, S)]
    assert max(after) == reach and sum(f // page != (a - 1) // page >= mp // 2 for f, a, s in zip(fills, after, S) if s) >= 2
    st = Step(page, mp, D, dtype, H, Hkv, seed=61, S=S, lens=fills, owned=after)
    c = st.c
    kn_b, vn_b = new_rows(len(S), Hkv, max(S), D, dtype, 62)
    new = [(kn_b[b:b + 1, :, :s].contiguous(), vn_b[b:b + 1, :, :s].contiguous()) for b, s in enumerate(S)]
    want = appended(c.pools, c.table, page, fills, new)
    assert not any(same_bits(w, p) for w, p in zip(want, c.pools))
    K, V = gathered64(want, c.table)
    full = torch.tensor(after, dtype=I32, device="cuda")
    for n in (0, 3):
        vck.splits(n)
        pools = [t.clone() for t in c.pools]
        if form == "paged":
            q = torch.cat(st.q_seq)
            o, lse = tk.paged(q, *pools, c.sl, c.table, k_new=kn_b, v_new=vn_b, is_causal=True)
            nxt = tk.paged(q, *want, full, c.table, is_causal=True)
        else:
            res = st.ragged(c.table, pools, k_new=[x[0] for x in new], v_new=[x[1] for x in new], is_causal=True)
            nxt = tk.packed(st.q_seq, *want, full, c.table, total_q=st.tq, is_causal=True)
        torch.cuda.synchronize()
        assert torch.equal(c.sl.cpu(), torch.tensor(fills, dtype=I32))             # cache_seqlens is not modified
        for name, got, w in zip(("k_cache", "v_cache", "k_scale", "v_scale"), pools, want):
            assert same_bits(got, w), (name, n, int((bits(got) != bits(w)).sum()))
        # attention sees the new keys: the bits of the next step's call over the pools as the append left them, held to fp64
        if form == "paged":
            assert finite((o, lse)) and tk.same((o, lse), nxt), n
            held("append n=%d" % n, q, o, lse, tk.truth(q, K, V, after, True), after)
        else:
            for b, (got, nx) in enumerate(zip(res, nxt)):
                if S[b]:
                    assert finite(got) and tk.same(got, nx), (n, b)
                    held("packed append n=%d b=%d" % (n, b), st.q_seq[b], *got,
                         tk.truth(st.q_seq[b], K[b:b + 1], V[b:b + 1], [after[b]], True), [after[b]])


# ---- 7. table entries outside the pools, guarded -----------------------------------------------------------------------------
def guarded(pool):
    """(big, view): the pool as pages [GUARD, GUARD + num_pages) of a new allocation whose other pages are 0xFF bytes (the
    caches) or NaN (the scales) throughout"""
    n = pool.shape[0]
    big = torch.empty(n + 2 * GUARD, *pool.shape[1:], dtype=pool.dtype, device=pool.device)
    if pool.element_size() == 1:
        bits(big).fill_(FF)
    else:
        big.fill_(float("nan"))
    bits(big)[GUARD:GUARD + n] = bits(pool)
    return big, big[GUARD:GUARD + n]


def guards_intact(big):
    fresh = guarded(big[:0])[0]                                                    # 2 * GUARD pages of the fill
    return same_bits(big[:GUARD], fresh[:GUARD]) and same_bits(big[big.shape[0] - GUARD:], fresh[GUARD:])


OUT_OF_RANGE = [("paged", 64, F16), ("paged", 128, BF16), ("packed", 64, BF16), ("packed", 128, F16), ("packed", 256, BF16)]


@pytest.mark.parametrize("form,D,dtype", OUT_OF_RANGE, ids=["%s-d%d-%s" % (f, D, _name[dt]) for f, D, dt in OUT_OF_RANGE])
def test_out_of_range_entries_read_as_empty_pages_and_drop_their_rows(form, D, dtype):
    """Why this cannot fault: page_desc gives an entry outside [0, num_pages) four descriptors of 0 bytes at the pools' own
    bases -- the two of the cache pools and the two of the scale pools; every buffer load through them returns 0, so the page
    reads as keys and values of 0 with scales of 0 --, the append's paged_dst returns false before any store of bytes or of a
    scale, and the binding does not read the table.  Were any of these checks missing, page * stride for these entries still
    lands in a guard page of the same allocation, of the caches (0xFF) and of the scales (NaN) alike."""
    page, mp, H, Hkv = 96, 15, 8, 2
    h, NG = mp // 2, 2 if D == 256 else 4
    packed = form == "packed"
    S = [1, 3, 40, 3, 9] if packed else [3] * 5
    # sequences 1 and 3 get the bad entries; their appends start one row before the boundary of the pages h and mp - 1
    lens = [h * page + 33, h * page - 1, 33, (mp - 1) * page - 1, page * mp - 40]
    full = [L + s for L, s in zip(lens, S)]
    where = out_of_range_positions(page, mp)
    pages_of = lambda L: -(-L // page)
    assert all(i < pages_of(lens[b]) or i == pages_of(full[b]) - 1 for b, i in where)
    # looked up inside a wave's loop: at one split the entry of a tile t >= 3 NG comes from the loop's page_of(t + 3 NG)
    assert sum(i * (page // 32) >= 3 * NG for _, i in where) >= 4
    st = Step(page, mp, D, dtype, H, Hkv, seed=91, S=S, lens=lens, owned=full)
    c = st.c
    NP = c.NP
    bad_entries = [-1, -GUARD, NP, NP + GUARD - 1]                        # guard pages of the same allocation, nothing outside it
    bad, lost = c.table.clone(), []
    for k, (b, i) in enumerate(where):
        lost.append(int(bad[b, i]))
        bad[b, i] = bad_entries[k % 4]
    assert all(-GUARD <= int(bad[b, i]) < NP + GUARD and not 0 <= int(bad[b, i]) < NP for b, i in where)
    q = None if packed else torch.cat(st.q_seq)
    kn_b, vn_b = new_rows(len(S), Hkv, max(S), D, dtype, 92)
    kn_s, vn_s = ([x[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)] for x in (kn_b, vn_b))

    def run(table, pools, append=False, **kw):
        if packed:
            return st.ragged(table, pools, k_new=kn_s if append else None, v_new=vn_s if append else None, **kw)
        o, lse = tk.paged(q, *pools, c.sl, table, k_new=kn_b if append else None, v_new=vn_b if append else None, **kw)
        return [(o[b:b + 1], lse[b:b + 1]) for b in range(len(S))]

    def compare(got, clean, what):
        for b, (g, r) in enumerate(zip(got, clean)):
            if b in (1, 3):                                                # an empty page reads as zeros: no NaN scale
                assert finite(g), (what, b)
            else:
                assert tk.same(g, r), (what, b)

    bigs, views = zip(*(guarded(p) for p in c.pools))
    assert all(v.data_ptr() == b[GUARD].data_ptr() and v.is_contiguous() and v.shape[0] == NP for b, v in zip(bigs, views))
    for n in (1, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            compare(run(bad, views, **kw), run(c.table, views, **kw), (n, is_causal, window))
        assert all(guards_intact(b) for b in bigs) and all(same_bits(v, p) for v, p in zip(views, c.pools))
        # the append: through the clean table, then through the bad one into a second set of guarded copies
        cb, cv = zip(*(guarded(p) for p in c.pools))
        bb, bv = zip(*(guarded(p) for p in c.pools))
        clean = run(c.table, cv, append=True, is_causal=True)
        got = run(bad, bv, append=True, is_causal=True)
        torch.cuda.synchronize()
        compare(got, clean, ("append", n))
        assert all(guards_intact(b) for b in cb + bb), n
        # the rows bound for a replaced page are dropped -- that page keeps every bit -- and every other row is where the
        # clean append put it; every page no sequence names keeps every bit (the whole pools are compared)
        for name, p, x, y in zip(("k_cache", "v_cache", "k_scale", "v_scale"), c.pools, cv, bv):
            want = x.clone()
            bits(want)[lost] = bits(p)[lost]
            assert not same_bits(want, x) and not same_bits(x, p), (name, n)       # rows were dropped, rows were written
            assert same_bits(y, want), (name, n, int((bits(y) != bits(want)).sum()))
            assert torch.equal(bits(x)[c.spare], bits(p)[c.spare]) and torch.equal(bits(y)[c.spare], bits(p)[c.spare]), (name, n)


def out_of_range_positions(page, mp):
    """test 7's (sequence, table position) pairs: the first page, both sides of the middle of the table and its last page"""
    h = mp // 2
    return [(1, 0), (1, h - 1), (1, h), (3, 1), (3, mp - 1), (3, h)]


# ---- 8. the soft-capped per-token kernels, deep ------------------------------------------------------------------------------
CAPPED = [(32, 44, 64, F16), (160, 9, 128, BF16), (224, 7, 64, BF16)]             # (page 96: test_gpu_kvcache_quant_softcap.py)
CAPPED_SQS, CAPPED_GROUPS = (3, 40), [(8, 2), (8, 1)]
CAPPED_PACKED = [(96, 15, 256, BF16), (224, 7, 128, F16)]


@pytest.mark.parametrize("page,mp,D,dtype", CAPPED, ids=_id(CAPPED))
def test_deep_capped_paged_call_has_the_bits_of_the_padded_call_and_holds_to_fp64(page, mp, D, dtype):
    lens = lengths(page, mp)
    sl = qc.sl_of(lens)
    for H, Hkv in CAPPED_GROUPS:
        for Sq in CAPPED_SQS:
            q, c = qc.make("token", len(lens), H, Hkv, Sq, page * mp, D, dtype, CAP, seed=D + Sq + Hkv)
            pools, table = qc.scatter(c, lens, page, mp, seed=9)
            flat = qc.gather(pools, table)
            for is_causal, window in MASKS:
                gt = qc.truth(q, c, lens, CAP, is_causal, window)
                for n in PACKED_SPLITS:
                    vck.splits(n)
                    what = "capped p%d d%d %s" % (page, D, (H, Hkv, Sq, is_causal, window, n))
                    o, lse = qc.paged(q, pools, sl, table, CAP, is_causal=is_causal, window_size=window)
                    assert finite((o, lse)), what
                    assert qc.same((o, lse), qc.padded(q, flat, sl, CAP, is_causal=is_causal, window_size=window)), what
                    qc.check(what, q, o, lse, gt, lens, matters=window == (-1, -1))


@pytest.mark.parametrize("page,mp,D,dtype", CAPPED_PACKED, ids=_id(CAPPED_PACKED))
def test_deep_capped_packed_rows_have_the_bits_of_the_sequence_alone(page, mp, D, dtype):
    lens, S = packed_lens(page, mp), S_PACKED
    sl = qc.sl_of(lens)
    for H, Hkv in CAPPED_GROUPS:
        q, c = qc.make("token", len(lens), H, Hkv, max(S), page * mp, D, dtype, CAP, seed=D + Hkv)
        qs = [q[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)]
        pools, table = qc.scatter(c, lens, page, mp, seed=9)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            gts = [None if s == 0 else qc.truth(qs[b], c.rows(b, lens[b]), [lens[b]], CAP, is_causal, window) for b, s in enumerate(S)]
            for n in PACKED_SPLITS:
                vck.splits(n)
                res = qc.packed(qs, pools, sl, table, CAP, total_q=sum(S) + PAD, **kw)
                for b, (got, s) in enumerate(zip(res, S)):
                    if s == 0:
                        continue
                    what = "capped packed p%d d%d %s" % (page, D, (H, Hkv, is_causal, window, n, b))
                    if D == 256:
                        one = qc.packed([qs[b]], pools, sl[b:b + 1], table[b:b + 1], CAP, **kw)[0]
                    else:
                        one = qc.paged(qs[b], pools, sl[b:b + 1], table[b:b + 1], CAP, **kw)
                    assert finite(got) and qc.same(got, one), what
                    qc.check(what, qs[b], *got, gts[b], [lens[b]], matters=window == (-1, -1))
