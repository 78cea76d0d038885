"""GPU tests of MXFP4 decoding over DEEP block tables and long padded caches (fa_decode_mod_kernel's KV4 forms, padded, paged
and packed, and the quantising appends; include/mi355fa_kvcache_fp4.h, include/mi355fa_ragged_fp4.h).

tests/test_gpu_kvcache_fp4.py and tests/test_gpu_ragged_fp4.py stop at 7 tiles (one paged case at 9): there a wave runs 2 to
4 loop steps, so the lookup pipeline of csrc/fa_decode_body.inc (table entry three steps ahead, descriptors two, loads one)
runs its prologue only -- and with KV4 that pipeline also carries two scale-pool descriptors and two scale offsets over the
loop's back edge.  The geometries below are those of tests/test_gpu_paged_deep.py, 44 to 49 tiles with 1, 3, 4, 5 and 7 tiles
per page: waves of up to 12 steps (22 at D = 256, where a workgroup takes two tiles a step), the multiply path of FastDiv,
windows and splits that begin many pages into a table and mid-page, and padded caches of 1408 to 1568 rows.
tests/test_host_fp4_deep.py holds the CPU model of the body's arithmetic over THIS module's constants and fails if the shapes
are shrunk below that reach.

  1. the bits of the padded MXFP4 call on the gathered cache: every geometry, head group, S_q, mask, split count, sinks or not
  2. fp64 (tests/attn_ref.py on the dequantised cache) per (sequence, head), the padded and the paged call; the empty sequence
     is O = 0 and LSE = -inf, or the sink's logit
  3. the block table as a strided view of a wider tensor
  4. packed queries at D = 64 and 128: the rows of a sequence have the bits of the paged call on it alone; fp64 per (sequence, head)
  5. packed queries at D = 256 (no rectangular sibling): the bits of the packed call on the sequence alone; fp64 likewise
  6. appends deep in the table, paged and packed: the four pools afterwards are the old bytes with quantize_kv_mxfp4's CPU
     result in exactly the appended rows
  7. table entries outside [0, num_pages) at positions a wave looks up inside its loop.  The four pools are the middle of
     larger 0xFF-filled (NaN-scale) allocations and the bad entries name guard pages of the same allocation only, so this is
     defined behaviour, never a fault: page_desc gives such an entry descriptors of 0 bytes at the pools' own bases and
     paged_dst drops the row before any store

Inputs are test_gpu_kvcache_fp4.make4's: random nibbles, scale bytes 127 +- 6 per (row, block), scattered under a permuted
table, every byte no sequence owns 0xFF.  The conversions are exact for these scales, so the error is the 16-bit kernel's, and
the bounds are the project's own per (sequence, head): relative Frobenius 1e-3 (fp16) / 8e-3 (bf16), LSE by check_lse.
Measured on an MI355X (profiles/fp4_deep_errors.jsonl, written by this module when MI355FA_FP4_DEEP_ERRORS names a file), the
worst (sequence, head) over every case:
  fp16: padded 5.3e-4, paged 5.3e-4, packed 4.9e-4   (bound 1e-3)
  bf16: padded 4.0e-3, paged 4.0e-3, packed 3.2e-3   (bound 8e-3)
Run on its own the module takes about 27 s on an MI355X (94 cases; the slowest 2.3 s, the first, which warms the device up,
every other below 0.5 s).  Shapes are the smallest that reach each path."""
import json
import os

import pytest
import torch

import fa_oracle as fo
import raggedcheck as rg
import variantcheck as vck
import test_gpu_kvcache_fp4 as t4
import test_gpu_paged_deep as deep
from test_gpu_kvcache_fp4 import BF16, BOUND, F16, FF

pytestmark = pytest.mark.gpu

GEOMS = [(32, 44), (96, 15), (128, 11), (160, 9), (224, 7)]    # (page_size, max_pages): 44 to 49 tiles; 1, 3, 4, 5, 7 a page
SPLITS = (0, 1, 2, 3, 5, 11)                # 0: the formula
MASKS = t4.MASKS + [(False, (300, 8)), (True, (700, -1))]      # + two that begin mid-table (mid-page at 3, 5, 7 tiles a page)
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


def _F():
    import fp4_kvcache as F
    return F


def _R():
    import fp4_ragged_kvcache as R
    return R


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def record(test, dtype, D, page, mp, sink, worst):
    """one line of profiles/fp4_deep_errors.jsonl: appended to the file MI355FA_FP4_DEEP_ERRORS names, if any"""
    path = os.environ.get("MI355FA_FP4_DEEP_ERRORS")
    line = dict(test=test, dtype=_name[dtype], D=D, page_size=page, max_pages=mp, sinks=sink, worst_per_head_rel=worst,
                bound=BOUND[dtype])
    print(json.dumps(line))
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


# ---- the caches: built once per (geometry, format, H_kv, fill levels), shared by the tests and never written ----------------
class Cache:
    """pad: the four padded byte tensors [B, H_kv, page * mp, .], 0xFF at and past L_b; pools / table: the same rows under a
    permuted table with pages for owned[b] >= L_b rows, every byte no sequence owns 0xFF; K, V: the dequantised cache in fp64"""

    def __init__(self, page, mp, D, dtype, Hkv, lens, owned, seed):
        B = len(lens)
        _, kc, vc, ks, vs = t4.make4(B, Hkv, Hkv, 1, page * mp, D, dtype, seed=seed)
        self.pad = [kc, vc, ks, vs]
        for b, L in enumerate(lens):
            for t in self.pad:
                t[b, :, L:] = FF
        self.lens, self.owned, self.page, self.mp = list(lens), list(owned), page, mp
        self.NP = sum(-(-L // page) for L in owned) + 4
        self.pools, self.table = t4.scatter4(self.pad, self.owned, page, self.NP, mp, seed=seed + 1)
        self._kv = None
        self.sl = torch.tensor(self.lens, dtype=torch.int32, device="cuda")

    def _deq(self):
        if self._kv is None:
            self._kv = t4.deq64(self.pad[0], self.pad[2]), t4.deq64(self.pad[1], self.pad[3])
        return self._kv

    K = property(lambda self: self._deq()[0])
    V = property(lambda self: self._deq()[1])


_CACHES = {}                                # the last few, so that a case's loops and its neighbours share one


def cache(page, mp, D, dtype, Hkv, lens=None, owned=None, seed=0):
    lens = tuple(lengths(page, mp) if lens is None else lens)
    owned = lens if owned is None else tuple(owned)
    key = (page, mp, D, dtype, Hkv, lens, owned, seed)
    if key not in _CACHES:
        while len(_CACHES) >= 8:
            del _CACHES[next(iter(_CACHES))]
        _CACHES[key] = Cache(page, mp, D, dtype, Hkv, lens, owned, seed + page + D + Hkv)
    return _CACHES[key]


def queries(B, H, Sq, D, dtype, seed):
    """make4's q: scaled so that the scores stay of order one"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(B, H, Sq, D, generator=g, device="cuda") * 0.03).to(dtype)


def sinks_of(H):
    return torch.linspace(-1.0, 3.0, H, device="cuda", dtype=torch.float32)


def gather4(pool, table):
    """the padded byte tensor [B, H_kv, max_pages * page, w] a pool and a table describe"""
    B, mp = table.shape
    out = pool[table.long()]                                   # [B, max_pages, H_kv, page, w]
    return out.permute(0, 2, 1, 3, 4).reshape(B, pool.shape[1], mp * pool.shape[2], pool.shape[3]).contiguous()


def truth(q, K, V, lens, wl, wr, sinks):
    """test_gpu_kvcache_fp4.truth per sequence; the empty sequence directly: O = 0 and LSE = -inf, or the sink's logit"""
    B, H, Sq, D = q.shape
    O = torch.zeros(B, H, Sq, D, dtype=torch.float64, device=q.device)
    LSE = torch.full((B, H, Sq), float("-inf"), dtype=torch.float64, device=q.device)
    for b, L in enumerate(lens):
        if L == 0:
            if sinks is not None:
                LSE[b] = sinks.double()[:, None].expand(H, Sq)
            continue
        o, lse = t4.truth(q[b:b + 1], K[b:b + 1], V[b:b + 1], [L], wl, wr, sinks)
        O[b], LSE[b] = o[0], lse[0]
    return O, LSE


def held(tag, q, o, lse, ref):
    """test_gpu_kvcache_fp4.check, rows without a key exactly 0; returns the worst (sequence, head) error"""
    t4.check(tag, q, o, lse, *ref)
    assert (o[(ref[0] == 0).all(-1)] == 0).all(), tag
    return float(fo.block_errors(ref[0], o, block=q.shape[2]).max())


# ---- 1. the bits of the padded call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sink", SINKS, ids=SINK_IDS)
@pytest.mark.parametrize("page,mp,D,dtype", CONFIGS, ids=_id(CONFIGS))
def test_deep_paged_call_has_the_bits_of_the_padded_call(page, mp, D, dtype, sink):
    F = _F()
    for H, Hkv in GROUPS:
        c = cache(page, mp, D, dtype, Hkv)
        sk = sinks_of(H) if sink else None
        table = t4.wide(c.table) if Hkv == 2 else c.table
        for Sq in SQS:
            q = queries(len(c.lens), H, Sq, D, dtype, seed=D + Sq + H + page)
            for is_causal, window in MASKS:
                kw = dict(is_causal=is_causal, window_size=window, return_lse=True, sinks=sk)
                for n in SPLITS:
                    vck.splits(n)
                    what = (H, Hkv, Sq, is_causal, window, n)
                    ref = F.flash_attention_kvcache_fp4(q, *c.pad, c.sl, **kw)
                    got = F.flash_attention_kvcache_fp4_paged(q, *c.pools, c.sl, table, **kw)
                    assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), what
                    assert t4.same(got, ref), what


# ---- 2. fp64 on its own, per (sequence, head) --------------------------------------------------------------------------------
@pytest.mark.parametrize("sink", SINKS, ids=SINK_IDS)
@pytest.mark.parametrize("call", ["padded", "paged"])
@pytest.mark.parametrize("page,mp,D,dtype", CONFIGS, ids=_id(CONFIGS))
def test_every_sequence_and_head_matches_fp64(page, mp, D, dtype, call, sink):
    F = _F()
    worst = 0.0
    for H, Hkv in GROUPS:
        c = cache(page, mp, D, dtype, Hkv)
        sk = sinks_of(H) if sink else None
        for Sq in SQS:
            q = queries(len(c.lens), H, Sq, D, dtype, seed=7 + D + Sq + H + page)
            for is_causal, window in MASKS:
                kw = dict(is_causal=is_causal, window_size=window, return_lse=True, sinks=sk)
                ref = truth(q, c.K, c.V, c.lens, *t4.window_of(is_causal, window), sk)     # once per mask, shared by the splits
                for n in SPLITS:
                    vck.splits(n)
                    if call == "padded":
                        o, lse = F.flash_attention_kvcache_fp4(q, *c.pad, c.sl, **kw)
                    else:
                        o, lse = F.flash_attention_kvcache_fp4_paged(q, *c.pools, c.sl, c.table, **kw)
                    worst = max(worst, held("%s %s" % (call, (H, Hkv, Sq, is_causal, window, n)), q, o, lse, ref))
    record(call, dtype, D, page, mp, sink, worst)


# ---- 3. the table as a view --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page,mp", [(32, 44), (96, 15)])
def test_table_as_a_strided_view_of_a_wider_tensor(page, mp):
    F, R = _F(), _R()
    D, H, Hkv, Sq, Snew, dtype = 128, 8, 2, 3, 3, BF16
    lens = [min(L, page * mp - Snew) for L in lengths(page, mp)]          # room for the append
    c = cache(page, mp, D, dtype, Hkv, lens, [L + Snew for L in lens], seed=33)
    w = t4.wide(c.table)
    assert w.stride(0) == mp + 7 > w.shape[1] and w.stride(1) == 1 and torch.equal(w, c.table) and not w.is_contiguous()
    assert w.data_ptr() % 16 == 12
    q = queries(len(lens), H, Sq, D, dtype, seed=34)
    kn, vn = t4.append_inputs(len(lens), Hkv, Snew, D, dtype, 35)
    for n in (1, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window, return_lse=True)
            got = F.flash_attention_kvcache_fp4_paged(q, *c.pools, c.sl, w, **kw)
            assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), (n, is_causal, window)
            assert t4.same(got, F.flash_attention_kvcache_fp4_paged(q, *c.pools, c.sl, c.table, **kw)), (n, is_causal, window)
        p1, p2 = [t.clone() for t in c.pools], [t.clone() for t in c.pools]
        kw = dict(k_new=kn, v_new=vn, is_causal=True, return_lse=True)
        a = F.flash_attention_kvcache_fp4_paged(q, *p1, c.sl, c.table, **kw)
        b = F.flash_attention_kvcache_fp4_paged(q, *p2, c.sl, w, **kw)
        assert t4.same(b, a) and torch.isfinite(b[0]).all(), ("append", n)
        assert all(torch.equal(x, y) for x, y in zip(p1, p2)) and not torch.equal(p1[2], c.pools[2]), n
        # one sequence alone (B = 1: the call passes max_pages as the stride), the base still 12 bytes off
        for s in (4, 8):
            one = F.flash_attention_kvcache_fp4_paged(q[s:s + 1], *c.pools, c.sl[s:s + 1], w[s:s + 1], is_causal=True, return_lse=True)
            ref = F.flash_attention_kvcache_fp4_paged(q[s:s + 1], *c.pools, c.sl[s:s + 1], c.table[s:s + 1].contiguous(),
                                                      is_causal=True, return_lse=True)
            assert w[s:s + 1].data_ptr() % 16 != 0 and t4.same(one, ref), ("B = 1", n, s)
    # the packed call
    st = Step(page, mp, D, dtype, H, Hkv, seed=36)
    sw = t4.wide(st.c.table)
    for n in (1, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            a, b = st.ragged(st.c.table, **kw), st.ragged(sw, **kw)
            assert torch.isfinite(b[0][:st.rows]).all() and not torch.isnan(b[1][:, :st.rows]).any(), (n, is_causal, window)
            assert t4.same((a[0][:st.rows], a[1][:, :st.rows]), (b[0][:st.rows], b[1][:, :st.rows])), (n, is_causal, window)


# ---- 4, 5. packed queries over deep tables -----------------------------------------------------------------------------------
class Step:
    """one packed step over a deep table: S_PACKED's query counts (or `S`) over packed_lens' fill levels (or `lens`)"""

    def __init__(self, page, mp, D, dtype, H, Hkv, seed, S=None, lens=None, owned=None):
        self.S = list(S_PACKED if S is None else S)
        self.c = cache(page, mp, D, dtype, Hkv, packed_lens(page, mp) if lens is None else lens, owned, seed=seed)
        assert len(self.c.lens) == len(self.S)
        self.rows, self.tq = sum(self.S), sum(self.S) + PAD
        qb = queries(len(self.S), H, max(self.S), D, dtype, seed=seed + 3)
        self.q_seq = [qb[b:b + 1, :, :s].contiguous() for b, s in enumerate(self.S)]
        self.q = rg.pack(self.q_seq, self.tq, fill=0.0)
        self.cu = rg.cu_of(self.S, device="cuda")

    def ragged(self, table, pools=None, **kw):
        return _R().flash_attention_kvcache_fp4_ragged(self.q, *(self.c.pools if pools is None else pools), self.cu, self.c.sl,
                                                       table, return_lse=True, **kw)

    def alone(self, b, pools=None, k_new=None, v_new=None, **kw):
        """(O [1, H, S_b, D], LSE [1, H, S_b]) of sequence b on its own: the paged call at D <= 128, the packed call with
        B = 1 at D = 256, which has no rectangular sibling"""
        c, pools = self.c, self.c.pools if pools is None else pools
        if self.q.shape[-1] == 256:
            flat = lambda t: None if t is None else t[0].transpose(0, 1).contiguous()
            o, lse = _R().flash_attention_kvcache_fp4_ragged(flat(self.q_seq[b]), *pools, rg.cu_of([self.S[b]], device="cuda"),
                                                             c.sl[b:b + 1], c.table[b:b + 1], return_lse=True,
                                                             k_new=flat(k_new), v_new=flat(v_new), **kw)
            return o.transpose(0, 1)[None].contiguous(), lse[None].contiguous()
        return _F().flash_attention_kvcache_fp4_paged(self.q_seq[b], *pools, c.sl[b:b + 1], c.table[b:b + 1], return_lse=True,
                                                      k_new=k_new, v_new=v_new, **kw)


def _packed(page, mp, D, dtype, sink):
    worst = 0.0
    for H, Hkv in GROUPS:
        st = Step(page, mp, D, dtype, H, Hkv, seed=D + H)
        c = st.c
        sk = sinks_of(H) if sink else None
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window, sinks=sk)
            wl, wr = t4.window_of(is_causal, window)
            refs64 = [None if s == 0 else t4.truth(st.q_seq[b], c.K[b:b + 1], c.V[b:b + 1], [c.lens[b]], wl, wr, sk)
                      for b, s in enumerate(st.S)]                          # fp64 per sequence, once per mask
            for n in PACKED_SPLITS:
                vck.splits(n)
                what = (H, Hkv, is_causal, window, n)
                o, lse = st.ragged(c.table, **kw)
                assert torch.isfinite(o[:st.rows]).all() and not torch.isnan(lse[:, :st.rows]).any(), what
                ob, lb = rg.unpack(o, st.S), rg.unpack_lse(lse, st.S)
                for b, s in enumerate(st.S):
                    if s:
                        assert t4.same((ob[b], lb[b]), st.alone(b, **kw)), what + (b,)
                        worst = max(worst, held("packed %s b=%d" % (what, b), st.q_seq[b], ob[b], lb[b], refs64[b]))
    record("packed", dtype, D, page, mp, sink, worst)


@pytest.mark.parametrize("sink", SINKS, ids=SINK_IDS)
@pytest.mark.parametrize("page,mp,D,dtype", PACKED_GEOMS, ids=_id(PACKED_GEOMS))
def test_deep_packed_rows_have_the_bits_of_the_paged_call_on_each_sequence(page, mp, D, dtype, sink):
    _packed(page, mp, D, dtype, sink)


@pytest.mark.parametrize("sink", SINKS, ids=SINK_IDS)
@pytest.mark.parametrize("page,mp,D,dtype", PACKED_256, ids=_id(PACKED_256))
def test_deep_d256_rows_have_the_bits_of_the_sequence_alone(page, mp, D, dtype, sink):
    """NG is 2 here: the odd and empty shares of a wave pair, which only join the barrier, occur many pages deep"""
    _packed(page, mp, D, dtype, sink)


# ---- 6. appends deep in the table --------------------------------------------------------------------------------------------
_APPEND = [(96, 15, 64, F16), (128, 11, 128, BF16), (160, 9, 64, BF16)]
APPEND_CONFIGS = [(form,) + c for form in ("paged", "packed") for c in _APPEND] + [("packed", 96, 15, 256, F16)]   # D = 256: packed only


def appended(pools, table, page, fills, new):
    """the pools with quantize_kv_mxfp4's CPU bytes of new[b] = (k_new, v_new) [1, H_kv, S_b, D] in the rows
    [fills[b], fills[b] + S_b) of sequence b, through the table; every other byte as it was"""
    F = _F()
    want = [t.clone() for t in pools]
    tab = table.cpu()
    for b, (kn, vn) in enumerate(new):
        if kn.shape[2] == 0:
            continue
        (kq, kqs), (vq, vqs) = F.quantize_kv_mxfp4(kn.cpu()), F.quantize_kv_mxfp4(vn.cpu())
        for i in range(kn.shape[2]):
            row = fills[b] + i
            pg, r = int(tab[b, row // page]), row % page
            for t, x in zip(want, (kq, vq, kqs, vqs)):
                t[pg, :, r] = x[0, :, i].cuda()
    return want


@pytest.mark.parametrize("form,page,mp,D,dtype", APPEND_CONFIGS, ids=[c[0] + "-" + i for c, i in zip(APPEND_CONFIGS, _id(c[1:] for c in APPEND_CONFIGS))])
def test_append_deep_in_the_table_writes_exactly_the_quantised_rows(form, page, mp, D, dtype):
    """rows [L, L + S_new) that cross a page boundary in the table's second half, and that end at its reach"""
    F = _F()
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
    kn_b, vn_b = t4.append_inputs(len(S), Hkv, max(S), D, dtype, 62)
    new = [(kn_b[b:b + 1, :, :s].contiguous(), vn_b[b:b + 1, :, :s].contiguous()) for b, s in enumerate(S)]
    want = appended(c.pools, c.table, page, fills, new)
    assert not torch.equal(want[0], c.pools[0]) and not torch.equal(want[2], c.pools[2])
    full = torch.tensor(after, dtype=torch.int32, device="cuda")
    for n in (0, 3):
        vck.splits(n)
        pools = [t.clone() for t in c.pools]
        if form == "paged":
            q = torch.cat(st.q_seq)
            o, lse = F.flash_attention_kvcache_fp4_paged(q, *pools, c.sl, c.table, k_new=kn_b, v_new=vn_b, is_causal=True,
                                                         return_lse=True)
            nxt = F.flash_attention_kvcache_fp4_paged(q, *want, full, c.table, is_causal=True, return_lse=True)
        else:
            kn, vn = (rg.pack([x[i] for x in new], st.tq, fill=7.0) for i in (0, 1))   # (the padding rows: real values, dropped)
            o, lse = st.ragged(c.table, pools, k_new=kn, v_new=vn, is_causal=True)
            nxt = _R().flash_attention_kvcache_fp4_ragged(st.q, *want, st.cu, full, c.table, is_causal=True, return_lse=True)
            o, lse, nxt = o[:st.rows], lse[:, :st.rows], (nxt[0][:st.rows], nxt[1][:, :st.rows])
        torch.cuda.synchronize()
        assert torch.equal(c.sl.cpu(), torch.tensor(fills, dtype=torch.int32))       # cache_seqlens is not modified
        for name, got, w in zip(("k_cache", "v_cache", "k_scale", "v_scale"), pools, want):
            assert torch.equal(got, w), (name, n, int((got != w).sum()))
        # attention sees the new keys: the bits of the next step's call over the pools as the append left them, held to fp64
        assert torch.isfinite(o).all() and t4.same((o, lse), nxt), n
        K, V = t4.deq64(gather4(want[0], c.table), gather4(want[2], c.table)), t4.deq64(gather4(want[1], c.table), gather4(want[3], c.table))
        if form == "paged":
            held("append n=%d" % n, q, o, lse, truth(q, K, V, after, -1, 0, None))
        else:
            for b, (ob, lb) in enumerate(zip(rg.unpack(o, S), rg.unpack_lse(lse, S))):
                if S[b]:
                    held("packed append n=%d b=%d" % (n, b), st.q_seq[b], ob, lb,
                         t4.truth(st.q_seq[b], K[b:b + 1], V[b:b + 1], [after[b]], -1, 0))


# ---- 7. table entries outside the pools, guarded -----------------------------------------------------------------------------
def guarded(pool):
    """(big, view): the pool as pages [GUARD, GUARD + num_pages) of a new allocation whose other pages are 0xFF throughout"""
    n = pool.shape[0]
    big = torch.full((n + 2 * GUARD, *pool.shape[1:]), FF, dtype=torch.uint8, device=pool.device)
    big[GUARD:GUARD + n] = pool
    return big, big[GUARD:GUARD + n]


def guards_intact(big):
    return bool((big[:GUARD] == FF).all() and (big[big.shape[0] - GUARD:] == FF).all())


OUT_OF_RANGE = [("paged", 64, F16), ("paged", 128, BF16), ("packed", 64, BF16), ("packed", 128, F16), ("packed", 256, BF16)]


@pytest.mark.parametrize("form,D,dtype", OUT_OF_RANGE, ids=["%s-d%d-%s" % (f, D, _name[dt]) for f, D, dt in OUT_OF_RANGE])
def test_out_of_range_entries_read_as_empty_pages_and_drop_their_rows(form, D, dtype):
    """Why this cannot fault: page_desc gives an entry outside [0, num_pages) four descriptors of 0 bytes at the pools' own
    bases (every buffer load through them returns 0), paged_dst returns false before any store, and the binding does not read
    the table.  Were either check missing, page * stride for these entries still lands in a guard page of the same allocation."""
    F = _F()
    page, mp, H, Hkv = 96, 15, 8, 2
    h, NG = mp // 2, 2 if D == 256 else 4
    packed = form == "packed"
    S = [1, 3, 40, 3, 9] if packed else [3] * 5
    # sequences 1 and 3 get the bad entries; their appends start one row before the boundary of the pages h and mp - 1
    lens = [h * page + 33, h * page - 1, 33, (mp - 1) * page - 1, page * mp - 40]
    full = [L + s for L, s in zip(lens, S)]
    where = [(1, 0), (1, h - 1), (1, h), (3, 1), (3, mp - 1), (3, h)]
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

    def run(table, pools, **kw):
        if packed:
            o, lse = st.ragged(table, pools, **kw)
            return list(zip(rg.unpack(o, S), rg.unpack_lse(lse, S)))
        o, lse = F.flash_attention_kvcache_fp4_paged(q, *pools, c.sl, table, return_lse=True, **kw)
        return [(o[b], lse[b]) for b in range(len(S))]

    def compare(got, clean, what):
        for b, ((o, lse), (ro, rl)) in enumerate(zip(got, clean)):
            if b in (1, 3):                                                # an empty page reads as zeros: no 0xFF scale
                assert torch.isfinite(o).all() and not torch.isnan(lse).any(), (what, b)
            else:
                assert t4.same((o, lse), (ro, rl)), (what, b)

    kn_b, vn_b = t4.append_inputs(len(S), Hkv, max(S), D, dtype, 92)
    if packed:
        kn, vn = (rg.pack([x[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)], st.tq, fill=0.0) for x in (kn_b, vn_b))
    else:
        kn, vn = kn_b, vn_b
    bigs, views = zip(*(guarded(p) for p in c.pools))
    assert all(v.data_ptr() == b[GUARD].data_ptr() and v.is_contiguous() and v.shape[0] == NP for b, v in zip(bigs, views))
    for n in (1, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            kw = dict(is_causal=is_causal, window_size=window)
            compare(run(bad, views, **kw), run(c.table, views, **kw), (n, is_causal, window))
        assert all(guards_intact(b) for b in bigs) and all(torch.equal(v, p) for v, p in zip(views, c.pools))
        # the append: through the clean table, then through the bad one into a second set of guarded copies
        cb, cv = zip(*(guarded(p) for p in c.pools))
        bb, bv = zip(*(guarded(p) for p in c.pools))
        clean = run(c.table, cv, k_new=kn, v_new=vn, is_causal=True)
        got = run(bad, bv, k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        compare(got, clean, ("append", n))
        assert all(guards_intact(b) for b in cb + bb), n
        # the rows bound for a replaced page are dropped -- that page keeps every byte -- and every other row is where the
        # clean append put it; every page no sequence names keeps every byte (the whole pools are compared)
        for name, p, x, y in zip(("k_cache", "v_cache", "k_scale", "v_scale"), c.pools, cv, bv):
            want = x.clone()
            want[lost] = p[lost]
            assert not torch.equal(want, x) and not torch.equal(x, p), (name, n)      # rows were dropped, rows were written
            assert torch.equal(y, want), (name, n, int((y != want).sum()))
