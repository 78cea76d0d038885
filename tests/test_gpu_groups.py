"""GPU tests of split-KV decoding at head groups that are no power of two and at more than one 32-row block, for every
instance of fa_decode_mod_kernel: plain, soft-cap, ALiBi, sinks, e4m3 caches and e4m3 caches with sinks.

The kernel's MFMA rows are the g * S_q (query, head) rows of one K/V head, query-major, cut into 32-row blocks
(fa_decode_body.inc): with g = 3, 5, 7 or 12 a block boundary cuts through one query's heads, and the block's tile
range, the lane's slope, the row's sink and the output address all rest on qrow / g arithmetic.  The geometries, fill
levels, windows, split counts and parameters are those of tests/groups_ref.py (each geometry asserts RB >= 2 and, where g
is no power of two, 32 % g != 0); the truth is the fp64 reference of tests/attn_ref.py on the cache the
kernel left behind, dequantised for the e4m3 kinds.  tests/test_host_groups.py checks on the CPU that the chosen cap,
slopes and sinks matter on these inputs; the same conditions are asserted here before the kernel's output is looked at.

Every launch: no NaN / Inf in O; LSE = -inf exactly on the rows without a key (= the sink within 1e-5 for the sink
kinds) and O = 0 there; the same bits on a repeated call; O per (batch, head) with fa_oracle.block_errors against the
project's per-(batch, head) decode bounds (1e-3 fp16, 8e-3 bf16: test_gpu_kvcache.py), the (batch, head) pairs that see
fewer than blockcheck.FEW keys also row by row against the same bound; LSE row by row within a + u * SABS with the kind's
own LSE_BOUND (plain and e4m3: test_gpu_blockwise.py's).  Window (0, 0) leaves a row its own-position key only: P = 1, so
O is that V row and LSE the score (plus the sink), and a mask off by one key is a gross error.

Grouped equals expanded, bit for bit (test_grouped_equals_expanded_bit_for_bit): with one split and window_left = -1 the
block's first tile is tile 0, tile t goes to wave t mod 4, a row's online softmax sees only its own scores and a tile
that is fully masked for a row leaves its (m, l, O) unchanged (corr = 1, p = 0; a wave that saw only such tiles merges
with weight 0), so a row's arithmetic does not depend on the block it sits in and H_kv = H on repeat_interleave'd K/V
gives the same bits.

Full cross product kinds x geometries x {fp16, bf16} x {64, 128}; nothing is thinned.  k_new / v_new (S_new = 2) are
appended on every second parametrisation.

Measured on an MI355X, the largest value over every geometry, head dim, window and split count as a fraction of its bound
(O: per-(batch, head) relFro / (1e-3 fp16, 8e-3 bf16); LSE: row error / (a + u SABS)); every parametrisation prints its
own "GROUPS ..." line:
    kind       fp16 O   fp16 LSE   bf16 O   bf16 LSE
    plain      0.321    0.010      0.326    < 0.001
    softcap    0.261    0.019      0.261    < 0.001
    alibi      0.296    0.005      0.298    < 0.001
    sink       0.336    0.004      0.338    < 0.001
    fp8        0.319    0.010      0.315    < 0.001
    fp8_sink   0.317    0.004      0.329    < 0.001
(the rounding of the 16-bit output alone gives O 0.22 - 0.31: the fp64 truth rounded to the dtype, on the CPU).  No case
needed the eager yardstick, and grouped equals expanded bit for bit in all 144 parametrisations."""
from types import SimpleNamespace

import pytest
import torch

import blockcheck as bc
import fa_oracle as fo
import groups_ref as gr
import variantcheck as vck
from test_gpu_alibi import BOUNDS as ALIBI_BOUNDS
from test_gpu_blockwise import LSE_BOUND as PLAIN_LSE_BOUND
from test_gpu_sink import BOUNDS as SINK_BOUNDS
from test_gpu_softcap import BOUNDS as SOFTCAP_BOUNDS
from variantcheck import formula_splits   # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

F16, BF16 = gr.F16, gr.BF16
O_BOUND = {F16: 1e-3, BF16: 8e-3}     # per (batch, head): test_gpu_kvcache.py, test_gpu_kvcache_fp8.py
LSE_BOUND = {"plain": PLAIN_LSE_BOUND, "fp8": PLAIN_LSE_BOUND, "softcap": SOFTCAP_BOUNDS["LSE_BOUND"],
             "alibi": ALIBI_BOUNDS["LSE_BOUND"], "sink": SINK_BOUNDS["LSE_BOUND"], "fp8_sink": SINK_BOUNDS["LSE_BOUND"]}
GEOM_IDS = [gr.geom_id(g) for g in gr.GEOMS]


def _M():
    import My_FlashAttention_optimized as M
    return M


def _call(c, window, q=None):
    """One decode call of c's kind on clones of its caches: (O, LSE, the K cache and the V cache it left behind)."""
    M = _M()
    k_, v_ = c.kc.clone(), c.vc.clone()
    q = c.q if q is None else q
    kw = dict(k_new=c.kn, v_new=c.vn, window_size=window, return_lse=True)
    if c.kind == "plain":
        o, lse = M.flash_attention_kvcache(q, k_, v_, c.sl, **kw)
    elif c.kind == "softcap":
        o, lse = M.flash_attention_kvcache_softcap(q, k_, v_, c.sl, gr.CAP, **kw)
    elif c.kind == "alibi":
        o, lse = M.flash_attention_kvcache_alibi(q, k_, v_, c.sl, c.slopes, **kw)
    elif c.kind == "sink":
        o, lse = M.flash_attention_kvcache_sink(q, k_, v_, c.sl, c.sinks, **kw)
    elif c.kind == "fp8":
        o, lse = M.flash_attention_kvcache_fp8(q, k_, v_, c.sl, c.kd, c.vd, **kw)
    else:
        o, lse = M.flash_attention_kvcache_fp8_sink(q, k_, v_, c.sl, c.sinks, c.kd, c.vd, **kw)
    torch.cuda.synchronize()
    return o, lse, k_, v_


def _expanded(c):
    """The same call with H_kv = H: K / V, the appended rows and the descales repeat_interleave'd by g."""
    g = c.geom[0] // c.geom[1]
    rep = lambda t: None if t is None else t.repeat_interleave(g, dim=1).contiguous()
    e = SimpleNamespace(**vars(c))
    e.kc, e.vc, e.kn, e.vn, e.kd, e.vd = (rep(t) for t in (c.kc, c.vc, c.kn, c.vn, c.kd, c.vd))
    return e


def _assert_geometry(geom):
    H, Hkv, Sq = geom
    g = H // Hkv
    assert -(-g * Sq // 32) >= 2, geom          # RB >= 2: a second row block
    if g & (g - 1):
        assert 32 % g != 0, geom                # the 32-row boundary cuts through a query's heads


def _check_launch(c, t, window, n, o, lse):
    """Every check of one launch against the truth t; returns (largest per-(batch, head) O error, largest LSE excess)."""
    kind, dtype = c.kind, c.dtype
    H, Hkv, Sq = c.geom
    where = lambda b, h: "%s b=%d h=%d window=%s splits=%d L_b=%d" % (kind, b, h, window, n, c.Ls[b])
    sink = kind.endswith("sink")
    nokey = t.nokey
    assert torch.isfinite(o).all(), (kind, window, n, "NaN / Inf in O")
    assert (o[nokey] == 0).all(), (kind, window, n, "O != 0 on a row without a key")
    if sink:
        assert torch.isfinite(lse).all(), (kind, window, n)
        z = c.sinks.double()[None, :, None].expand(gr.B, H, Sq)
        if nokey.any():
            assert (lse.double()[nokey] - z[nokey]).abs().max().item() <= 1e-5, (kind, window, n, "LSE != z without a key")
    else:
        assert torch.equal(torch.isneginf(lse), nokey), (kind, window, n, "LSE = -inf exactly on the rows without a key")
    # O per (batch, head)
    bound = O_BOUND[dtype]
    err = fo.block_errors(t.gt["O"], o, block=Sq)[..., 0]                          # [B, H]
    at = tuple(int(x) for x in torch.unravel_index(err.argmax(), err.shape))
    assert err[at] <= bound, "%s: O off by %.3e (bound %.1e)" % (where(*at), err[at].item(), bound)
    # the (batch, head) pairs whose rows see fewer than FEW keys in all: every row on its own
    nkeys = t.vis[:, 0].any(1).sum(-1)                                             # [B] distinct keys the rows see
    few = (nkeys > 0) & (nkeys < bc.FEW)
    if few.any():
        r = t.gt["O"][few]
        rerr = (o[few].double() - r).norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-300)
        rerr = torch.where(nokey[few], torch.zeros_like(rerr), rerr)
        at = tuple(int(x) for x in torch.unravel_index(rerr.argmax(), rerr.shape))
        b = int(few.nonzero()[at[0]])
        assert rerr[at] <= bound, "%s row %d: O off by %.3e (bound %.1e)" % (where(b, at[1]), at[2], rerr[at].item(), bound)
    # LSE row by row
    a, u = LSE_BOUND[kind][dtype]
    ref = t.gt["LSE"]
    fin = torch.isfinite(ref)
    lerr = torch.where(fin, (lse.double() - ref).abs(), torch.zeros_like(ref))
    lerr = torch.where(torch.isnan(lerr), float("inf"), lerr)
    excess = lerr / (a + u * t.gt["SABS"])
    at = tuple(int(x) for x in torch.unravel_index(excess.argmax(), excess.shape))
    assert excess[at] <= 1, "%s row %d: LSE off by %.3e (bound %.3e)" % (
        where(at[0], at[1]), at[2], lerr[at].item(), a + u * t.gt["SABS"][at].item())
    return err.max().item() / bound, excess.max().item()


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("gi", range(len(gr.GEOMS)), ids=GEOM_IDS)
@pytest.mark.parametrize("kind", gr.KINDS)
def test_decode_per_head_against_fp64(kind, gi, dtype, D, formula_splits):
    geom = gr.GEOMS[gi]
    _assert_geometry(geom)
    c = gr.make_case(kind, geom, dtype, D, gr.s_new(gi, dtype, D), "cuda")
    truths, worst_o, worst_l = None, 0.0, 0.0
    for window in gr.WINDOWS:
        for n in gr.SPLITS:
            vck.splits(n)
            o, lse, k_, v_ = _call(c, window)
            o2, lse2, _, _ = _call(c, window)
            assert bc.same_bits(o, o2) and bc.same_bits(lse, lse2), (kind, window, n, "a repeated call gave other bits")
            # the cache afterwards: the padded cache plus exactly the new rows
            assert torch.equal(gr._bits(k_), gr._bits(c.k_after)) and torch.equal(gr._bits(v_), gr._bits(c.v_after)), \
                (kind, window, n, "the cache after the call")
            if truths is None:   # fp64 on the cache the kernel left behind; the conditions on the reference come first
                truths = {w: gr.truth(c, w) for w in gr.WINDOWS}
                fig = gr.check_conditions(c, truths)
            eo, el = _check_launch(c, truths[window], window, n, o, lse)
            worst_o, worst_l = max(worst_o, eo), max(worst_l, el)
    print("GROUPS %s %s %s D%d O/bound %.3f LSE/bound %.3f %s" % (
        kind, gr.geom_id(geom), "bf16" if dtype == BF16 else "fp16", D, worst_o, worst_l,
        " ".join("%s=%.2f" % kv for kv in fig.items())))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("gi", range(len(gr.GEOMS)), ids=GEOM_IDS)
@pytest.mark.parametrize("kind", gr.KINDS)
def test_grouped_equals_expanded_bit_for_bit(kind, gi, dtype, D, formula_splits):
    """One split, window_left = -1: the grouped cache and H_kv = H on repeat_interleave'd K / V give the same bits of O
    and LSE (module docstring: a row's arithmetic does not depend on the row block it sits in)."""
    geom = gr.GEOMS[gi]
    _assert_geometry(geom)
    c = gr.make_case(kind, geom, dtype, D, gr.s_new(gi, dtype, D), "cuda")
    e = _expanded(c)
    assert e.kc.shape[1] == geom[0] and (kind[:3] != "fp8" or e.kd.shape == (gr.B, geom[0]))
    vck.splits(1)
    for window in ((-1, -1), (-1, 0)):
        o, lse, _, _ = _call(c, window)
        o2, lse2, _, _ = _call(e, window)
        assert torch.isfinite(o).all()
        for name, x, y in (("O", o, o2), ("LSE", lse, lse2)):
            assert bc.same_bits(x, y), (kind, geom, window, name, "%d elements differ" % int((x != y).sum()))


@pytest.mark.parametrize("ki", range(len(gr.KINDS)), ids=gr.KINDS)
def test_strided_q_and_o_give_the_contiguous_bits(ki, formula_splits):
    """g = 3: q as a [B, S_q, H, D] buffer seen as [B, H, S_q, D]; O comes back in that memory order with the bits of the
    contiguous call."""
    kind, dtype, D = gr.KINDS[ki], (F16, BF16)[ki % 2], (64, 128)[ki % 3 == 0]
    c = gr.make_case(kind, gr.GEOMS[0], dtype, D, 2, "cuda")
    qs = c.q.transpose(1, 2).contiguous().transpose(1, 2)
    assert not qs.is_contiguous() and torch.equal(qs, c.q)
    for n in (0, 1, 3):
        vck.splits(n)
        for window in ((-1, 0), (40, 8)):
            o, lse, _, _ = _call(c, window)
            os_, lses, _, _ = _call(c, window, q=qs)
            assert os_.transpose(1, 2).is_contiguous() and o.is_contiguous()
            assert bc.same_bits(os_.contiguous(), o) and bc.same_bits(lses, lse), (kind, window, n)
