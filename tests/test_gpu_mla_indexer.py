"""The indexer logits over a paged FP8 key cache (mla_indexer.mla_indexer_logits_fp8) against the fp64 truth on the cache's own
bytes and scales, under the bound of tests/mlaindexercheck.py (200 * 2^-24 * M per element, -inf bit for bit where hidden).
Permuted tables, NaN bytes and NaN scales wherever nothing may read, `out` pre-filled with NaN; fills around the 16-key column
block, the 32-key tile and the page edge, 300 keys for more than one tile per wave."""
import functools

import pytest
import torch

import mla_indexer as MI
import mlaindexercheck as ic
import variantcheck as vck
from blockcheck import same_bits

pytestmark = pytest.mark.gpu

FILLS = [0, 1, 15, 17, 33, 129, 300]


@functools.lru_cache(maxsize=None)
def problem(Hi, Sq, page, layout="plain"):
    return ic.Problem(FILLS, Hi, Sq, page, -(-320 // page), seed=Hi + Sq + page, row_stride=160 if layout == "padded" else 128,
                      joined=layout == "joined")


def run(p, causal, **kw):
    out = torch.full((len(p.fills), p.Sq, p.mp * p.page), float("nan"), device="cuda")
    assert MI.mla_indexer_logits_fp8(*p.args(), is_causal=causal, out=out, **kw) is out
    return out


def check(tag, p, got, causal, Ls=None, w=None, q8=None):
    ref, m, vis = ic.truth(p.q8 if q8 is None else q8, p.w if w is None else w, p.keys, p.scales, p.fills if Ls is None else Ls,
                           causal, got.shape[-1])
    return ic.held(tag, got, ref, m, vis)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Hi,Sq,page,layout", [(Hi, Sq, page, "plain") for Hi in (16, 64) for Sq in (1, 3, 9) for page in (32, 64)] +
                         [(64, 3, 32, "padded"), (48, 2, 64, "joined")])
def test_parity_over_fills_heads_rows_and_pages(Hi, Sq, page, layout, causal):
    p = problem(Hi, Sq, page, layout)
    got = run(p, causal)
    check("parity H%d S%d p%d %s %s" % (Hi, Sq, page, layout, causal), p, got, causal)
    assert same_bits(got, run(p, causal)), "a repeated call gave other bits"


def small():
    return ic.Problem([17, 70], 64, 2, 32, 3, seed=5)


@pytest.mark.parametrize("h", [0, 15, 16, 47, 63])
def test_one_head_at_a_time(h):
    """one-hot weights: the row is k_scale * relu(q_h . k); a head permutation or a dropped lane group fails"""
    p = small()
    w = torch.zeros_like(p.w)
    w[..., h] = 1.0
    p.wd = w.cuda()
    check("head %d" % h, p, run(p, False), False, w=w)


@pytest.mark.parametrize("grp", range(8))
def test_one_16_dim_group_at_a_time(grp):
    """q zero outside dims [16 grp, 16 grp + 16): a q / K byte-layout mismatch fails"""
    p = small()
    q = torch.zeros_like(p.q8.float())
    q[..., 16 * grp:16 * grp + 16] = p.q8.float()[..., 16 * grp:16 * grp + 16]
    q8 = q.to(ic.F8)
    p.q = q8.cuda()
    check("dims %d" % grp, p, run(p, False), False, q8=q8)


def test_relu_comes_before_the_weights():
    p = small()
    w = -p.w.abs() - 0.01
    p.wd = w.cuda()
    got = run(p, False)
    check("negative weights", p, got, False, w=w)
    assert (got[torch.isfinite(got)] <= 0).all() and (got[1, :, :70] < 0).any()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_append_quantises_rows_in_through_the_table(dtype):
    """fills inside a page, across a page edge and onto a fresh page; an all-zero row (scale 1.0) and an outlier row"""
    from fp8_token_kvcache import quantize_kv_fp8_per_token
    fills, Sq, page = [5, 30, 64], 3, 32
    p = ic.Problem(fills, 64, Sq, page, 4, seed=9, reach=[f + Sq for f in fills])
    new = torch.randn(3, Sq, 128, generator=torch.Generator().manual_seed(10)).to(dtype)
    new[0, 1] = 0
    new[1, 2, 77] = 3000.0
    x8, s = quantize_kv_fp8_per_token(new)
    pool, scale, table = p.pool.cpu(), p.scale.cpu(), p.table.cpu()
    for b, f in enumerate(fills):
        for i in range(Sq):
            pool[table[b, (f + i) // page], (f + i) % page] = x8[b, i].view(torch.uint8)
            scale[table[b, (f + i) // page], (f + i) % page] = s[b, i]
            p.keys.view(torch.uint8)[b, f + i], p.scales[b, f + i] = x8[b, i].view(torch.uint8), s[b, i]
    got = run(p, True, k_new=new.cuda())
    assert torch.equal(p.pool.cpu(), pool) and torch.equal(p.scale.cpu().view(torch.int32), scale.view(torch.int32))
    assert p.sl.cpu().tolist() == fills
    check("append %s" % dtype, p, got, True, Ls=[f + Sq for f in fills])


def test_layouts_strided_q_and_weights_and_an_out_slice_wider_than_the_table():
    p = problem(64, 3, 32)
    B, S = len(FILLS), p.mp * p.page
    plain = run(p, True)
    q = p.q.view(torch.uint8).transpose(1, 2).contiguous().transpose(1, 2)   # a [B, H_i, S_q, 128] tensor transposed, as bytes
    w = p.wd.transpose(1, 2).contiguous().transpose(1, 2)
    wide = torch.full((B, 3, S + 100), float("nan"), device="cuda")
    out = wide[..., 4:S + 54]                                        # W = S + 50: past the table's reach
    MI.mla_indexer_logits_fp8(q, w, p.pool, p.scale, p.sl, p.table, is_causal=True, out=out)
    assert same_bits(out[..., :S].contiguous(), plain)
    assert (out[..., S:] == float("-inf")).all()
    assert torch.isnan(wide[..., :4]).all() and torch.isnan(wide[..., S + 54:]).all()
    check("layouts", p, out.contiguous(), True)
    assert MI.mla_indexer_logits_fp8(*p.args()).shape == (B, 3, S)    # no out: W = max_pages_per_seq * page_size


def test_graph_replay_while_seqlens_and_table_change_in_place():
    p = ic.Problem([100, 100], 64, 2, 32, 4, seed=11)
    call = lambda t: MI.mla_indexer_logits_fp8(p.q, p.wd, p.pool, p.scale, p.sl, p.table if t is None else t, is_causal=True)
    vck.graph_replay(call, p.sl, [([100, 37], None), ([5, 64], p.table.flip(0).clone()), ([0, 96], None)], extra=p.table)


def test_topk_gives_the_truths_index_set_and_pads_short_rows():
    p = ic.Problem([300, 10], 64, 1, 64, 5, seed=12)
    got = run(p, False)
    idx = MI.mla_indexer_topk(got, 16)
    ref, _, _ = ic.truth(p.q8, p.w, p.keys, p.scales, p.fills, False, got.shape[-1])
    assert idx.dtype == torch.int32 and idx.shape == (2, 1, 16)
    assert sorted(idx[0, 0].tolist()) == sorted(torch.topk(ref[0, 0], 16).indices.tolist())
    assert sorted(idx[1, 0, :10].tolist()) == list(range(10)) and (idx[1, 0, 10:] == -1).all()
