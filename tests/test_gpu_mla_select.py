"""The top-k selection kernel (mla_indexer.mla_indexer_select) against a CPU reference of a few lines: NaN -> -inf, a stable
descending sort, the first topk columns whose value is above -inf, those in ascending order, -1 to the end.  The result is exact
and unique, so the comparison is torch.equal on int32 -- no tolerance.  Widths around the 16-byte vector (1, 5, 255, 1024, 1025,
4099), the last resident and the first streaming width (32768, 32769) and one 40000-wide row; topk below, at and above the
candidate count and the width; one row kind per way the radix passes can go wrong."""
import pytest
import torch

import mla_indexer as MI
import mlaindexercheck as ic
import variantcheck as vck

pytestmark = pytest.mark.gpu

NEG, INF, NAN = float("-inf"), float("inf"), float("nan")
SIZES = [(W, k) for W in (1, 5, 255, 1024, 1025, 4099) for k in (1, 7, 64, 2048)] + [(32768, 2048), (32769, 2048), (40000, 2048)]
KINDS = ["normal", "equal", "three", "low8", "negative", "up", "down", "mixed", "ninf"]


def reference(logits, topk, lengths=None):
    x = logits.detach().cpu().clone()
    W = x.shape[-1]
    for b, L in enumerate([] if lengths is None else lengths):
        x[b, :, max(0, min(int(L), W)):] = NEG
    x[torch.isnan(x)] = NEG
    val, idx = torch.sort(x, dim=-1, descending=True, stable=True)
    k = min(topk, W)
    idx = torch.where(val[..., :k] > NEG, idx[..., :k], torch.full_like(idx[..., :k], 1 << 40)).sort(-1).values
    idx = torch.where(idx == 1 << 40, torch.full_like(idx, -1), idx).to(torch.int32)
    return torch.nn.functional.pad(idx, (0, topk - k), value=-1)


def row(kind, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "normal":
        return torch.randn(W, generator=g)
    if kind == "equal":       # the threshold bin is the whole row: the overflow path, the first topk columns
        return torch.full((W,), 1.5)
    if kind == "three":       # the threshold falls inside a tie run
        return torch.randint(1, 4, (W,), generator=g).float()
    if kind == "low8":        # one coarse bin, one bin at both 8-bit levels: only the last five bits tell
        return (0x3F800000 + torch.randint(0, 256, (W,), generator=g)).to(torch.int32).view(torch.float32)
    if kind == "negative":    # the flipped half of the key space
        return -torch.rand(W, generator=g).exp()
    if kind in ("up", "down"):  # the chosen set at one end: the emit's bases carry across every step
        return torch.arange(W).float() * (1 if kind == "up" else -1)
    if kind == "ninf":
        return torch.full((W,), NEG)
    x = torch.zeros(W)        # mixed: +-0.0 ties at the threshold, denormals, +inf, NaN and -inf runs
    x[1::2] = -0.0
    x[::97] = torch.rand(len(x[::97]), generator=g) + 0.1
    x[5::211], x[6::211] = 1e-40, -1e-40
    x[10:20], x[30:45], x[3:4], x[W // 2:W // 2 + 1] = NAN, NEG, INF, INF
    return x


def rows(kind, B, Sq, W, seed=0):
    return torch.stack([row(kind, W, seed + j) for j in range(B * Sq)]).view(B, Sq, W)


@pytest.mark.parametrize("kind", KINDS)
def test_every_size_of_a_row_kind_equals_the_reference(kind):
    for W, k in SIZES:
        x = rows(kind, 1, 2, W, seed=W + k)
        got = MI.mla_indexer_select(x.cuda(), k)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), reference(x, k)), (kind, W, k)
    if kind == "equal":
        assert got[0, 0].tolist() == list(range(2048))


def test_rows_are_independent():
    x = torch.stack([row(kind, 4099, 7) for kind in KINDS[:6]]).view(3, 2, 4099)
    assert torch.equal(MI.mla_indexer_select(x.cuda(), 64).cpu(), reference(x, 64))


@pytest.mark.parametrize("W,k", [(5, 7), (1025, 64), (4099, 2048), (32768, 2048), (40000, 2048)])
def test_lengths_bound_the_scan(W, k):
    """+inf in every column at or past lengths[b]: it must not be chosen; lengths of 0, W and beyond W"""
    lens = [0, W, W + 9, W // 2 + 1, 3]
    x = rows("normal", len(lens), 2, W, seed=W)
    for b, L in enumerate(lens):
        x[b, :, min(L, W):] = INF
    got = MI.mla_indexer_select(x.cuda(), k, lengths=torch.tensor(lens, dtype=torch.int32).cuda())
    assert torch.equal(got.cpu(), reference(x, k, lens)) and (got[0] == -1).all()


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("W", [255, 4099, 32768, 32769])
def test_slices_of_wider_buffers(W, shift):
    """logits 1, 2 and 3 elements into a NaN-filled buffer with a row stride above W, `out` inside a sentinel-filled one"""
    k = 64
    x = rows("mixed", 2, 2, W, seed=shift)
    wide = torch.full((2, 2, W + 11), NAN, device="cuda")
    wide[..., shift:shift + W] = x.cuda()
    buf = torch.full((2, 2, k + 6), 77, dtype=torch.int32, device="cuda")
    out = buf[..., 3:3 + k]
    assert MI.mla_indexer_select(wide[..., shift:shift + W], k, out=out) is out
    assert torch.equal(out, MI.mla_indexer_select(x.cuda(), k)) and torch.equal(out.cpu(), reference(x, k))
    assert (buf[..., :3] == 77).all() and (buf[..., 3 + k:] == 77).all()


def test_the_same_set_as_the_torch_path():
    for W, k in [(4099, 64), (32768, 2048), (40000, 2048)]:
        x = rows("normal", 2, 1, W, seed=k).cuda()
        assert torch.equal(MI.mla_indexer_select(x, k), MI.mla_indexer_topk(x, k).sort(-1).values), (W, k)
    p = ic.Problem([40, 300], 64, 2, 64, 5, seed=3)        # fills below and above topk
    logits = MI.mla_indexer_logits_fp8(*p.args(), is_causal=True)
    got = MI.mla_indexer_select(logits, 64, lengths=p.sl)
    assert torch.equal(got.sort(-1).values, MI.mla_indexer_topk(logits, 64).sort(-1).values)
    assert torch.equal(got.cpu(), reference(logits, 64, p.fills))


def test_repeats_and_graph_replay():
    W, k = 4099, 64
    x = rows("three", 2, 2, W, seed=1).cuda()
    first = MI.mla_indexer_select(x, k)
    assert all(torch.equal(first, MI.mla_indexer_select(x, k)) for _ in range(5))
    lens = torch.tensor([W, W], dtype=torch.int32).cuda()
    vck.graph_replay(lambda lg: MI.mla_indexer_select(lg, k, lengths=lens), lens,
                     [([W, 100], None), ([0, 3000], rows("normal", 2, 2, W, seed=2).cuda()), ([5000, 64], None)], extra=x)
