"""mla_indexer.mla_indexer_logits_fp8_prefill against the fp64 truth on the same bytes and scales (einsum, clamp_min(0), weighted
head sum, scale, range mask) under the bound of tests/mlaindexercheck.py: visible columns within BOUND * M, hidden ones -inf bit
for bit, a repeated call the same bits.  `out` is pre-filled with NaN, and K holds 0x7F bytes and NaN scales in every row outside
the union of the ranges.  M 1, 15, 17, 33 (a partial block, a block edge, three blocks, a last wave of repeated rows) x N 1, 31,
33, 70, 300 (a column block, the tile edge, more tiles than the two-deep LDS ring)."""
import pytest
import torch

import mla_indexer as MI
import mlaindexercheck as ic
import variantcheck as vck
from blockcheck import same_bits

pytestmark = pytest.mark.gpu

MS, NS, BIG = (1, 15, 17, 33), (1, 31, 33, 70, 300), 2 ** 31 - 1
KINDS = ("full", "context", "packed", "random", "outside", "reversed")


def problem(M, N, Hi):
    g = torch.Generator().manual_seed(1000 * M + N + Hi)
    q8 = torch.randn(M, Hi, 128, generator=g).to(ic.F8)
    w = torch.randn(M, Hi, generator=g) * Hi ** -0.5                         # both signs
    k8 = torch.randn(N, 128, generator=g).to(ic.F8)
    sc = torch.exp2(torch.rand(N, generator=g) * 12 - 6)
    return q8, w, k8, sc


def ranges(kind, M, N):
    """(ks, ke) as lists; the kernel clamps both to [0, N]"""
    i = torch.arange(M)
    if kind == "full":
        ks, ke = torch.zeros(M), torch.full((M,), N)
    elif kind == "context":                                                 # a chunk behind N - M cached keys
        ks, ke = torch.zeros(M), N - M + i + 1
    elif kind == "packed":                                                  # three sequences; the second sees nothing
        seq = (3 * i) // max(M, 1)
        cu_k, cu_q = torch.tensor([0, N // 3, N // 2, N]), torch.tensor([0, -(-M // 3), -(-2 * M // 3), M])
        prior = (cu_k[1:] - cu_k[:-1]) - (cu_q[1:] - cu_q[:-1])
        ks = cu_k[seq]
        ke = torch.where(seq == 1, ks, ks + prior[seq] + (i - cu_q[seq]) + 1)
    elif kind == "random":                                                  # unaligned, ks mostly no multiple of 16
        g = torch.Generator().manual_seed(M + N)
        ks = torch.randint(0, N + 1, (M,), generator=g)
        ke = ks + torch.randint(0, N + 1, (M,), generator=g)
    elif kind == "outside":                                                 # negative and huge: clamped
        ks = torch.where(i % 3 == 2, torch.full((M,), 2 ** 30), -1 - i * (2 ** 31 // 40))
        ke = torch.where(i % 2 == 0, torch.full((M,), BIG), N + 7 + i)
    else:                                                                   # ke < ks
        ks, ke = N // 2 + 1 + i, N // 2 - i
    return ks.long().tolist(), ke.long().tolist()


def visible(ks, ke, N, W):
    lo, hi = (torch.tensor(x).clamp(0, N)[:, None] for x in (ks, ke))
    t = torch.arange(W)
    return (t >= lo) & (t < hi)


def truth(q8, w, k8, sc, ks, ke, W):
    """(fp64 logits [M, W] with -inf where hidden, the magnitude M of mlaindexercheck, the visibility mask)"""
    N = k8.shape[0]
    s = torch.einsum("mhd,td->mht", q8.double(), k8.double())
    ref = (w.double()[..., None] * s.clamp_min(0)).sum(1) * sc.double()
    mag = (w.double().abs()[..., None] * torch.einsum("mhd,td->mht", q8.double().abs(), k8.double().abs())).sum(1) * sc.double()
    vis = visible(ks, ke, N, W)
    pad = lambda x: torch.nn.functional.pad(x, (0, W - N))
    return torch.where(vis, pad(ref), torch.full((), float("-inf"), dtype=torch.float64)), pad(mag), vis


def device_args(q8, w, k8, sc, ks, ke):
    """the call's arguments, K and its scales poisoned in every row no range reaches"""
    used = visible(ks, ke, k8.shape[0], k8.shape[0]).any(0)
    kb = torch.where(used[:, None], k8.view(torch.uint8), torch.tensor(0x7F, dtype=torch.uint8))
    sd = torch.where(used, sc, torch.tensor(float("nan")))
    dev = lambda x: torch.tensor(x, dtype=torch.int64).clamp(-2 ** 31, BIG).to(torch.int32).cuda()
    return q8.cuda(), w.cuda(), kb.cuda().view(ic.F8), sd.cuda(), dev(ks), dev(ke)


def run(args):
    out = torch.full((args[0].shape[0], args[2].shape[0]), float("nan"), device="cuda")
    assert MI.mla_indexer_logits_fp8_prefill(*args, out=out) is out
    return out


check = lambda tag, prob, ks, ke, got: ic.held(tag, got, *truth(*prob, ks, ke, got.shape[1]))


@pytest.mark.parametrize("Hi,M", [(Hi, M) for Hi in (16, 64) for M in MS] + [(48, 33)])
def test_parity_over_rows_keys_heads_and_ranges(Hi, M):
    for N in NS if Hi != 48 else (70,):
        prob = problem(M, N, Hi)
        for kind in KINDS:
            ks, ke = ranges(kind, M, N)
            args = device_args(*prob, ks, ke)
            got = run(args)
            check("prefill H%d M%d N%d %s" % (Hi, M, N, kind), prob, ks, ke, got)
            assert same_bits(got, run(args)), "a repeated call gave other bits"


@pytest.mark.parametrize("h", [0, 15, 16, 63])
def test_one_head_at_a_time(h):
    """one-hot weights, another head in every row: a head permutation or a wave on another wave's weights fails"""
    q8, _, k8, sc = problem(17, 70, 64)
    w = torch.zeros(17, 64)
    w[torch.arange(17), (h + 5 * torch.arange(17)) % 64] = 1.0
    ks, ke = ranges("context", 17, 70)
    check("prefill head %d" % h, (q8, w, k8, sc), ks, ke, run(device_args(q8, w, k8, sc, ks, ke)))


@pytest.mark.parametrize("grp", range(8))
def test_one_16_dim_group_at_a_time(grp):
    """q zero outside dims [16 grp, 16 grp + 16): K read back from LDS in another byte order than q's fails"""
    q8, w, k8, sc = problem(17, 70, 64)
    q = torch.zeros(17, 64, 128)
    q[..., 16 * grp:16 * grp + 16] = q8.float()[..., 16 * grp:16 * grp + 16]
    q8 = q.to(ic.F8)
    ks, ke = ranges("full", 17, 70)
    check("prefill dims %d" % grp, (q8, w, k8, sc), ks, ke, run(device_args(q8, w, k8, sc, ks, ke)))


def test_relu_comes_before_the_weights():
    q8, w, k8, sc = problem(17, 70, 64)
    w = -w.abs() - 0.01
    ks, ke = ranges("full", 17, 70)
    got = run(device_args(q8, w, k8, sc, ks, ke))
    check("prefill negative weights", (q8, w, k8, sc), ks, ke, got)
    assert (got <= 0).all() and (got < 0).any()


def test_layouts_strided_q_weights_k_and_scales_and_an_out_slice_wider_than_n():
    M, N, Hi = 33, 70, 64
    prob = problem(M, N, Hi)
    ks, ke = ranges("random", M, N)
    q, w, k, s, lo, hi = device_args(*prob, ks, ke)
    plain = run((q, w, k, s, lo, hi))
    qt = q.view(torch.uint8).transpose(0, 1).contiguous().transpose(0, 1)        # a [H_i, M, 128] tensor transposed, as bytes
    wt = w.t().contiguous().t()
    kp = torch.full((N, 160), 0x7F, dtype=torch.uint8, device="cuda")            # a padded row stride
    kp[:, :128] = k.view(torch.uint8)
    s2 = torch.full((N, 2), float("nan"), device="cuda")
    s2[:, 0] = s
    wide = torch.full((M, N + 100), float("nan"), device="cuda")
    out = wide[:, 3:N + 53]                                                      # W = N + 50, rows only 4-byte aligned
    assert MI.mla_indexer_logits_fp8_prefill(qt, wt, kp[:, :128], s2[:, 0], lo, hi, out=out) is out
    assert same_bits(out[:, :N].contiguous(), plain) and (out[:, N:] == float("-inf")).all()
    assert torch.isnan(wide[:, :3]).all() and torch.isnan(wide[:, N + 53:]).all()
    check("prefill layouts", prob, ks, ke, out.contiguous())
    assert MI.mla_indexer_logits_fp8_prefill(q, w, k, s, lo, hi).shape == (M, N)          # no out: W = N
    assert MI.mla_indexer_logits_fp8_prefill(q[:0], w[:0], k, s, lo[:0], hi[:0]).shape == (0, N)          # M == 0: no launch
    assert (MI.mla_indexer_logits_fp8_prefill(q, w, k[:0], s[:0], lo, hi, out=wide) == float("-inf")).all()   # N == 0


def test_graph_replay_while_ks_and_ke_change_in_place():
    M, N = 17, 300
    q, w, k, s, lo, hi = device_args(*problem(M, N, 64), [0] * M, [N] * M)
    steps = [(ranges(kind, M, N)[1], torch.tensor(ranges(kind, M, N)[0], dtype=torch.int32).cuda()) for kind in ("context", "random", "packed")]
    vck.graph_replay(lambda x: MI.mla_indexer_logits_fp8_prefill(q, w, k, s, x, hi), hi, steps, extra=lo)


def test_select_on_the_logits_gives_the_truths_index_set():
    M, N, topk = 33, 300, 16
    prob = problem(M, N, 64)
    ks, ke = ranges("context", M, N)
    args = device_args(*prob, ks, ke)
    idx = MI.mla_indexer_select(run(args).view(M, 1, N), topk, lengths=args[5])
    want = torch.topk(truth(*prob, ks, ke, N)[0], topk).indices.sort(-1).values      # every row sees more than topk keys
    assert torch.equal(idx[:, 0].cpu().long(), want)
