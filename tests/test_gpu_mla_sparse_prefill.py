"""mla_sparse_prefill.flash_attention_mla_sparse_prefill against the fp64 truth: per token the visible rows of its list gathered
(duplicates kept, in list order), softmax(scale q k^T) times kv[:, :512].  The packed problem is tests/mlasparsecheck.py's with
ONE sequence of N keys and the M tokens as its S_q rows, non-causal: truth, level and bounds are that module's and
tests/mlacheck.py's, unchanged (16-bit P, fp32 accumulation, as the sparse decode call)."""
import pytest
import torch

import fa_oracle as fo
import mlacheck as mc
import mlasparsecheck as msc
from blockcheck import same_bits

pytestmark = pytest.mark.gpu


def P():
    import mla_sparse_prefill
    return mla_sparse_prefill.flash_attention_mla_sparse_prefill


def run(q4, kv3, idx, **kw):
    """the call on the decode-shaped problem (q [1, H, M, 576], kv [1, N, 576], indices [1, M, topk]) -> (O [1, H, M, 512],
    LSE [1, H, M]); q goes in as a strided [M, H, 576] view"""
    O, LSE = P()(q4[0].transpose(0, 1), kv3[0], idx[0], return_lse=True, **kw)
    assert O.shape == (q4.shape[2], q4.shape[1], mc.DV) and LSE.shape == O.shape[:2]
    return O.transpose(0, 1)[None], LSE.t()[None]


def check(tag, q4, kv3, idx, scale=None, **kw):
    got = run(q4, kv3, idx, **kw)
    msc.held(tag, msc.reference(q4, kv3, idx, [kv3.shape[1]], False, scale), got)
    return got


# M: ids past M, tokens on either side of a group of 8; H: a partial head block, several blocks; topk: a partial last tile, several
SHAPES = [(1, 1, 1, 5), (7, 16, 31, 40), (9, 40, 33, 100), (19, 128, 160, 300), (1, 128, 33, 64), (9, 16, 160, 70), (19, 1, 31, 20),
          (7, 40, 1, 33)]


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
@pytest.mark.parametrize("M,H,topk,N", SHAPES)
def test_parity_over_tokens_heads_and_list_lengths(M, H, topk, N, dtype):
    q4, kv3 = mc.make(1, H, M, N, dtype, seed=M + H + topk)
    idx = msc.draw([N], M, topk, seed=N).cuda()
    check("prefill M%d H%d topk%d N%d" % (M, H, topk, N), q4, kv3, idx)


@pytest.mark.parametrize("dtype", mc.DT, ids=mc.IDS)
def test_distinct_heads_with_a_rising_maximum(dtype):
    """every head its own query and score magnitude (2^-2 .. 2^2), keys that score higher the later they come in an ascending
    list: the running maximum rises in every tile, so a wave pairing P or a rescale factor with another head fails"""
    M, H, N = 3, 40, 160
    g = torch.Generator(device="cuda").manual_seed(7)
    u = torch.randn(mc.D, generator=g, device="cuda")
    gain = torch.exp2((torch.arange(H, device="cuda") % 5 - 2).float())[None, :, None, None]
    q4 = (gain * (u + 0.5 * torch.randn(1, H, M, mc.D, generator=g, device="cuda"))).to(dtype)
    ramp = torch.arange(N, device="cuda")[None, :, None] / N
    kv3 = (0.25 * ramp * u + 0.5 * torch.randn(1, N, mc.D, generator=g, device="cuda")).to(dtype)
    idx = torch.arange(N, dtype=torch.int32, device="cuda").expand(1, M, N)
    check("prefill distinct heads", q4, kv3, idx)


@pytest.mark.parametrize("grp", range(36))
def test_one_16_column_group_of_q_at_a_time(grp):
    """q zero outside columns [16 grp, 16 grp + 16): a wave on another wave's columns, or K in another order than q, fails"""
    dtype = mc.DT[grp % 2]
    q0, kv3 = mc.make(1, 8, 2, 40, dtype, seed=200 + grp)
    q4 = torch.zeros_like(q0)
    q4[..., 16 * grp:16 * grp + 16] = 4 * q0[..., 16 * grp:16 * grp + 16]
    check("prefill q group %d" % grp, q4, kv3, msc.draw([40], 2, 40, seed=grp).cuda())


def test_awkward_lists_and_poisoned_unnamed_rows():
    N, topk, H = 300, 2017, 16
    q4, kv3 = mc.make(1, H, 6, N, mc.F16, seed=11)
    g = torch.Generator().manual_seed(12)
    junk = torch.tensor([-1, N, 1 << 30, -(1 << 31)])
    rows = [junk[torch.arange(topk) % 4] for _ in range(6)]                       # row 0: nothing visible
    rows[1][2016] = 17                                                             # one visible entry in 2017
    live = lambda n: torch.randint(0, 150, (n,), generator=g)
    rows[2] = torch.full((topk,), -1)                                              # dead tiles first, between and after live ones
    rows[2][64:96], rows[2][224:260], rows[2][1000:1003] = live(32), live(36), live(3)
    rows[3] = torch.cat([torch.full((100,), 5), live(50), torch.full((topk - 150,), 5)])      # duplicates, in every tile
    rows[4] = torch.tensor([-1, N - 1, N, 1 << 30, -(1 << 31)]).repeat(404)[:topk]
    rows[5] = torch.cat([live(40), torch.full((topk - 40,), N)])                  # live, then dead to the end
    idx = torch.stack(rows)[None].to(torch.int32).cuda()
    got = check("prefill awkward lists", q4, kv3, idx)
    assert (got[0][0, :, 0] == 0).all() and torch.isneginf(got[1][0, :, 0]).all()
    named = torch.zeros(N, dtype=torch.bool, device="cuda")
    named[idx[(idx >= 0) & (idx < N)].long()] = True
    assert 0 < named.sum() < N
    poisoned = torch.where(named[None, :, None], kv3, torch.full_like(kv3, float("nan")))
    again = run(q4, poisoned, idx)
    assert same_bits(got[0], again[0]) and same_bits(got[1], again[1]), "a row no valid entry names reached the result"


def test_strides_outputs_and_repeated_launches():
    M, H, N, topk = 9, 40, 100, 70
    q4, kv3 = mc.make(1, H, M, N, mc.BF16, seed=21)
    idx = msc.draw([N], M, topk, seed=22).cuda()
    q, kv, ix = q4[0].transpose(0, 1).contiguous(), kv3[0], idx[0]
    O, LSE = P()(q, kv, ix, return_lse=True)
    msc.held("prefill contiguous", msc.reference(q4, kv3, idx, [N], False), (O.transpose(0, 1)[None], LSE.t()[None]))
    O2, LSE2 = P()(q, kv, ix, return_lse=True)
    assert same_bits(O, O2) and same_bits(LSE, LSE2), "a repeated call gave other bits"
    nan = float("nan")
    qw = torch.full((M, H, 640), nan, dtype=q.dtype, device="cuda")                  # strided q, read in place
    qw[..., 32:608] = q
    kw = torch.full((N, 640), nan, dtype=q.dtype, device="cuda")                     # a kv row stride of 640
    kw[:, :576] = kv
    iw = torch.full((M, topk + 5), 3, dtype=torch.int32, device="cuda")              # an indices row stride of topk + 5
    iw[:, 3:3 + topk] = ix
    ow = torch.full((M, H, 520), nan, dtype=q.dtype, device="cuda")
    out = ow[..., :512]
    assert P()(qw[..., 32:608], kw[:, :576], iw[:, 3:3 + topk], out=out) is out
    assert same_bits(out.contiguous(), O) and torch.isnan(ow[..., 512:]).all()
    qo = torch.zeros(M, H, 577, dtype=q.dtype, device="cuda")                        # strides no multiple of 8: copied
    qo[..., :576] = q
    assert same_bits(P()(qo[..., :576], kv, ix), O)
    assert P()(q[:0], kv, ix[:0]).shape == (0, H, 512)                               # M == 0: no launch
    half = check("prefill scale", q4, kv3, idx, 0.5 * mc.DEFAULT_SCALE, softmax_scale=0.5 * mc.DEFAULT_SCALE)
    assert not same_bits(half[0].contiguous(), O.transpose(0, 1)[None].contiguous())


def test_agreement_with_the_decode_call_on_one_sequence_of_pages():
    import mla_sparse_kvcache
    M, H, N, topk, page = 5, 40, 128, 70, 64
    q4, kv3 = mc.make(1, H, M, N, mc.F16, seed=31)
    idx = msc.draw([N], M, topk, seed=32).cuda()
    o, lse = run(q4, kv3, idx)
    lens = torch.tensor([N], dtype=torch.int32, device="cuda")
    table = torch.arange(N // page, dtype=torch.int32, device="cuda")[None]
    od, ld = mla_sparse_kvcache.flash_attention_mla_kvcache_sparse(q4, kv3[0].view(N // page, page, mc.D), idx, lens, table, return_lse=True)
    assert fo.rel_fro(od.double(), o) < mc.FP16_BOUND
    assert torch.allclose(lse, ld, rtol=1e-3, atol=2e-3)


def test_a_latent_array_beyond_4_gib():
    N, H, M = 3_800_000, 16, 3
    try:
        kv = torch.empty(N, mc.D, dtype=mc.F16, device="cuda")
    except RuntimeError as e:                                                         # (torch.OutOfMemoryError is one)
        pytest.skip("no room for a latent array of %d bytes: %s" % (N * mc.D * 2, str(e)[:80]))
    assert kv.numel() * 2 > 1 << 32
    named = torch.tensor([0, 1_864_135, 1_864_136, 3_728_270, 3_728_271, N - 2, N - 1], device="cuda")    # across 2^31 and 2^32 bytes
    q4, small = mc.make(1, H, M, len(named), mc.F16, seed=41)
    kv[named] = small[0]                                                              # only these rows are ever initialised
    pick = torch.tensor([[6, 3, 4, 0, 1, 2, 5, 6], [4, 4, 6, 1, 0, 0, 0, 3], [5, 6, 2, 3, 3, 1, 0, 4]], device="cuda")
    junk = torch.tensor([-1, N, -1], device="cuda")[:, None]
    idx = torch.cat([named[pick], junk], 1).to(torch.int32)
    O, LSE = P()(q4[0].transpose(0, 1), kv, idx, return_lse=True)
    ref = msc.reference(q4, small, torch.cat([pick, junk.clamp(max=-1)], 1).to(torch.int32)[None], [len(named)], False)
    msc.held("prefill beyond 4 GiB", ref, (O.transpose(0, 1)[None], LSE.t()[None]))


def test_logits_select_and_attention_end_to_end_on_two_packed_sequences():
    import mla_indexer as MI
    from test_gpu_mla_indexer_prefill import device_args, problem
    lens, topk, H = (23, 50), 16, 16                                                  # two prompts, packed: M = N = 73
    M = N = sum(lens)
    ks = [0] * lens[0] + [lens[0]] * lens[1]
    ke = [i + 1 for i in range(lens[0])] + [lens[0] + i + 1 for i in range(lens[1])]
    args = device_args(*problem(M, N, 64), ks, ke)
    logits = MI.mla_indexer_logits_fp8_prefill(*args)
    idx = MI.mla_indexer_select(logits.view(M, 1, N), topk, lengths=args[5])[:, 0]
    assert ((idx < 0) |((idx >= args[4][:, None]) & (idx < args[5][:, None]))).all()
    q4, kv3 = mc.make(1, H, M, N, mc.BF16, seed=51)
    check("prefill end to end", q4, kv3, idx[None])
