"""CPU tests: the oracle against the reference's own outputs (tests/golden, produced by
oracle/make_golden.py from the reference's Triton kernel bodies) and against fp64 math."""
import pytest
import torch

import fa_oracle as fo
from _util import golden_names, load_golden, load_kat, rand_inputs


@pytest.mark.parametrize("name", golden_names())
def test_oracle_matches_reference_kernels(name):
    g = load_golden(name)
    m = g["meta"]
    r = fo.fwd_bwd_tiled(g["Q"], g["K"], g["V"], g["dO"], m["causal"], m["BM"], m["BN"])
    # same algorithm, same rounding points: only fp32 summation order differs (a few fp16 ulps flip)
    for k in ("O", "dQ", "dK", "dV"):
        assert fo.rel_fro(g["ref_" + k], r[k]) < 5e-5, k
        assert (g["ref_" + k].float() - r[k].float()).abs().max() < 4e-3, k
    assert (g["ref_LSE"] - r["LSE"]).abs().max() < 4e-6
    assert (g["ref_delta"] - r["delta"]).abs().max() < 1e-3


@pytest.mark.parametrize("name", golden_names())
def test_reference_kernels_match_fp64(name):
    """The pins themselves are sane: reference outputs vs fp64 attention."""
    g = load_golden(name)
    m = g["meta"]
    gt = fo.attention_fp64(g["Q"], g["K"], g["V"], g["dO"], m["causal"])
    for k in ("O", "dQ", "dK", "dV"):
        assert fo.rel_fro(gt[k], g["ref_" + k]) < 1e-3, k  # BASELINE "within 1e-3 rel"
        assert fo.verify_metrics(gt[k], g["ref_" + k])["passed"], k
    assert (g["ref_LSE"].double() - gt["LSE"]).abs().max() < 1e-3  # Phase_3.md:752-753
    assert (g["ref_delta"].double() - gt["delta"]).abs().max() < 5e-3


@pytest.mark.parametrize("shape", [(1, 2, 500, 500, 64, True), (1, 2, 500, 500, 64, False),
                                   (1, 1, 77, 333, 64, False), (1, 2, 384, 128, 64, True),
                                   (1, 1, 200, 200, 128, True)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_oracle_ragged_and_cross_vs_fp64(shape, dtype):
    """Masked tails (Phase-3/4 semantics): any S_q, S_k; where the reference's descriptor path is wrong."""
    B, H, Sq, Sk, D, causal = shape
    Q, K, V, dO = rand_inputs(B, H, Sq, Sk, D, dtype, seed=3)
    gt = fo.attention_fp64(Q, K, V, dO, causal)
    r = fo.fwd_bwd_tiled(Q, K, V, dO, causal, 64, 64)
    tol = 1e-3 if dtype == torch.float16 else 8e-3
    for k in ("O", "dQ", "dK", "dV"):
        assert fo.rel_fro(gt[k], r[k]) < tol, (k, fo.rel_fro(gt[k], r[k]))
    assert (r["LSE"].double() - gt["LSE"]).abs().max() < 1e-3


def test_oracle_tile_config_insensitive():
    Q, K, V, dO = rand_inputs(1, 2, 256, 256, 64, torch.float16, seed=5)
    a = fo.fwd_bwd_tiled(Q, K, V, dO, True, 64, 64)
    b = fo.fwd_bwd_tiled(Q, K, V, dO, True, 32, 64)
    for k in ("O", "dQ", "dK", "dV"):
        assert fo.rel_fro(a[k], b[k]) < 1e-4


def test_fp64_matches_torch_sdpa():
    Q, K, V, dO = rand_inputs(2, 2, 96, 160, 64, torch.float32, seed=7)
    for causal in (False, True):
        gt = fo.attention_fp64(Q, K, V, dO, causal)
        o = torch.nn.functional.scaled_dot_product_attention(Q.double(), K.double(), V.double(), is_causal=causal)
        assert torch.allclose(gt["O"], o, atol=1e-12)


def test_verify_metrics_kat():
    kat = load_kat()["verify"]
    b = torch.linspace(-1, 1, 64).view(8, 8)
    for case in kat:
        t = b + case["eps"] * torch.sin(torch.arange(64.0)).view(8, 8)
        m = fo.verify_metrics(b, t)
        assert m["passed"] == case["passed"]
        for k in ("max_abs", "mean_abs", "max_rel", "max_norm"):
            assert abs(m[k] - case[k]) <= 6e-3 * abs(case[k]), k  # the reference prints 3 digits
        assert abs(m["cos"] - case["cos"]) < 2e-6


def test_naive_attention_kat():
    n = 2 * 1 * 4 * 8
    q = ((torch.arange(n) % 7 - 3) / 4.0).view(2, 1, 4, 8)
    k = ((torch.arange(n) % 5 - 2) / 3.0).view(2, 1, 4, 8)
    v = ((torch.arange(n) % 3 - 1) / 2.0).view(2, 1, 4, 8)
    for case in load_kat()["naive"]:
        o = fo.naive_attention(q, k, v, case["causal"])
        assert torch.allclose(o.flatten(), torch.tensor(case["o"]), atol=1e-6)


def test_flops_kat():
    for c in load_kat()["flops"]:
        for mode in ("fwd", "bwd", "fwd_bwd"):
            assert fo.attention_flops(c["B"], c["H"], c["S"], c["S"], c["D"], c["causal"], mode) == c[mode]
    assert fo.attention_flops(4, 32, 4096, 4096, 64, True, "fwd") == 274_877_906_944
    assert fo.attention_flops(4, 32, 4096, 4096, 64, True, "fwd_bwd") == 962_072_674_304


def test_varlen_oracle_equals_the_batched_oracle_on_equal_lengths():
    """attention_varlen_fp64 (the ground truth of the varlen extension, Phase_6.md:119-178) on a batch whose sequences
    all have the same length is the batched fp64 oracle on the packed-to-[B,H,S,D] view, and sequences do not leak."""
    torch.manual_seed(3)
    B, H, S, D = 3, 2, 24, 16
    Q, K, V, dO = (torch.randn(B, H, S, D) for _ in range(4))
    pack = lambda t: t.transpose(1, 2).reshape(B * S, H, D)
    cu = [0, S, 2 * S, 3 * S]
    for causal in (False, True):
        ref = fo.attention_fp64(Q, K, V, dO, causal)
        got = fo.attention_varlen_fp64(pack(Q), pack(K), pack(V), pack(dO), cu, cu, causal)
        for k in ("O", "dQ", "dK", "dV"):
            assert torch.allclose(got[k], pack(ref[k]), atol=1e-12), k
        assert torch.allclose(got["LSE"], ref["LSE"].permute(1, 0, 2).reshape(H, B * S), atol=1e-12)
    # ragged, different q / k lengths, one empty sequence: each sequence is its own problem
    cu_q, cu_k = [0, 5, 5, 17], [0, 9, 12, 20]
    Q, dO = torch.randn(17, H, D), torch.randn(17, H, D)
    K, V = torch.randn(20, H, D), torch.randn(20, H, D)
    got = fo.attention_varlen_fp64(Q, K, V, dO, cu_q, cu_k, True)
    one = fo.attention_fp64(Q[5:17].transpose(0, 1)[None], K[12:20].transpose(0, 1)[None], V[12:20].transpose(0, 1)[None],
                            dO[5:17].transpose(0, 1)[None], True)
    assert torch.allclose(got["O"][5:17], one["O"][0].transpose(0, 1), atol=1e-12)
    assert got["dK"][9:12].abs().max() == 0          # keys of the empty-query sequence get no gradient


def test_philox4x32_10_known_answers_and_keep_mask_layout():
    """The oracle's Philox against the Random123 known-answer vectors (kat_vectors: philox4x32 10), and the byte /
    word layout of the 4 x 4 keep patches the kernels regenerate (include/mi355fa.h, fa_*_dropout)."""
    import numpy as np
    kats = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
             (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kats:
        got = fo.philox4x32_10(*[np.uint32(c) for c in ctr], key[0], key[1])
        assert tuple(int(x) for x in got) == out
    keep, rp = fo.dropout_keep_mask(2, 3, 37, 50, 0.25, seed=0x123456789abcdef, offset=7)
    assert keep.shape == (2, 3, 37, 50) and rp == 256.0 / 192.0
    # element (b=1, h=2, q=13, k=22): word q & 3 = 1, byte k & 3 = 2 of the patch (q >> 2, k >> 2) = (3, 5)
    w = fo.philox4x32_10(np.uint32(3), np.uint32(5), np.uint32(1 * 3 + 2), np.uint32(7), 0x89abcdef, 0x01234567)
    assert bool(keep[1, 2, 13, 22]) == (((int(w[1]) >> 16) & 255) >= 64)
    frac = keep.float().mean().item()
    assert abs(frac - 0.75) < 0.02                      # P(keep) = 1 - p
    k0, _ = fo.dropout_keep_mask(1, 1, 8, 8, 0.0, seed=1)
    assert k0.all()                                     # p = 0 keeps everything
    k2, _ = fo.dropout_keep_mask(2, 3, 37, 50, 0.25, seed=0x123456789abcdef, offset=8)
    assert not torch.equal(keep, k2)                    # a different offset is a different mask


def test_varlen_dropout_oracle_equals_the_batched_one_on_equal_lengths():
    """attention_varlen_dropout_fp64 on a packed batch of equal-length sequences = attention_dropout_fp64 on the same
    sequences stacked as [B, H, S, D] with the same (seed, offset): sequence b uses the mask of batch index b."""
    B, H, S, D, p, seed, offset = 3, 2, 37, 16, 0.3, 0x1234ABCD, 7
    torch.manual_seed(2)
    Q, K, V, dO = (torch.randn(B, H, S, D, dtype=torch.float64) for _ in range(4))
    keep, rp = fo.dropout_keep_mask(B, H, S, S, p, seed, offset)
    want = fo.attention_dropout_fp64(Q, K, V, dO, True, keep, rp)
    pk = lambda x: x.transpose(1, 2).reshape(B * S, H, D)
    cu = [S * i for i in range(B + 1)]
    got = fo.attention_varlen_dropout_fp64(pk(Q), pk(K), pk(V), pk(dO), cu, cu, True, p, seed, offset)
    for k in ("O", "dQ", "dK", "dV"):
        assert torch.allclose(got[k], pk(want[k]), rtol=1e-12, atol=1e-12), k


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_chunked_fp64_reference_equals_the_autograd_one(causal):
    """attention_fp64_chunked (closed-form gradients, a few (batch, head) slices at a time; the device reference of
    tests/test_gpu_persistent.py) against attention_fp64 (autograd), with chunks smaller than the batch so that the slicing
    itself is exercised; S_q > S_k and S_q < S_k under the top-left causal mask."""
    for (B, H, Sq, Sk) in ((2, 3, 200, 333), (1, 4, 333, 160)):
        Q, K, V, dO = rand_inputs(B, H, Sq, Sk, 64, torch.bfloat16, seed=Sq)
        gt = fo.attention_fp64(Q, K, V, dO, causal)
        ch = fo.attention_fp64_chunked(Q, K, V, dO, causal, max_bytes=2 * Sq * Sk * 8)
        for k in ("O", "LSE", "dQ", "dK", "dV", "delta"):
            assert ch[k].dtype == torch.float64 and ch[k].shape == gt[k].shape, k
            assert (ch[k] - gt[k]).abs().max() <= 1e-10 * gt[k].abs().max(), k
        if causal and Sk > Sq:
            assert (ch["dK"][:, :, Sq:] == 0).all() and (ch["dV"][:, :, Sq:] == 0).all()
        a = Q.double().abs() @ K.double().abs().transpose(-1, -2) / 8
        if causal:
            a = a.masked_fill(torch.arange(Sq)[:, None] < torch.arange(Sk)[None, :], 0)
        assert torch.allclose(ch["SABS"], a.amax(-1), rtol=1e-12, atol=0)


def test_block_check_catches_one_bad_block_the_global_norm_misses():
    """The per-block check of tests/test_gpu_persistent.py has teeth where the whole-tensor relative Frobenius norm has none:
    at the headline shape [4, 32, 4096, 64] with bf16-level noise everywhere, one 128-row block 3 % wrong moves the global
    norm by ~6e-5, far inside the 6e-3 the device-SDPA comparisons allow -- the block check names that block."""
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(4, 32, 4096, 64, generator=g, dtype=torch.float64)
    out = ref + ref * (2.0 ** -9) * torch.randn(ref.shape, generator=g, dtype=torch.float32).to(torch.float64)
    clean = fo.rel_fro(ref, out)
    b, h, rb = 2, 17, 21
    blk = (slice(b, b + 1), slice(h, h + 1), slice(rb * 128, rb * 128 + 128))
    noise = torch.randn(1, 1, 128, 64, generator=g, dtype=torch.float64)
    out[blk] += 0.03 * noise * ref[blk].norm() / noise.norm()
    glob = fo.rel_fro(ref, out)
    assert glob < 6e-3 and glob - clean < 1e-4, (clean, glob)   # alone, the bad block is 3e-2 / 64 ~ 5e-4
    st = fo.block_stats(ref, out)
    assert st["worst"] == (b, h, rb) and st["worst_ratio_at"] == (b, h, rb)
    assert abs(st["max"] - 0.03) < 1e-3 and st["median"] < 3e-3, st["median"]
    with pytest.raises(AssertionError, match=r"\(2, 17, 21\) has error 3\.0"):
        fo.assert_blocks("O", st, bound=6e-3)
    fo.assert_blocks("O", fo.block_stats(ref[:, :, :2048], out[:, :, :2048]), bound=6e-3)   # the clean half passes
    # below the absolute bound, the median limit still catches a block far off its group's error scale
    out[blk] = ref[blk] + (out[blk] - ref[blk]) * (4e-3 / 0.03)
    st = fo.block_stats(ref, out)
    assert st["max"] < 6e-3 and st["worst_ratio_at"] == (b, h, rb)
    with pytest.raises(AssertionError, match="median"):
        fo.assert_blocks("O", st, bound=6e-3, ratio=1.5)


def test_block_check_zero_blocks_and_nan():
    """A block whose reference is exactly zero must come out exactly zero; NaN is an error of inf, never a pass;
    a ragged last block counts only its real rows; groups take their own median."""
    ref = torch.randn(2, 3, 300, 64, dtype=torch.float64)
    ref[1, 2] = 0
    out = ref.clone()
    st = fo.block_stats(ref, out)
    assert st["err"].shape == (2, 3, 3) and st["max"] == 0.0
    fo.assert_blocks("x", st, bound=1e-12)
    out[1, 2, 299, 5] = 1e-30                       # a zero block written non-zero, in the ragged last block
    st = fo.block_stats(ref, out)
    assert st["worst"] == (1, 2, 2) and st["max"] == float("inf")
    with pytest.raises(AssertionError, match=r"\(1, 2, 2\)"):
        fo.assert_blocks("x", st, bound=1.0)
    out = ref.clone()
    out[0, 1, 130] = float("nan")
    st = fo.block_stats(ref, out)
    assert st["worst"] == (0, 1, 1) and st["max"] == float("inf")
    with pytest.raises(AssertionError):
        fo.assert_blocks("x", st, bound=1.0, ratio=1e9)
    # two groups whose error scales differ by 10x: each within 4x of its own median
    out = ref * (1 + 1e-4 * torch.randn_like(ref))
    out[:, 0] = ref[:, 0] * (1 + 1e-3 * torch.randn_like(ref[:, 0]))
    groups = torch.tensor([[1, 0, 0], [1, 0, 0]])
    fo.assert_blocks("x", fo.block_stats(ref, out, groups), bound=1e-2)
    with pytest.raises(AssertionError, match="median"):
        fo.assert_blocks("x", fo.block_stats(ref, out), bound=1e-2)


def _assert_same_fp64(got, want, what):
    """got == want to 1e-10 of want's largest magnitude; -inf (a row without a visible key) exactly where want has it."""
    assert got.dtype == torch.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    want = want.double()
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], want[inf]), what
    fin = ~inf
    tol = 1e-10 * max(want[fin].abs().max().item(), 1e-300) if fin.any() else 0.0
    assert (got[fin] - want[fin]).abs().max().item() <= tol, (what, (got[fin] - want[fin]).abs().max().item(), tol)


# (H, H_kv): g = 1, 4, 32 (multi-query); windows: full, causal, (w, 0), (w, w), (0, w), (-1, w).  With S_q = 90 > S_k = 61
# the rows past S_k + wl of a window with wl >= 0 see no key at all.
CHUNK_GROUPS = [(2, 2), (8, 2), (32, 1)]
CHUNK_WINDOWS = [(-1, -1), (-1, 0), (9, 0), (7, 7), (0, 5), (-1, 3)]


@pytest.mark.parametrize("H,Hkv", CHUNK_GROUPS, ids=["g1", "g4", "g32"])
def test_chunked_oracle_window_and_groups_equal_the_gpu_tests_formulas(H, Hkv):
    """attention_fp64_chunked with window= and H_kv < H against the independent masked / repeat_interleave'd closed form of
    tests/attn_ref.py, the truth of tests/test_gpu_local.py (g = 1) and tests/test_gpu_gqa.py (g > 1): O, LSE, dQ, dK, dV, delta = rowsum(dO * O), and
    rows with no visible key (O = 0, LSE = -inf, dQ = 0).  max_bytes holds two (batch, head) slices, so several chunks
    run and the K/V head of a chunk's slices changes inside a chunk and between chunks."""
    import attn_ref
    import test_gpu_gqa as tg
    B, Sq, Sk, D = 2, 90, 61, 64
    Q, K, V, dO = tg.inputs(B, H, Hkv, Sq, Sk, D, torch.bfloat16, seed=H + Hkv)
    for w in CHUNK_WINDOWS:
        want = attn_ref.attention_fp64(Q, K, V, dO, D ** -0.5, attn_ref.visible(Sq, Sk, *w, "cpu"))
        got = fo.attention_fp64_chunked(Q, K, V, dO, window=w, max_bytes=2 * Sq * Sk * 8)
        for n in ("O", "LSE", "dQ", "dK", "dV"):
            _assert_same_fp64(got[n], want[n], (w, n))
        _assert_same_fp64(got["delta"], (dO.double() * want["O"]).sum(-1), (w, "delta"))
        vis = fo.visible_mask(Sq, Sk, w)
        empty = ~vis.any(-1)
        assert bool(empty.any()) == (w[0] >= 0), w
        assert (got["O"][:, :, empty] == 0).all() and (got["dQ"][:, :, empty] == 0).all()
        assert torch.isneginf(got["LSE"][:, :, empty]).all() and (got["delta"][:, :, empty] == 0).all()
        # SABS over the visible keys only (a row without one: 0)
        Ke = K.double().repeat_interleave(H // Hkv, 1)
        a = (Q.double().abs() @ Ke.abs().transpose(-1, -2) / 8).masked_fill(~vis, 0)
        assert torch.allclose(got["SABS"], a.amax(-1), rtol=1e-12, atol=0), w


@pytest.mark.parametrize("scale", [0.02, 1.0])
@pytest.mark.parametrize("H,Hkv", CHUNK_GROUPS, ids=["g1", "g4", "g32"])
def test_chunked_oracle_scale_equals_the_autograd_one(H, Hkv, scale):
    """scale= of attention_fp64_chunked against attention_fp64(scale=) (autograd) on repeat_interleave'd K/V, dK / dV
    summed per group; full and causal; the result differs from the default scale's (the argument is used)."""
    B, Sq, Sk, D = 2, 70, 50, 64
    g = torch.Generator().manual_seed(int(scale * 100) + H)
    Q, dO = (torch.randn(B, H, Sq, D, generator=g).to(torch.float16) for _ in range(2))
    K, V = (torch.randn(B, Hkv, Sk, D, generator=g).to(torch.float16) for _ in range(2))
    G = H // Hkv
    for causal in (False, True):
        want = fo.attention_fp64(Q, K.repeat_interleave(G, 1), V.repeat_interleave(G, 1), dO, causal, scale=scale)
        for n in ("dK", "dV"):
            want[n] = want[n].reshape(B, Hkv, G, Sk, D).sum(2)
        got = fo.attention_fp64_chunked(Q, K, V, dO, causal, max_bytes=3 * Sq * Sk * 8, scale=scale)
        for n in ("O", "LSE", "dQ", "dK", "dV", "delta"):
            _assert_same_fp64(got[n], want[n], (causal, n))
        a = (Q.double().abs() @ K.double().repeat_interleave(G, 1).abs().transpose(-1, -2) * scale)
        if causal:
            a = a.masked_fill(~fo.visible_mask(Sq, Sk, (-1, 0)), 0)
        assert torch.allclose(got["SABS"], a.amax(-1), rtol=1e-12, atol=0)
        dflt = fo.attention_fp64_chunked(Q, K, V, dO, causal)
        assert fo.rel_fro(dflt["O"], got["O"]) > 0.05


def test_scale_argument_of_the_other_fp64_oracles():
    """attention_fp64, attention_varlen_fp64 and attention_dropout_fp64 take scale=: S * scale is the same as the
    default-scale oracle on Q * scale * sqrt(D) (O, LSE, dK and dV up to rounding; dQ times the factor)."""
    B, H, S, D = 1, 2, 40, 64
    g = torch.Generator().manual_seed(11)
    Q, K, V, dO = (torch.randn(B, H, S, D, generator=g, dtype=torch.float64) for _ in range(4))
    scale = 0.3
    f = scale * D ** 0.5
    for causal in (False, True):
        got = fo.attention_fp64(Q, K, V, dO, causal, scale=scale)
        want = fo.attention_fp64(Q * f, K, V, dO, causal)
        for n in ("O", "LSE", "dK", "dV", "delta"):
            _assert_same_fp64(got[n], want[n], n)
        _assert_same_fp64(got["dQ"], want["dQ"] * f, "dQ")
        keep, rp = fo.dropout_keep_mask(B, H, S, S, 0.25, 5)
        got = fo.attention_dropout_fp64(Q, K, V, dO, causal, keep, rp, scale=scale)
        want = fo.attention_dropout_fp64(Q * f, K, V, dO, causal, keep, rp)
        for n in ("O", "LSE", "dK", "dV"):
            _assert_same_fp64(got[n], want[n], n)
        _assert_same_fp64(got["dQ"], want["dQ"] * f, "dQ")
    pk = lambda x: x[0].transpose(0, 1).contiguous()
    cu = [0, 15, 40]
    got = fo.attention_varlen_fp64(pk(Q), pk(K), pk(V), pk(dO), cu, cu, True, scale=scale)
    want = fo.attention_varlen_fp64(pk(Q * f), pk(K), pk(V), pk(dO), cu, cu, True)
    for n in ("O", "LSE", "dK", "dV"):
        _assert_same_fp64(got[n], want[n], n)
    _assert_same_fp64(got["dQ"], want["dQ"] * f, "dQ")


@pytest.mark.parametrize("Sq,Sk,offset", [(37, 50, 0), (131, 77, (1 << 32) - 1), (5, 3, 2)])
def test_torch_keep_mask_is_bit_identical_to_the_numpy_one(Sq, Sk, offset):
    """dropout_keep_mask_torch (exact 32-bit Philox on int64 tensors, the device references' mask) against
    dropout_keep_mask: odd S_q / S_k, a seed whose high word is set, offsets 0 and 2^32 - 1, every slice and sub-ranges of
    slices (a chunk of (batch, head) slices starts at its own counter)."""
    seed = 0xFEDCBA9876543210
    for p in (0.1, 0.5):
        want, rp = fo.dropout_keep_mask(3, 2, Sq, Sk, p, seed, offset)
        want = want.reshape(6, Sq, Sk)
        got, rp_t = fo.dropout_keep_mask_torch(0, 6, Sq, Sk, p, seed, offset)
        assert rp_t == rp and got.dtype == torch.bool and torch.equal(got, want)
        for a, b in ((2, 5), (5, 6)):
            assert torch.equal(fo.dropout_keep_mask_torch(a, b, Sq, Sk, p, seed, offset)[0], want[a:b])
    # the multiply-high / multiply-low split against Python integers at the extremes of 32 bits
    a = torch.tensor([0, 1, 0xFFFF, 0x10000, 0xFFFFFFFF, 0x80000000, 0x12345678], dtype=torch.int64)
    for m in (0xD2511F53, 0xCD9E8D57, 0xFFFFFFFF):
        hi, lo = fo._mul32(a, m)
        assert hi.tolist() == [(x * m) >> 32 for x in a.tolist()] and lo.tolist() == [(x * m) & 0xFFFFFFFF for x in a.tolist()]


@pytest.mark.parametrize("causal", [False, True])
def test_chunked_dropout_reference_equals_the_autograd_one(causal):
    """attention_fp64_chunked(dropout=(p, seed, offset)) -- the closed-form gradients with the device mask, several
    (batch, head) chunks -- against attention_dropout_fp64 (autograd) with dropout_keep_mask, S_q != S_k both ways; and
    the b0 element: batch b of the tensors takes the counter of batch b0 + b."""
    for Sq, Sk in ((70, 45), (45, 70)):
        B, H, D = 2, 3, 16
        Q, K, V, dO = rand_inputs(B, H, Sq, Sk, D, torch.float64, seed=Sq)
        p, seed, offset = 0.3, 0x8000000100000007, (1 << 32) - 1
        keep, rp = fo.dropout_keep_mask(B, H, Sq, Sk, p, seed, offset)
        want = fo.attention_dropout_fp64(Q, K, V, dO, causal, keep, rp)
        got = fo.attention_fp64_chunked(Q, K, V, dO, causal, max_bytes=2 * Sq * Sk * 8, dropout=(p, seed, offset))
        for n in ("O", "LSE", "dQ", "dK", "dV", "delta"):
            assert (got[n] - want[n]).abs().max() <= 1e-12 * max(want[n].abs().max().item(), 1.0), (Sq, Sk, n)
        one = fo.attention_fp64_chunked(Q[1:], K[1:], V[1:], dO[1:], causal, dropout=(p, seed, offset, 1))
        for n in ("O", "dQ", "dK", "dV"):
            assert (one[n] - want[n][1:]).abs().max() <= 1e-12 * max(want[n].abs().max().item(), 1.0), (Sq, Sk, n)


def test_one_wrong_keep_bit_clears_the_dropout_row_bound():
    """test_gpu_dropout.py checks fp16 O row by row because a block norm can hide one wrong keep bit.  At the paired
    case's S_k (4096, causal, p = 0.1 and 0.5), flipping one keep bit at a median-sized weight of the LAST row (the most
    keys, so the smallest weights) moves that row's relative error well past the row bound."""
    import test_gpu_dropout as td
    S, D = 4096, 64
    g = torch.Generator().manual_seed(3)
    q, v = torch.randn(D, generator=g, dtype=torch.float64), torch.randn(S, D, generator=g, dtype=torch.float64)
    k = torch.randn(S, D, generator=g, dtype=torch.float64)
    s = (k @ q) / D ** 0.5
    P = torch.softmax(s, 0)
    for p in (0.1, 0.5):
        keep, rp = fo.dropout_keep_mask_torch(0, 1, S, S, p, 0x8000000100000007, (1 << 32) - 1)
        kr = keep[0, -1].to(torch.float64) * rp
        O = (P * kr) @ v
        j = int(P.sort().indices[S // 2])
        flip = kr.clone()
        flip[j] = rp - flip[j]
        err = ((P * flip) @ v - O).norm() / O.norm()
        assert err > 3 * td.ROW_BOUND_F16, (p, err.item(), td.ROW_BOUND_F16)
