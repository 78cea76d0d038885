"""GPU tests of the ALiBi bias (include/mi355fa_alibi.h): O, LSE, dQ, dK and dV of the ALiBi GQA / window kernels and the
ALiBi decode kernel against the fp64 reference of tests/attn_ref.py, computed on the device.

Every case is checked four ways, as test_gpu_softcap.py: relFro per output against the suite's per-feature bounds (1e-3
fp16, 8e-3 bf16; bf16 dK / dV without the q_scaled workspace: RAW_BF16_DKV), block by block with
blockcheck.check_outputs (bounds below), LSE row by row, and exact zeros where fp64 has them.  Every case also requires
the kernel's O to be far from the UNBIASED attention of the same inputs (relFro >= BIAS_MATTERS), so a kernel that ignores
the slopes fails.  Zero slopes must give the bits of flash_attention_gqa."""
import pytest
import torch

import attn_ref as ar
import blockcheck as bc
import variantcheck as vck
from variantcheck import formula_splits   # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
REL = {F16: 1e-3, BF16: 8e-3}
RAW_BF16_DKV = 3e-2
BIAS_MATTERS = 0.05
# per-block bounds (blockcheck.check_outputs): about 1.5x the largest block error measured on an MI355X over every case in
# this file (fp16 O 3.02e-4, dQ 4.60e-4, dK 3.78e-4, dV 3.20e-4; bf16 O 2.94e-3, dQ 4.11e-3, dK 3.72e-3, dV 2.94e-3; bf16
# dK / dV without the workspace 4.07e-3)
BLOCK_BOUND = {
    (F16, "O"): 4.5e-4, (F16, "dQ"): 7e-4, (F16, "dK"): 5.7e-4, (F16, "dV"): 4.8e-4,
    (BF16, "O"): 4.5e-3, (BF16, "dQ"): 6.2e-3, (BF16, "dK"): 5.6e-3, (BF16, "dV"): 4.5e-3,
}
# LSE per row: |LSE - fp64| <= a + u * max |s| of the row (s: the biased scores); the suite's soft-capping bounds (largest
# block error measured: fp16 2.85e-6, bf16 5.90e-3)
BOUNDS = dict(BLOCK_BOUND=BLOCK_BOUND, BLOCK_BOUND_RAW_BF16_DKV=6.1e-3, FEW_BOUND={F16: 1e-2, BF16: 1e-1}, RATIO=4.0,
              FLOOR=1e-5, LSE_BOUND={F16: (2e-4, 2.0 ** -16), BF16: (1.5e-2, 2.0 ** -8)}, DELTA_BOUND=1e-6)


def _slopes(kind, B, H):
    """geometric: the paper's; steep: 2x them (the bias dominates the unit-variance scores beyond a few positions; much
    steeper, a row's softmax is one-hot on the diagonal and dQ / dK are pure cancellation); neg: negative slopes, the bias
    grows with the distance; per-batch: (B, H), each sequence its own multiple of the paper's"""
    s = vck.M().alibi_slopes(H, device="cuda")
    if kind == "steep":
        return s * 2
    if kind == "neg":
        return -s / 16
    if kind == "batch":
        return (s[None, :] * torch.linspace(0.25, 2.0, B, device="cuda")[:, None]).contiguous()
    return s


def _autograd(Q, K, V, dO, slopes, window):
    call = lambda q, k, v: vck.M().flash_attention_alibi(q, k, v, slopes, window_size=window)
    return vck.autograd_run(call, Q, K, V, dO)


def _raw(Q, K, V, dO, slopes, window, scale, workspace):
    extra = (slopes.data_ptr(), Q.shape[1] if slopes.dim() == 2 else 0)
    return vck.raw_run(("fa_fwd_alibi", "fa_bwd_dq_alibi", "fa_bwd_dkv_alibi"), extra, Q, K, V, dO, window, scale, workspace)


def _check(tag, gt, got, dO, dtype, mode, unb=None, few=None):
    """vck.check_training under this file's bounds; the bias must matter."""
    return vck.check_training(tag, gt, got, dO, dtype, mode, REL, RAW_BF16_DKV, BOUNDS, unb, BIAS_MATTERS, few)


# dtype, D, H, H_kv, S_q, S_k, window, slopes, strided
CASES = [
    ("fp16-d64-mha-full-geo", F16, 64, 4, 4, 256, 256, (-1, -1), "geo", False),
    ("bf16-d64-gqa4-causal-batch-ragged", BF16, 64, 8, 2, 200, 333, (-1, 0), "batch", False),
    ("fp16-d128-mqa-w127-steep", F16, 128, 4, 1, 384, 384, (127, 0), "steep", False),
    ("bf16-d128-gqa4-w64x64-geo", BF16, 128, 8, 2, 256, 256, (64, 64), "geo", False),
    ("fp16-d128-gqa4-causal-batch-strided", F16, 128, 8, 2, 300, 300, (-1, 0), "batch", True),
    ("bf16-d64-mqa-full-steep-sq<sk", BF16, 64, 4, 1, 128, 200, (-1, -1), "steep", False),
    ("fp16-d64-gqa4-w127-geo-sq>sk", F16, 64, 4, 1, 333, 200, (127, 0), "geo", False),
    ("bf16-d128-mha-full-neg", BF16, 128, 4, 4, 256, 256, (-1, -1), "neg", False),
    ("fp16-d64-mha-causal-neg", F16, 64, 2, 2, 256, 256, (-1, 0), "neg", False),
    ("bf16-d128-gqa4-causal-steep", BF16, 128, 8, 2, 512, 512, (-1, 0), "steep", False),
    # head groups that are no power of two: g = 3, and g = 7 as multi-query (the slope of head h / g's neighbours)
    ("fp16-d128-g3-w64x40-batch-ragged", F16, 128, 6, 2, 301, 211, (64, 40), "batch", False),   # rows 275.. see no key
    ("bf16-d64-g7-causal-geo-ragged", BF16, 64, 7, 1, 233, 333, (-1, 0), "geo", False),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_alibi_matches_fp64(case):
    tag, dtype, D, H, Hkv, Sq, Sk, window, kind, strided = case
    scale = D ** -0.5
    B = 2
    Q, K, V, dO = vck.inputs(B, H, Hkv, Sq, Sk, D, dtype, seed=Sq + Sk + D)
    slopes = _slopes(kind, B, H)
    vis = ar.visible(Sq, Sk, window[0], window[1], "cuda")
    dist = ar.distance(Sq, Sk, "cuda")
    gt = ar.attention_fp64(Q, K, V, dO, scale, vis, slopes=slopes, dist=dist)
    unb = ar.attention_fp64(Q, K, V, None, scale, vis)["O"]
    if strided:   # [B, S, H, D] buffers seen as [B, H, S, D]: read in place, the same bits as contiguous tensors
        Qs, Ks, Vs = (x.transpose(1, 2).contiguous().transpose(1, 2) for x in (Q, K, V))
        got = _autograd(Qs, Ks, Vs, dO, slopes, window)
        ref = _autograd(Q, K, V, dO, slopes, window)
        for n in got:
            assert bc.same_bits(got[n], ref[n]), (tag, n)
    few = bc.few_rows(vis)
    got = _autograd(Q, K, V, dO, slopes, window)
    _check(tag + " autograd", gt, got, dO, dtype, "ws", unb, few)
    raw = _raw(Q, K, V, dO, slopes, window, scale, workspace=False)
    _check(tag + " raw", gt, raw, dO, dtype, "raw", unb, few)
    if dtype == BF16:
        ws = _raw(Q, K, V, dO, slopes, window, scale, workspace=True)
        _check(tag + " ws", gt, ws, dO, dtype, "ws", unb, few)
        assert bc.same_bits(ws["O"], raw["O"])   # the workspace changes the backward only


@pytest.mark.parametrize("dtype,D", [(F16, 64), (BF16, 64), (F16, 128), (BF16, 128)])
def test_zero_slopes_give_the_gqa_bits(dtype, D):
    """Zero slopes reproduce flash_attention_gqa bit for bit: O, LSE, dQ, dK and dV (fma(0, -|d|, x) = x)."""
    M = vck.M()
    Q, K, V, dO = vck.inputs(2, 8, 2, 300, 333, D, dtype, seed=D + 1)
    zero = torch.zeros(8, device="cuda")
    for window in ((-1, -1), (-1, 0), (100, 20)):
        a = _autograd(Q, K, V, dO, zero, window)
        q, k, v = (x.detach().clone().requires_grad_(True) for x in (Q, K, V))
        o = M.flash_attention_gqa(q, k, v, window_size=window)
        o.backward(dO)
        torch.cuda.synchronize()
        for n, t in (("O", o.detach()), ("dQ", q.grad), ("dK", k.grad), ("dV", v.grad)):
            assert bc.same_bits(a[n], t), (dtype, D, window, n)
        wl, wr = window
        la = M.flash_attention_alibi_forward(Q, K, V, zero, wl, wr)[1]
        lg = M.flash_attention_gqa_forward(Q, K, V, wl, wr)[1]
        torch.cuda.synchronize()
        assert bc.same_bits(la, lg), (dtype, D, window, "LSE")


def test_packed_batch_with_an_empty_sequence():
    dtype, D, H, Hkv = BF16, 64, 4, 2
    lens = [(130, 70), (0, 50), (64, 0), (257, 300), (5, 5)]
    slopes = _slopes("batch", len(lens), H)
    call = lambda q, k, v, **kw: vck.M().flash_attention_alibi(q, k, v, slopes, **kw)
    truth_kw = lambda i, a, b: dict(slopes=slopes[i], dist=ar.distance(a, b, "cuda"))
    got, gt, _ = vck.packed_case(call, truth_kw, lambda a, b: a == 0 or b == 0, lens, dtype, D, H, Hkv, seed=7)
    vck.check_packed(got, gt, REL[dtype])
    print("packed", "ok")


def test_slopes_get_no_gradient():
    M = vck.M()
    Q, K, V, dO = vck.inputs(1, 4, 2, 128, 128, 64, F16, seed=9)
    q = Q.clone().requires_grad_(True)
    o = M.flash_attention_alibi(q, K, V, _slopes("geo", 1, 4), is_causal=True)
    o.backward(dO)
    assert q.grad is not None
    with pytest.raises(AssertionError, match="grad"):
        M.flash_attention_alibi(q, K, V, _slopes("geo", 1, 4).requires_grad_(True))


def test_deterministic():
    Q, K, V, dO = vck.inputs(2, 8, 2, 200, 333, 128, BF16, seed=3)
    sl = _slopes("batch", 2, 8)
    a = _autograd(Q, K, V, dO, sl, (-1, 0))
    b = _autograd(Q, K, V, dO, sl, (-1, 0))
    for n in a:
        assert bc.same_bits(a[n], b[n]), n


@pytest.mark.parametrize("dtype,D,Sq,window,kind", [(F16, 128, 1, (-1, -1), "geo"), (BF16, 64, 4, (200, 0), "batch"),
                                                    (BF16, 128, 3, (-1, 0), "steep")])
def test_decode_matches_fp64(dtype, D, Sq, window, kind, formula_splits):
    slopes = _slopes(kind, 3, 8) / 8   # decode reads up to 650 keys: the slopes / 8 keep many keys in play
    call = lambda q, kc, vc, sl, **kw: vck.M().flash_attention_kvcache_alibi(q, kc, vc, sl, slopes, **kw)
    dist = lambda Ls: torch.stack([ar.distance(Sq, vck.DECODE_CACHE, "cuda", L=L) for L in Ls])[:, None]
    res = vck.decode_case(call, lambda Ls: dict(slopes=slopes, dist=dist(Ls)), dtype, D, Sq, window, REL[dtype], BIAS_MATTERS,
                          BOUNDS["LSE_BOUND"][dtype])
    for n, err, lerr in res:
        print("decode", dtype, D, Sq, window, kind, "splits", n, "O relFro %.2e LSE max %.2e" % (err, lerr))


def test_decode_graph_replay():
    """One captured decode step, replayed after cache_seqlens and the slopes change in place: each replay matches an
    eager call with the new values (the host never reads either)."""
    B, H, Hkv, Sq, Sc, D = 2, 8, 2, 1, 1024, 128
    g = torch.Generator(device="cuda").manual_seed(5)
    q = torch.randn(B, H, Sq, D, device="cuda", generator=g).to(BF16)
    kc, vc = (torch.randn(B, Hkv, Sc, D, device="cuda", generator=g).to(BF16) for _ in range(2))
    sl = torch.tensor([700, 1000], dtype=torch.int32, device="cuda")
    base = _slopes("batch", B, H) / 8
    call = lambda s: vck.M().flash_attention_kvcache_alibi(q, kc, vc, sl, s)
    vck.graph_replay(call, sl, [([700, 1000], base), ([300, 1024], base * 2.0), ([1, 512], base * 0.5)], extra=base.clone())
