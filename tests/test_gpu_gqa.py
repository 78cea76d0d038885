"""GPU tests of grouped-query attention (include/mi355fa_gqa.h, flash_attention_gqa): accuracy against the fp64 attention
of tests/attn_ref.py (repeat_interleave'd K/V, dK / dV summed per group), O / LSE / dQ bit for bit against the existing
kernels on the materialised K/V, determinism, strided views read in place, packed variable-length batches, the bf16
q_scaled workspace and the Python twin.

Tolerances as in test_gpu_local.py: fp16 relFro < 1e-3 against fp64; bf16 < max(2x PyTorch's own bf16 SDPA, 4e-3)."""
import ctypes

import pytest
import torch

from attn_ref import attention_fp64, sdpa_bf16_level, visible
from fa_oracle import rel_fro

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
# (H, H_kv): g = 1, 2, 4 and H (multi-query); then groups that are no power of two: g = 3, 7 (multi-query) and 6
GROUPS = [(4, 4), (4, 2), (8, 2), (4, 1), (6, 2), (7, 1), (12, 2)]
GROUP_IDS = ["g1", "g2", "g4", "mqa", "g3", "g7-mqa", "g6"]
MASKS = [(-1, -1), (-1, 0), (100, 0), (70, 70)]   # full, causal, (w, 0), (w, w)
SHAPES = [(333, 129), (129, 700), (500, 500)]     # S_q != S_k, ragged tails


def _M():
    import My_FlashAttention_optimized as M
    return M


def inputs(B, H, Hkv, Sq, Sk, D, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype)
    return mk(B, H, Sq, D), mk(B, Hkv, Sk, D), mk(B, Hkv, Sk, D), mk(B, H, Sq, D)


def window_of(wl, wr):
    return {"is_causal": True} if (wl, wr) == (-1, 0) else {"window_size": (wl, wr)}


def run_gqa(Q, K, V, dO, wl, wr):
    """fwd + bwd through flash_attention_gqa (C++ autograd function), LSE from the launcher; everything on the CPU."""
    M = _M()
    q, k, v = (x.cuda().requires_grad_(True) for x in (Q, K, V))
    o = M.flash_attention_gqa(q, k, v, **window_of(wl, wr))
    o.backward(dO.cuda())
    _, lse = M.flash_attention_gqa_forward(q.detach(), k.detach(), v.detach(), wl, wr)
    torch.cuda.synchronize()
    return {"O": o.detach().cpu(), "LSE": lse.cpu(), "dQ": q.grad.cpu(), "dK": k.grad.cpu(), "dV": v.grad.cpu()}


def run_expanded(Q, K, V, dO, wl, wr):
    """The path a GQA caller has without this feature: repeat_interleave K/V, the MHA function, autograd's group sum."""
    M = _M()
    g = Q.shape[1] // K.shape[1]
    q, k, v = (x.cuda().requires_grad_(True) for x in (Q, K, V))
    ke, ve = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    if (wl, wr) in ((-1, -1), (-1, 0)):
        o = M.flash_attention(q, ke, ve, is_causal=(wr == 0))
    else:
        o = M.flash_attention_local(q, ke, ve, wl, wr)
    o.backward(dO.cuda())
    torch.cuda.synchronize()
    return {"O": o.detach().cpu(), "dQ": q.grad.cpu(), "dK": k.grad.cpu(), "dV": v.grad.cpu()}


@pytest.fixture
def family1():
    import _mi355fa as fa
    fn = fa.lib.fa_debug_force_impl
    fn.argtypes = [ctypes.c_int] * 3
    fn.restype = None
    fn(1, 1, 1)
    yield
    fn(0, 0, 0)


@pytest.mark.parametrize("H,Hkv", GROUPS, ids=GROUP_IDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_against_fp64(H, Hkv, D, dtype):
    for Sq, Sk in SHAPES:
        Q, K, V, dO = inputs(1, H, Hkv, Sq, Sk, D, dtype, seed=Sq + 7 * Sk + D + H + Hkv)
        for wl, wr in MASKS:
            vis = visible(Sq, Sk, wl, wr, "cpu")
            gt = attention_fp64(Q, K, V, dO, D ** -0.5, vis)
            r = run_gqa(Q, K, V, dO, wl, wr)
            assert r["dK"].shape == K.shape and r["dV"].shape == V.shape
            for n in r:
                assert not torch.isnan(r[n]).any(), (n, wl, wr)
            fin = torch.isfinite(gt["LSE"])
            assert torch.equal(torch.isfinite(r["LSE"]), fin), (wl, wr)
            lse_tol = 1e-3 if dtype == F16 else 1.5e-2
            assert ((r["LSE"][fin].double() - gt["LSE"][fin]).abs() < lse_tol).all(), (wl, wr)
            level = sdpa_bf16_level(Q, K, V, dO, vis, gt) if dtype == BF16 else None
            errs = {n: rel_fro(gt[n], r[n]) for n in ("O", "dQ", "dK", "dV")}
            for n, e in errs.items():
                assert e < (1e-3 if dtype == F16 else max(2 * level[n], 4e-3)), (n, Sq, Sk, wl, wr, e)
            # the group sum in fp32 is no less accurate than the expanded path's 16-bit per-head gradients summed by
            # autograd (5% margin for noise; at g = 1 there is no sum, both are one rounding of different kernels: 25%)
            b = run_expanded(Q, K, V, dO, wl, wr)
            margin = 1.05 if H > Hkv else 1.25
            for n in ("dK", "dV"):
                eb = rel_fro(gt[n], b[n])
                assert errs[n] <= margin * eb + 1e-7, (n, Sq, Sk, wl, wr, errs[n], eb)


@pytest.mark.parametrize("H,Hkv", GROUPS, ids=GROUP_IDS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_matches_the_existing_kernels_on_materialised_kv_bit_for_bit(family1, H, Hkv, D, dtype):
    M = _M()
    Sq, Sk = 333, 500
    g = H // Hkv
    Q, K, V, dO = inputs(2, H, Hkv, Sq, Sk, D, dtype, seed=3)
    q, k, v, do = (x.cuda() for x in (Q, K, V, dO))
    ke, ve = k.repeat_interleave(g, 1).contiguous(), v.repeat_interleave(g, 1).contiguous()
    for wl, wr in MASKS:
        O, L = M.flash_attention_gqa_forward(q, k, v, wl, wr)
        dQ, dK, dV = M.flash_attention_gqa_backward(q, k, v, O, do, L, wl, wr)
        if (wl, wr) in ((-1, -1), (-1, 0)):
            O2, L2 = M.flash_attention_forward(q, ke, ve, wr == 0)
            dQ2, dK2, dV2 = M.flash_attention_backward(q, ke, ve, O2, do, L2, wr == 0)
        else:
            O2, L2 = M.flash_attention_local_forward(q, ke, ve, wl, wr)
            dQ2, dK2, dV2 = M.flash_attention_local_backward(q, ke, ve, O2, do, L2, wl, wr)
        for n, a, b in (("O", O, O2), ("LSE", L, L2), ("dQ", dQ, dQ2)):
            assert torch.equal(a, b), (n, wl, wr, (a != b).sum().item())
        if g == 1:
            assert torch.equal(dK, dK2) and torch.equal(dV, dV2), (wl, wr)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_gradients_are_deterministic(dtype):
    Q, K, V, dO = inputs(2, 8, 2, 700, 700, 64, dtype, seed=9)
    for wl, wr in ((-1, 0), (100, 0)):
        r1, r2 = run_gqa(Q, K, V, dO, wl, wr), run_gqa(Q, K, V, dO, wl, wr)
        for n in r1:
            assert torch.equal(r1[n], r2[n]), (n, wl, wr)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_bshd_views_are_read_in_place(dtype):
    M = _M()
    B, S, H, Hkv, D, wl, wr = 2, 700, 8, 2, 64, 100, 0
    mk = lambda h, i: torch.randn(B, S, h, D, generator=torch.Generator().manual_seed(i)).to(dtype).cuda()
    q, k, v, do = (t.transpose(1, 2) for t in (mk(H, 0), mk(Hkv, 1), mk(Hkv, 2), mk(H, 3)))   # [B, S, h, D] buffers
    assert not q.is_contiguous() and not k.is_contiguous()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    O, L = M.flash_attention_gqa_forward(q, k, v, wl, wr)
    torch.cuda.synchronize()
    rnd = lambda n: (n + 511) // 512 * 512
    assert torch.cuda.memory_allocated() - before == rnd(O.numel() * O.element_size()) + rnd(L.numel() * 4)  # no input copy
    assert O.transpose(1, 2).is_contiguous()                  # O comes back in the input's memory order
    dQ, dK, dV = M.flash_attention_gqa_backward(q, k, v, O, do, L, wl, wr)
    for grad, leaf in ((dQ, q), (dK, k), (dV, v)):            # gradients in the leaves' [B, S, h, D] order
        assert grad.shape == leaf.shape and grad.stride() == leaf.stride()
    del O, L
    qa, ka, va = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = M.flash_attention_gqa(qa, ka, va, window_size=(wl, wr))
    o.backward(do)
    qc, kc, vc = (t.detach().contiguous().requires_grad_(True) for t in (q, k, v))
    oc = M.flash_attention_gqa(qc, kc, vc, window_size=(wl, wr))
    oc.backward(do.contiguous())
    assert torch.equal(o, oc)
    for a, b in ((qa, qc), (ka, kc), (va, vc)):
        assert torch.equal(a.grad, b.grad)
    assert torch.equal(dK, ka.grad) and torch.equal(dQ, qa.grad)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_varlen_matches_each_sequence_alone(dtype, D):
    """Packed sequences (one without queries, one without keys) through flash_attention_gqa's cu_seqlens form: every
    sequence equals a fixed-length GQA launch of that sequence alone, bit for bit."""
    M = _M()
    H, Hkv, wl, wr = 8, 2, 90, 0
    lq, lk = [37, 0, 200, 129, 64], [37, 50, 260, 300, 0]
    cq = torch.tensor([0] + list(torch.tensor(lq).cumsum(0)), dtype=torch.int32)
    ck = torch.tensor([0] + list(torch.tensor(lk).cumsum(0)), dtype=torch.int32)
    tq, tk = int(cq[-1]), int(ck[-1])
    g = torch.Generator().manual_seed(11)
    mk = lambda n, h: torch.randn(n, h, D, generator=g).to(dtype).cuda()
    q, do, k, v = mk(tq, H), mk(tq, H), mk(tk, Hkv), mk(tk, Hkv)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = M.flash_attention_gqa(qa, ka, va, window_size=(wl, wr), cu_seqlens_q=cq.cuda(), cu_seqlens_k=ck.cuda(),
                              max_seqlen_q=max(lq), max_seqlen_k=max(lk))
    o.backward(do)
    torch.cuda.synchronize()
    assert ka.grad.shape == k.shape
    for b in range(len(lq)):
        qs, ks = slice(int(cq[b]), int(cq[b + 1])), slice(int(ck[b]), int(ck[b + 1]))
        if lq[b] == 0:
            assert (ka.grad[ks] == 0).all() and (va.grad[ks] == 0).all()
            continue
        if lk[b] == 0:
            assert (o[qs] == 0).all() and (qa.grad[qs] == 0).all()
            continue
        one = lambda t, s: t[s].transpose(0, 1).unsqueeze(0).contiguous().requires_grad_(True)    # [1, h, S, D]
        q1, k1, v1 = one(q, qs), one(k, ks), one(v, ks)
        o1 = M.flash_attention_gqa(q1, k1, v1, window_size=(wl, wr))
        o1.backward(do[qs].transpose(0, 1).unsqueeze(0).contiguous())
        back = lambda t: t[0].transpose(0, 1)
        assert torch.equal(o[qs], back(o1)), b
        assert torch.equal(qa.grad[qs], back(q1.grad)), b
        assert torch.equal(ka.grad[ks], back(k1.grad)) and torch.equal(va.grad[ks], back(v1.grad)), b


def test_bf16_workspace_path_at_large_scores():
    """bf16 autograd passes the Q-sized q_scaled workspace: dK / dV recomputed from the Q the forward used stay within
    bf16 accuracy of fp64 when the scores are large; the raw C call without the workspace gives the same O and dQ."""
    import _mi355fa as fa
    M = _M()
    B, H, Hkv, S, D, wl, wr = 1, 8, 2, 600, 64, 255, 0
    Q, K, V, dO = inputs(B, H, Hkv, S, S, D, BF16, seed=21)
    Q, K = (Q.float() * 3).to(BF16), (K.float() * 3).to(BF16)        # |scores| up to ~100
    r = run_gqa(Q, K, V, dO, wl, wr)
    vis = visible(S, S, wl, wr, "cpu")
    gt = attention_fp64(Q, K, V, dO, D ** -0.5, vis)
    level = sdpa_bf16_level(Q, K, V, dO, vis, gt)
    for n in ("dK", "dV"):   # what the workspace changes (O and dQ: bit-identical to the MHA kernels, tested above)
        assert rel_fro(gt[n], r[n]) < max(2 * level[n], 8e-3), (n, rel_fro(gt[n], r[n]), level[n])
    q, k, v, do = (x.cuda() for x in (Q, K, V, dO))
    o, dq, dk, dv = (torch.empty_like(x) for x in (q, q, k, v))
    lse, delta = torch.empty(B, H, S, device="cuda"), torch.empty(B, H, S, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L, sc = fa.lib, D ** -0.5
    fa.check(L.fa_fwd_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, Hkv, S, S, D, fa.BF16,
                          sc, wl, wr, None, st), "fwd_gqa")
    fa.check(L.fa_bwd_dq_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(),
                             dq.data_ptr(), delta.data_ptr(), B, H, Hkv, S, S, D, fa.BF16, sc, wl, wr, None, st), "dq_gqa")
    fa.check(L.fa_bwd_dkv_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), do.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                              dk.data_ptr(), dv.data_ptr(), B, H, Hkv, S, S, D, fa.BF16, sc, wl, wr, None, st), "dkv_gqa")
    torch.cuda.synchronize()
    assert torch.equal(o.cpu(), r["O"]) and torch.equal(dq.cpu(), r["dQ"])   # the workspace only changes dK / dV


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_python_class_matches_the_cpp_function(dtype):
    M = _M()
    Q, K, V, dO = inputs(2, 6, 2, 333, 500, 128, dtype, seed=4)
    outs = []
    for fn in (lambda q, k, v: M.flash_attention_gqa(q, k, v, window_size=(63, 17)),
               lambda q, k, v: M.FlashAttentionGQAFunction.apply(q, k, v, 63, 17)):
        q, k, v = (x.cuda().requires_grad_(True) for x in (Q, K, V))
        o = fn(q, k, v)
        o.backward(dO.cuda())
        outs.append((o.detach(), q.grad, k.grad, v.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # and the packed form
    cq = torch.tensor([0, 100, 333], dtype=torch.int32, device="cuda")
    ck = torch.tensor([0, 200, 500], dtype=torch.int32, device="cuda")
    pk = lambda t: t[0].transpose(0, 1).contiguous().cuda()
    outs = []
    for fn in (lambda q, k, v: M.flash_attention_gqa(q, k, v, is_causal=True, cu_seqlens_q=cq, cu_seqlens_k=ck,
                                                      max_seqlen_q=233, max_seqlen_k=300),
               lambda q, k, v: M.FlashAttentionGQAFunction.apply(q, k, v, -1, 0, cq, ck, 233, 300)):
        q, k, v = (pk(x).requires_grad_(True) for x in (Q, K, V))
        o = fn(q, k, v)
        o.backward(pk(dO))
        outs.append((o.detach(), q.grad, k.grad, v.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_dropout_is_refused():
    import _mi355fa as fa
    q = torch.randn(1, 2, 64, 64, dtype=F16, device="cuda")
    k = torch.randn(1, 1, 64, 64, dtype=F16, device="cuda")
    o, lse = torch.empty_like(q), torch.empty(1, 2, 64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = fa.lib.fa_fwd_gqa(q.data_ptr(), k.data_ptr(), k.data_ptr(), o.data_ptr(), lse.data_ptr(), 1, 2, 1, 64, 64, 64,
                           fa.FP16, 0.125, -1, 0, ctypes.byref(fa.Opts.make(p_drop=0.1)), st)
    assert rc == -2
