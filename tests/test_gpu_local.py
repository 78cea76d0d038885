"""GPU tests of sliding-window (local) attention (include/mi355fa_local.h, flash_attention_local): accuracy against the
fp64 masked attention of tests/attn_ref.py, degenerate windows against the existing kernels bit for bit, rows and keys
outside every band, strided views, packed variable-length batches, the bf16 q_scaled workspace and determinism.

Tolerances as in test_gpu_parity.py: fp16 relFro < 1e-3 against fp64; bf16 < max(2x PyTorch's own bf16 SDPA, 4e-3)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from attn_ref import attention_fp64, sdpa_bf16_level, visible
from fa_oracle import rel_fro

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
WINDOWS = [(0, 0), (1, 0), (63, 0), (64, 0), (200, 0), (127, 129), (0, 300), (-1, 17), (300, -1)]
SHAPES = [(1, 1), (77, 77), (500, 500), (1024, 1024), (333, 129), (129, 700)]


def _M():
    import My_FlashAttention_optimized as M
    return M


def check_close(gt, got, tol, what):
    """relFro < tol; where the fp64 reference is exactly zero (a one-key window: P = 1, so dS = 0 and dQ = dK = 0) only
    the kernel's rounding noise (delta comes from the 16-bit O) may remain."""
    assert not torch.isnan(got).any(), what
    if gt.abs().max() == 0:
        assert got.float().abs().max() < 1e-4, what
    else:
        assert rel_fro(gt, got) < tol, (what, rel_fro(gt, got), tol)


def rel_tol(dtype, level):
    """relFro bound of O, dQ, dK, dV (module docstring); level: PyTorch's own bf16 SDPA error on the same inputs"""
    return 1e-3 if dtype == F16 else max(2 * level, 4e-3)


def lse_tol(dtype):
    # bf16: the scores come from the scale-folded, bf16-rounded Q (fa_common.h kFoldScale): each product carries ~2^-9, so
    # a row that sees one key (LSE = its score) is off by up to ~1e-2 in absolute terms
    return 1e-3 if dtype == F16 else 1.5e-2


def run_local(Q, K, V, dO, wl, wr):
    """fwd + bwd through the C++ autograd function, plus LSE from the launcher; everything back on the CPU."""
    M = _M()
    q, k, v = (x.cuda().requires_grad_(True) for x in (Q, K, V))
    o = M.flash_attention_local(q, k, v, wl, wr)
    o.backward(dO.cuda())
    _, lse = M.flash_attention_local_forward(q.detach(), k.detach(), v.detach(), wl, wr)
    torch.cuda.synchronize()
    return {"O": o.detach().cpu(), "LSE": lse.cpu(), "dQ": q.grad.cpu(), "dK": k.grad.cpu(), "dV": v.grad.cpu()}


def inputs(B, H, Sq, Sk, D, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype)
    return mk(B, H, Sq, D), mk(B, H, Sk, D), mk(B, H, Sk, D), mk(B, H, Sq, D)


@pytest.fixture
def family1():
    import _mi355fa as fa
    fn = fa.lib.fa_debug_force_impl
    fn.argtypes = [ctypes.c_int] * 3
    fn.restype = None
    fn(1, 1, 1)
    yield
    fn(0, 0, 0)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("Sq,Sk", SHAPES)
def test_against_fp64(D, dtype, Sq, Sk):
    Q, K, V, dO = inputs(1, 2, Sq, Sk, D, dtype, seed=Sq + 7 * Sk + D)
    for wl, wr in WINDOWS:
        vis = visible(Sq, Sk, wl, wr, "cpu")
        gt = attention_fp64(Q, K, V, dO, D ** -0.5, vis)
        r = run_local(Q, K, V, dO, wl, wr)
        for n in ("O", "LSE", "dQ", "dK", "dV"):
            assert not torch.isnan(r[n]).any(), (n, wl, wr)
        fin = torch.isfinite(gt["LSE"])
        assert torch.equal(torch.isfinite(r["LSE"]), fin) and (r["LSE"][~fin] == float("-inf")).all(), (wl, wr)
        if fin.any():
            assert ((r["LSE"][fin].double() - gt["LSE"][fin]).abs() < lse_tol(dtype)).all(), (wl, wr)
        level = sdpa_bf16_level(Q, K, V, dO, vis, gt) if dtype == BF16 else None
        for n in ("O", "dQ", "dK", "dV"):
            check_close(gt[n], r[n], rel_tol(dtype, level and level[n]), (n, wl, wr))
        # the device's own SDPA with the same boolean mask, on the rows that see a key
        if fin.any():
            o_ref = F.scaled_dot_product_attention(Q.cuda(), K.cuda(), V.cuda(), attn_mask=vis.cuda()).float().cpu()
            rows = fin[0, 0]
            err = rel_fro(o_ref[:, :, rows], r["O"][:, :, rows].float())
            assert err < (2e-3 if dtype == F16 else 1e-2), (wl, wr, err)


def _all_outputs(fwd, Q, K, V, dO):
    """(O, LSE, dQ, dK, dV) of one launcher pair on device copies."""
    q, k, v, do = (x.cuda() for x in (Q, K, V, dO))
    return fwd(q, k, v, do)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("Sq,Sk", [(77, 77), (500, 500), (333, 129), (129, 700), (1024, 1024)])
def test_degenerate_windows_match_the_existing_kernels_bit_for_bit(family1, D, dtype, Sq, Sk):
    M = _M()
    Q, K, V, dO = inputs(2, 2, Sq, Sk, D, dtype, seed=3)
    q, k, v, do = (x.cuda() for x in (Q, K, V, dO))

    def plain(causal):
        O, L = M.flash_attention_forward(q, k, v, causal)
        return (O, L) + tuple(M.flash_attention_backward(q, k, v, O, do, L, causal))

    def local(wl, wr):
        O, L = M.flash_attention_local_forward(q, k, v, wl, wr)
        return (O, L) + tuple(M.flash_attention_local_backward(q, k, v, O, do, L, wl, wr))

    for (wl, wr), causal in (((-1, 0), True), ((Sq, 0), True), ((-1, -1), False), ((-1, Sk), False)):
        want, got = plain(causal), local(wl, wr)
        for n, a, b in zip(("O", "LSE", "dQ", "dK", "dV"), want, got):
            assert torch.equal(a, b), (n, wl, wr, (a != b).sum().item())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_rows_and_keys_outside_every_band_are_exactly_zero(dtype, D):
    for Sq, Sk, wl, wr in ((300, 100, 0, 0), (100, 300, 0, 0), (400, 150, 2, -1), (130, 500, 5, 3), (700, 64, 1, 1)):
        Q, K, V, dO = inputs(1, 2, Sq, Sk, D, dtype, seed=5)
        r = run_local(Q, K, V, dO, wl, wr)
        mask = visible(Sq, Sk, wl, wr, "cpu")
        rows, keys = ~mask.any(1), ~mask.any(0)
        for n in r:
            assert not torch.isnan(r[n]).any(), (n, Sq, Sk, wl, wr)
        assert rows.any() or keys.any()
        assert (r["O"][:, :, rows] == 0).all() and (r["dQ"][:, :, rows] == 0).all()
        assert (r["LSE"][:, :, rows] == float("-inf")).all()
        assert (r["dK"][:, :, keys] == 0).all() and (r["dV"][:, :, keys] == 0).all()
        gt = attention_fp64(Q, K, V, dO, D ** -0.5, mask)
        for n in ("O", "dQ", "dK", "dV"):
            check_close(gt[n], r[n], 1e-3 if dtype == F16 else 8e-3, (n, Sq, Sk, wl, wr))


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_bshd_views_are_read_in_place(dtype):
    M = _M()
    B, S, H, D, wl, wr = 2, 700, 4, 64, 100, 3
    base = [torch.randn(B, S, H, D, generator=torch.Generator().manual_seed(i)).to(dtype).cuda() for i in range(4)]
    q, k, v, do = (t.transpose(1, 2) for t in base)          # [B, H, S, D] views of [B, S, H, D] buffers
    assert not q.is_contiguous()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    O, L = M.flash_attention_local_forward(q, k, v, wl, wr)
    torch.cuda.synchronize()
    rnd = lambda n: (n + 511) // 512 * 512
    assert torch.cuda.memory_allocated() - before == rnd(O.numel() * O.element_size()) + rnd(L.numel() * 4)  # no input copy
    assert O.transpose(1, 2).is_contiguous()                  # O comes back in the input's memory order
    del O, L
    qa, ka, va = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = M.flash_attention_local(qa, ka, va, wl, wr)
    o.backward(do)
    qc, kc, vc = (t.detach().contiguous().requires_grad_(True) for t in (q, k, v))
    oc = M.flash_attention_local(qc, kc, vc, wl, wr)
    oc.backward(do.contiguous())
    assert torch.equal(o, oc)
    for a, b in ((qa, qc), (ka, kc), (va, vc)):
        assert torch.equal(a.grad, b.grad)


def _raw_local(fa, q, k, v, do, B, H, Sq, Sk, D, dt, wl, wr, opts_fwd, opts_bwd, o, lse, dq, dk, dv, delta):
    st = torch.cuda.current_stream().cuda_stream
    L = fa.lib
    sc = D ** -0.5
    fa.check(L.fa_fwd_local(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, Sq, Sk, D, dt, sc,
                            wl, wr, opts_fwd, st), "fwd_local")
    fa.check(L.fa_bwd_dq_local(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(),
                               dq.data_ptr(), delta.data_ptr(), B, H, Sq, Sk, D, dt, sc, wl, wr, opts_bwd, st), "dq_local")
    fa.check(L.fa_bwd_dkv_local(q.data_ptr(), k.data_ptr(), v.data_ptr(), do.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                dk.data_ptr(), dv.data_ptr(), B, H, Sq, Sk, D, dt, sc, wl, wr, opts_bwd, st), "dkv_local")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_varlen_matches_each_sequence_alone(dtype, D):
    """Packed sequences through the C ABI with cu_seqlens (one sequence without queries, one without keys): every sequence
    equals a fixed-length local launch of that sequence alone, bit for bit.  bf16 runs with the q_scaled workspace."""
    import _mi355fa as fa
    H, wl, wr = 2, 90, 5
    lq, lk = [37, 0, 200, 129, 64], [37, 50, 260, 300, 0]
    cq = torch.tensor([0] + list(torch.tensor(lq).cumsum(0)), dtype=torch.int32)
    ck = torch.tensor([0] + list(torch.tensor(lk).cumsum(0)), dtype=torch.int32)
    tq, tk = int(cq[-1]), int(ck[-1])
    g = torch.Generator().manual_seed(11)
    mk = lambda n: torch.randn(n, H, D, generator=g).to(dtype).cuda()
    q, do, k, v = mk(tq), mk(tq), mk(tk), mk(tk)
    o, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    lse, delta = torch.empty(H, tq, device="cuda"), torch.empty(H, tq, device="cuda")
    ws = torch.empty_like(q)
    cqd, ckd = cq.cuda(), ck.cuda()
    dt = fa.BF16 if dtype == BF16 else fa.FP16
    vo = fa.Opts.make(cu_seqlens_q=cqd.data_ptr(), cu_seqlens_k=ckd.data_ptr(), total_q=tq, total_k=tk)
    vb = fa.Opts.make(cu_seqlens_q=cqd.data_ptr(), cu_seqlens_k=ckd.data_ptr(), total_q=tq, total_k=tk,
                      q_scaled=ws.data_ptr())
    _raw_local(fa, q, k, v, do, len(lq), H, max(lq), max(lk), D, dt, wl, wr, ctypes.byref(vo), ctypes.byref(vb),
               o, lse, dq, dk, dv, delta)
    torch.cuda.synchronize()
    for b in range(len(lq)):
        qs, ks = slice(int(cq[b]), int(cq[b + 1])), slice(int(ck[b]), int(ck[b + 1]))
        if lq[b] == 0:
            assert (dk[ks] == 0).all() and (dv[ks] == 0).all()
            continue
        if lk[b] == 0:
            assert (o[qs] == 0).all() and (dq[qs] == 0).all() and (lse[:, qs] == float("-inf")).all()
            continue
        one = lambda t, s: t[s].transpose(0, 1).unsqueeze(0).contiguous()     # [1, H, S, D]
        q1, k1, v1, do1 = one(q, qs), one(k, ks), one(v, ks), one(do, qs)
        o1, dq1, dk1, dv1 = (torch.empty_like(x) for x in (q1, q1, k1, v1))
        l1, d1 = torch.empty(1, H, lq[b], device="cuda"), torch.empty(1, H, lq[b], device="cuda")
        ws1 = torch.empty_like(q1)
        _raw_local(fa, q1, k1, v1, do1, 1, H, lq[b], lk[b], D, dt, wl, wr, None,
                   ctypes.byref(fa.Opts.make(q_scaled=ws1.data_ptr())), o1, l1, dq1, dk1, dv1, d1)
        torch.cuda.synchronize()
        back = lambda t: t[0].transpose(0, 1)
        assert torch.equal(o[qs], back(o1)) and torch.equal(lse[:, qs], l1[0]), b
        assert torch.equal(dq[qs], back(dq1)) and torch.equal(dk[ks], back(dk1)) and torch.equal(dv[ks], back(dv1)), b


def test_bf16_workspace_path_and_determinism():
    """The autograd path passes the q_scaled workspace for bf16; the plain C call without it must agree to bf16 accuracy,
    and two launches of either are bit-identical."""
    import _mi355fa as fa
    B, H, S, D, wl, wr = 2, 4, 1000, 64, 255, 0
    Q, K, V, dO = inputs(B, H, S, S, D, BF16, seed=9)
    r1, r2 = run_local(Q, K, V, dO, wl, wr), run_local(Q, K, V, dO, wl, wr)
    for n in r1:
        assert torch.equal(r1[n], r2[n]), n
    q, k, v, do = (x.cuda() for x in (Q, K, V, dO))
    o, dq, dk, dv = (torch.empty_like(x) for x in (q, q, k, v))
    lse, delta = torch.empty(B, H, S, device="cuda"), torch.empty(B, H, S, device="cuda")
    _raw_local(fa, q, k, v, do, B, H, S, S, D, fa.BF16, wl, wr, None, None, o, lse, dq, dk, dv, delta)
    torch.cuda.synchronize()
    assert torch.equal(o.cpu(), r1["O"]) and torch.equal(dq.cpu(), r1["dQ"])      # the workspace only changes dK / dV
    gt = attention_fp64(Q, K, V, dO, D ** -0.5, visible(S, S, wl, wr, "cpu"))
    for n, t in (("dK", dk), ("dV", dv)):
        assert rel_fro(gt[n], t.cpu()) < 8e-3 and rel_fro(gt[n], r1[n]) < 8e-3, n


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_python_class_matches_the_cpp_function(dtype):
    M = _M()
    Q, K, V, dO = inputs(2, 3, 333, 500, 128, dtype, seed=4)
    outs = []
    for fn in (lambda q, k, v: M.flash_attention_local(q, k, v, 63, 17),
               lambda q, k, v: M.FlashAttentionLocalFunction.apply(q, k, v, 63, 17)):
        q, k, v = (x.cuda().requires_grad_(True) for x in (Q, K, V))
        o = fn(q, k, v)
        o.backward(dO.cuda())
        outs.append((o.detach(), q.grad, k.grad, v.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_dropout_with_a_window_is_refused():
    import _mi355fa as fa
    q = torch.randn(1, 1, 64, 64, dtype=F16, device="cuda")
    o, lse = torch.empty_like(q), torch.empty(1, 1, 64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = fa.lib.fa_fwd_local(q.data_ptr(), q.data_ptr(), q.data_ptr(), o.data_ptr(), lse.data_ptr(), 1, 1, 64, 64, 64, fa.FP16,
                             0.125, 8, 0, ctypes.byref(fa.Opts.make(p_drop=0.1)), st)
    assert rc == -2
