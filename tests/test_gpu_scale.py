"""Every entry point at a softmax scale other than 1/sqrt(D), against the fp64 reference at that scale.

The scale reaches the kernels in several forms: bf16 folds c2 = scale * log2(e) into Q (forward, dQ) or K (dK/dV); fp16
keeps raw scores and derives its deferred-rescale threshold from the scale; LSE is stored as m * (ln 2 or scale); dQ and dK
are stored times the scale (dK times ln 2 when it reads the q_scaled workspace); the decode kernel computes its own c2.  A
test at the default scale cannot tell any of them from 1/sqrt(D), so every case here also asserts that the output is far
from the fp64 result at 1/sqrt(D).

Scales 0.02 and 1.0 (D = 64: 6x below and 8x above 1/sqrt(D) = 0.125; D = 128: 4x below, 11x above) in two regimes:
  * moderate -- Q and K scaled so that max |score * scale * log2 e| is 16: the per-feature tolerances of the rest of the
    suite apply unchanged (relFro 1e-3 fp16, 8e-3 bf16);
  * large -- unit-variance inputs at scale 1.0 (max |score * scale * log2 e| ~ 60): the forward's rescale branch, the
    lazy-tile bail-out and the family-4 second attempt run on ordinary data.  bf16 follows the error model of
    include/mi355fa.h: relFro <= 8e-3 + K_LARGE * 4.5e-4 * max |score * scale * log2 e|.

LSE is held per row to a + u * SABS (SABS: the row's largest sum_d |q_d k_d| * scale) and delta to rowsum(dO * O) of the
kernel's own O, as in tests/test_gpu_persistent.py.  bf16 dK / dV without the q_scaled workspace follow the error model in
both regimes (bound() below)."""
import ctypes
import math

import pytest
import torch

import fa_oracle as fo

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
LOG2E = 1.4426950408889634
SCALES = (0.02, 1.0)
TARGET = 16.0                     # max |score * scale * log2 e| of the moderate regime
TOL = {F16: 1e-3, BF16: 8e-3}     # relFro per output, moderate regime (test_gpu_parity.py, smoke())
K_LARGE = 2.0                     # bf16, large regime: this many times the documented 4.5e-4 * max|score * scale * log2 e|
TOL_LARGE_F16 = 2e-3
LSE_BOUND = {F16: (1e-4, 0.0), BF16: (1e-3, 2.0 ** -8)}     # |LSE - logsumexp| <= a + u * SABS, per row
FAR = 0.1                         # relFro of O against the 1/sqrt(D) reference, at least


def _lib():
    import _mi355fa as fa
    lib = fa.lib
    lib.fa_debug_force_impl.argtypes = [ctypes.c_int] * 3
    lib.fa_debug_force_impl.restype = None
    lib.fa_debug_pick.argtypes = [ctypes.c_int] * 8
    lib.fa_debug_kvcache_splits.argtypes = [ctypes.c_int]
    lib.fa_debug_kvcache_splits.restype = None
    return fa, lib


# ---------------------------------------------------------------- inputs
def max_score(Q, K, scale, window=None):
    """max over visible (query, key) of |q . k * scale * log2 e|, in fp64 ([B, H, S_q, D] Q, [B, H_kv, S_k, D] K)."""
    g = Q.shape[1] // K.shape[1]
    m = 0.0
    for b in range(Q.shape[0]):
        s = Q[b].double() @ K[b].double().repeat_interleave(g, 0).transpose(-1, -2)
        if window is not None:
            s = s.masked_fill(~fo.visible_mask(Q.shape[2], K.shape[2], window, Q.device), 0.0)
        m = max(m, s.abs().max().item())
    return m * scale * LOG2E


def make_inputs(B, H, Hkv, Sq, Sk, D, dtype, scale, regime, seed=0, window=None):
    """Q, K, V, dO ([B, H(_kv), S, D], device, `dtype`) and M = max |score * scale * log2 e| of the rounded inputs.
    moderate: Q and K both scaled so that M = TARGET before rounding; large: unit variance."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    Q, dO = (torch.randn(B, H, Sq, D, device="cuda", generator=g) for _ in range(2))
    K, V = (torch.randn(B, Hkv, Sk, D, device="cuda", generator=g) for _ in range(2))
    if regime == "moderate":
        a = math.sqrt(TARGET / max_score(Q, K, scale, window))
        Q, K = Q * a, K * a
    Q, K, V, dO = (t.to(dtype) for t in (Q, K, V, dO))
    M = max_score(Q, K, scale, window)
    if regime == "moderate":
        assert M <= TARGET * 1.02, M
    else:
        assert M > 40, M
    return Q, K, V, dO, M


def bound(dtype, regime, M, k_fold=False):
    """relFro bound of one output.  k_fold: bf16 dK / dV without the q_scaled workspace, which fold the scale into K and
    follow the error model in both regimes (at M = 16 the model's 7e-3 is already the size of the moderate tolerance)."""
    model = TOL[BF16] + K_LARGE * 4.5e-4 * M
    if dtype == BF16 and k_fold:
        return model
    if regime == "moderate":
        return TOL[dtype]
    return TOL_LARGE_F16 if dtype == F16 else model


def sabs(Q, K, scale):
    """[B, H, S_q] (on Q's device): per query row the largest sum_d |q_d k_d| * scale over all keys, an upper bound of the
    SABS of fa_oracle.attention_fp64_chunked (which takes the visible keys only) for the references without one."""
    g = Q.shape[1] // K.shape[1]
    return torch.stack([(Q[b].double().abs() @ K[b].double().abs().repeat_interleave(g, 0).transpose(-1, -2)).amax(-1)
                        for b in range(Q.shape[0])]) * scale


# ---------------------------------------------------------------- launches
def launch(Q, K, V, dO, scale, causal=False, window=None, workspace=False, strided=False, varlen=None, drop=None):
    """fa_*_ex (or fa_*_local with a window, fa_*_gqa with H_kv < H) through ctypes, every output NaN-filled first.
    strided: Q, K, V, dO, O, dQ, dK, dV are [B, S, H, D] buffers seen as [B, H, S, D]; varlen: (cu_q, cu_k, dims) with
    packed [T, H, D] tensors; drop: (p, seed)."""
    fa, lib = _lib()
    if varlen:
        B, H, Hkv, Sq, Sk, D = varlen[2]
    else:
        (B, H, Sq, D), Hkv, Sk = Q.shape, K.shape[1], K.shape[2]
    dt = int(Q.dtype == BF16)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()
    if strided:
        nan = lambda t: torch.full(t.transpose(1, 2).shape, float("nan"), dtype=t.dtype, device="cuda").transpose(1, 2)
    else:
        nan = lambda t: torch.full_like(t, float("nan"))
    O, dQ, dK, dV = nan(Q), nan(Q), nan(K), nan(V)
    LSE = torch.full((H, Q.shape[0]) if varlen else (B, H, Sq), float("nan"), device="cuda")
    delta = torch.full_like(LSE, float("nan"))
    qs = torch.full(Q.shape, float("nan"), dtype=Q.dtype, device="cuda") if workspace else None
    kw = {}
    if strided:
        keep = []
        for n, t in (("q", Q), ("k", K), ("v", V), ("dout", dO), ("o", O), ("dq", dQ), ("dk", dK), ("dv", dV)):
            s = fa.strides3(t)
            assert s is not None, n
            keep.append(s)
            kw[n + "_strides"] = ctypes.cast(s, ctypes.POINTER(ctypes.c_longlong))
    if varlen:
        kw.update(cu_seqlens_q=P(varlen[0]), cu_seqlens_k=P(varlen[1]), total_q=Q.shape[0], total_k=K.shape[0])
    if drop:
        kw.update(p_drop=drop[0], seed=drop[1])
    of = ctypes.byref(fa.Opts.make(**kw))
    ob = ctypes.byref(fa.Opts.make(q_scaled=P(qs) if qs is not None else None, **kw))
    if Hkv != H:
        wl, wr = window or ((-1, 0) if causal else (-1, -1))
        fa.check(lib.fa_fwd_gqa(P(Q), P(K), P(V), P(O), P(LSE), B, H, Hkv, Sq, Sk, D, dt, scale, wl, wr, of, st), "fwd")
        fa.check(lib.fa_bwd_dq_gqa(P(Q), P(K), P(V), P(O), P(dO), P(LSE), P(dQ), P(delta), B, H, Hkv, Sq, Sk, D, dt, scale,
                                   wl, wr, ob, st), "dq")
        fa.check(lib.fa_bwd_dkv_gqa(P(Q), P(K), P(V), P(dO), P(LSE), P(delta), P(dK), P(dV), B, H, Hkv, Sq, Sk, D, dt,
                                    scale, wl, wr, ob, st), "dkv")
    elif window:
        wl, wr = window
        fa.check(lib.fa_fwd_local(P(Q), P(K), P(V), P(O), P(LSE), B, H, Sq, Sk, D, dt, scale, wl, wr, of, st), "fwd")
        fa.check(lib.fa_bwd_dq_local(P(Q), P(K), P(V), P(O), P(dO), P(LSE), P(dQ), P(delta), B, H, Sq, Sk, D, dt, scale, wl,
                                     wr, ob, st), "dq")
        fa.check(lib.fa_bwd_dkv_local(P(Q), P(K), P(V), P(dO), P(LSE), P(delta), P(dK), P(dV), B, H, Sq, Sk, D, dt, scale,
                                      wl, wr, ob, st), "dkv")
    else:
        c = int(causal)
        fa.check(lib.fa_fwd_ex(P(Q), P(K), P(V), P(O), P(LSE), B, H, Sq, Sk, D, dt, c, scale, of, st), "fwd")
        fa.check(lib.fa_bwd_dq_ex(P(Q), P(K), P(V), P(O), P(dO), P(LSE), P(dQ), P(delta), B, H, Sq, Sk, D, dt, c, scale,
                                  ob, st), "dq")
        fa.check(lib.fa_bwd_dkv_ex(P(Q), P(K), P(V), P(dO), P(LSE), P(delta), P(dK), P(dV), B, H, Sq, Sk, D, dt, c, scale,
                                   ob, st), "dkv")
    torch.cuda.synchronize()
    return dict(O=O, LSE=LSE, delta=delta, dQ=dQ, dK=dK, dV=dV)


# ---------------------------------------------------------------- checks
def check(tag, gt, got, dO, dtype, regime, M, gt_default_O, workspace):
    """relFro of O, dQ, dK, dV within bound(); LSE per row within a + u * SABS; delta against rowsum(dO * O) of the
    kernel's own O; no NaN; O far from the 1/sqrt(D) reference.  Returns {output: relFro}."""
    errs = {}
    for n in ("O", "dQ", "dK", "dV"):
        t = got[n]
        assert not torch.isnan(t).any(), (tag, n, "NaN")
        errs[n] = fo.rel_fro(gt[n], t.to(gt[n].device))
        b = bound(dtype, regime, M, k_fold=n in ("dK", "dV") and not workspace)
        assert errs[n] < b, (tag, n, errs[n], b, M)
    L, R = got["LSE"].double().to(gt["LSE"].device), gt["LSE"]
    assert not torch.isnan(L).any() and torch.equal(torch.isneginf(L), torch.isneginf(R)), (tag, "LSE")
    fin = torch.isfinite(R)
    err = (L[fin] - R[fin]).abs()
    a, u = LSE_BOUND[dtype]
    lim = a + u * gt["SABS"].to(R.device)[fin]
    errs["LSE"] = err.max().item()
    assert (err <= lim).all(), (tag, "LSE", errs["LSE"])
    prod = dO.to(got["O"].device).double() * got["O"].double()
    d = (got["delta"].double() - prod.sum(-1)).abs() / prod.abs().sum(-1).clamp_min(1e-30)
    assert not torch.isnan(d).any() and d.max() <= 1e-6, (tag, "delta", d.max().item())
    errs["far"] = fo.rel_fro(gt_default_O, got["O"].to(gt_default_O.device))
    assert errs["far"] > FAR, (tag, "O is within %.3g of the 1/sqrt(D) result" % errs["far"])
    return errs


REGIMES = [(s, "moderate") for s in SCALES] + [(1.0, "large")]
REGIME_IDS = ["moderate-0.02", "moderate-1.0", "large-1.0"]
DTYPES = [pytest.param(F16, id="fp16"), pytest.param(BF16, id="bf16")]


def reference(Q, K, V, dO, scale, causal=False, window=None):
    gt = fo.attention_fp64_chunked(Q, K, V, dO, causal, scale=scale, window=window)
    dflt = fo.attention_fp64_chunked(Q, K, V, None, causal, window=window)
    return gt, dflt["O"]


# ---------------------------------------------------------------- families 1-4 of the plain entry points
FAMILY_SHAPE = (2, 8, 1024, 1024, 64)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale,regime", REGIMES, ids=REGIME_IDS)
def test_plain_entry_points_every_family(scale, regime, dtype, causal):
    """fa_fwd / fa_bwd_dq / fa_bwd_dkv with the family forced to 1, 2, 3, 4 (fa_debug_pick asserts it is taken; fp16
    causal dK/dV has no family 4 and takes 3).  There is no dQ family 2: beside the family-2 forward and dK/dV the dQ
    launch is pinned to family 1, which only feeds delta to the dK/dV launch there."""
    fa, lib = _lib()
    B, H, Sq, Sk, D = FAMILY_SHAPE
    Q, K, V, dO, M = make_inputs(B, H, H, Sq, Sk, D, dtype, scale, regime, seed=1)
    gt, dflt = reference(Q, K, V, dO, scale, causal)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()
    dt, c = int(dtype == BF16), int(causal)
    for f in (1, 2, 3, 4):
        forced = (f, 1 if f == 2 else f, f)
        lib.fa_debug_force_impl(*forced)
        try:
            for k in range(3):
                want = 3 if (k == 2 and f == 4 and causal and dtype == F16) else forced[k]
                assert lib.fa_debug_pick(k, D, dt, c, B, H, Sq, Sk) == want, (f, k)
            nan = lambda t: torch.full_like(t, float("nan"))
            O, dQ, dK, dV = nan(Q), nan(Q), nan(K), nan(V)
            LSE = torch.full((B, H, Sq), float("nan"), device="cuda")
            delta = nan(LSE)
            fa.check(lib.fa_fwd(P(Q), P(K), P(V), P(O), P(LSE), B, H, Sq, Sk, D, dt, c, scale, st), "fa_fwd")
            fa.check(lib.fa_bwd_dq(P(Q), P(K), P(V), P(O), P(dO), P(LSE), P(dQ), P(delta), B, H, Sq, Sk, D, dt, c, scale,
                                   st), "fa_bwd_dq")
            fa.check(lib.fa_bwd_dkv(P(Q), P(K), P(V), P(dO), P(LSE), P(delta), P(dK), P(dV), B, H, Sq, Sk, D, dt, c, scale,
                                    st), "fa_bwd_dkv")
            torch.cuda.synchronize()
        finally:
            lib.fa_debug_force_impl(0, 0, 0)
        # the plain pair has no workspace: bf16 dK / dV carry the K-fold error of the error model at any regime
        check("family %d" % f, gt, dict(O=O, LSE=LSE, delta=delta, dQ=dQ, dK=dK, dV=dV), dO, dtype, regime, M, dflt, False)


# ---------------------------------------------------------------- the general and companion entry points
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale,regime", REGIMES, ids=REGIME_IDS)
def test_ex_with_and_without_workspace_and_strided(scale, regime, dtype):
    """fa_*_ex on contiguous tensors with and without q_scaled (causal, D = 128), and on [B, S, H, D] views (full, D = 64)."""
    B, H, S, D = 2, 4, 777, 128
    Q, K, V, dO, M = make_inputs(B, H, H, S, S, D, dtype, scale, regime, seed=2)
    gt, dflt = reference(Q, K, V, dO, scale, True)
    for ws in (False, True):
        check("ex ws=%d" % ws, gt, launch(Q, K, V, dO, scale, causal=True, workspace=ws), dO, dtype, regime, M, dflt, ws)
    B, H, S, D = 2, 4, 640, 64
    Q, K, V, dO, M = make_inputs(B, H, H, S, S, D, dtype, scale, regime, seed=3)
    gt, dflt = reference(Q, K, V, dO, scale, False)
    view = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)
    Qv, Kv, Vv, dOv = (view(t) for t in (Q, K, V, dO))
    got = launch(Qv, Kv, Vv, dOv, scale, strided=True, workspace=dtype == BF16)
    check("ex strided", gt, got, dO, dtype, regime, M, dflt, True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale,regime", REGIMES, ids=REGIME_IDS)
def test_varlen(scale, regime, dtype):
    """fa_*_ex with cu_seqlens: four ragged sequences, one without keys; the workspace on for bf16."""
    H, D = 4, 64
    lens = [(300, 257), (1, 500), (640, 0), (129, 129)]
    cu_q, cu_k = [0], [0]
    for lq, lk in lens:
        cu_q.append(cu_q[-1] + lq)
        cu_k.append(cu_k[-1] + lk)
    Q4, K4, V4, dO4, M = make_inputs(1, H, H, cu_q[-1], cu_k[-1], D, dtype, scale, regime, seed=4)
    pk = lambda t: t[0].transpose(0, 1).contiguous()
    Q, K, V, dO = pk(Q4), pk(K4), pk(V4), pk(dO4)
    cq, ck = (torch.tensor(c, dtype=torch.int32, device="cuda") for c in (cu_q, cu_k))
    dims = (len(lens), H, H, max(l[0] for l in lens), max(l[1] for l in lens), D)
    got = launch(Q, K, V, dO, scale, causal=True, workspace=dtype == BF16, varlen=(cq, ck, dims))
    gt = fo.attention_varlen_fp64(Q.cpu(), K.cpu(), V.cpu(), dO.cpu(), cu_q, cu_k, True, scale=scale)
    dflt = fo.attention_varlen_fp64(Q.cpu(), K.cpu(), V.cpu(), dO.cpu(), cu_q, cu_k, True)["O"]
    gt["LSE"] = torch.where(gt["O"].abs().sum(-1).transpose(0, 1) == 0, float("-inf"), gt["LSE"])   # the rows without keys
    gt["SABS"] = sabs(Q4, K4, scale)[0].cpu()
    got["delta"] = got["delta"].transpose(0, 1)                  # [H, T] -> [T, H], the rows of the packed dO * O
    check("varlen", gt, got, dO.cpu(), dtype, regime, M, dflt, True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale,regime", REGIMES, ids=REGIME_IDS)
def test_dropout(scale, regime, dtype):
    """fa_*_ex with p_drop = 0.2: the same Philox keep mask, against attention_dropout_fp64 at the scale."""
    B, H, S, D = 1, 2, 384, 64
    p, seed = 0.2, 1234
    Q, K, V, dO, M = make_inputs(B, H, H, S, S, D, dtype, scale, regime, seed=5)
    got = launch(Q, K, V, dO, scale, causal=True, drop=(p, seed))
    keep, rp = fo.dropout_keep_mask(B, H, S, S, p, seed)
    cpu = [t.cpu() for t in (Q, K, V, dO)]
    gt = fo.attention_dropout_fp64(*cpu, True, keep, rp, scale=scale)
    dflt = fo.attention_dropout_fp64(*cpu, True, keep, rp)["O"]
    gt["SABS"] = sabs(Q, K, scale).cpu()
    check("dropout", gt, got, cpu[3], dtype, regime, M, dflt, False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale,regime", REGIMES, ids=REGIME_IDS)
def test_local_and_gqa(scale, regime, dtype):
    """fa_*_local with windows (127, 0) and (64, 200), fa_*_gqa at g = 4 causal and g = 8 with a window (workspace on for
    bf16)."""
    for (B, H, Hkv, Sq, Sk, D, w) in ((2, 4, 4, 900, 900, 64, (127, 0)), (1, 4, 4, 513, 700, 128, (64, 200)),
                                     (2, 8, 2, 600, 777, 64, (-1, 0)), (1, 16, 2, 1000, 1000, 128, (300, 300))):
        Q, K, V, dO, M = make_inputs(B, H, Hkv, Sq, Sk, D, dtype, scale, regime, seed=Sq, window=w)
        gt, dflt = reference(Q, K, V, dO, scale, window=w)
        got = launch(Q, K, V, dO, scale, window=w, workspace=dtype == BF16)
        check("H %d H_kv %d window %s" % (H, Hkv, w), gt, got, dO, dtype, regime, M, dflt, True)


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale,regime", REGIMES, ids=REGIME_IDS)
def test_kvcache_softmax_scale(scale, regime, dtype, splits):
    """flash_attention_kvcache(softmax_scale=...) with 1 and 3 forced splits, O and LSE against the fp64 reference of
    test_gpu_kvcache.py at that scale, and far from the one at 1/sqrt(D)."""
    import My_FlashAttention_optimized as M_
    import test_gpu_kvcache as tk
    _, lib = _lib()
    B, H, Hkv, Sq, Sc, D = 4, 16, 4, 3, 2048, 128
    lens = [2048, 777, 1, 1500]
    g = torch.Generator(device="cuda").manual_seed(6)
    q = torch.randn(B, H, Sq, D, device="cuda", generator=g)
    kc, vc = (torch.randn(B, Hkv, Sc, D, device="cuda", generator=g) for _ in range(2))
    if regime == "moderate":
        m = max_score(q, kc, scale)
        q, kc = q * math.sqrt(TARGET / m), kc * math.sqrt(TARGET / m)
    q, kc, vc = q.to(dtype), kc.to(dtype), vc.to(dtype)
    Mx = max_score(q, kc, scale)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    lib.fa_debug_kvcache_splits(splits)
    try:
        o, lse = M_.flash_attention_kvcache(q, kc, vc, sl, softmax_scale=scale, return_lse=True)
        torch.cuda.synchronize()
    finally:
        lib.fa_debug_kvcache_splits(0)
    O_ref, LSE_ref = tk.ref_fp64(q, kc, vc, lens, -1, -1, scale)
    O_dflt, _ = tk.ref_fp64(q, kc, vc, lens, -1, -1)
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()
    err = fo.rel_fro(O_ref, o)
    b = bound(dtype, regime, Mx)
    assert err < b, (err, b, Mx)
    a, u = LSE_BOUND[dtype]
    fin = torch.isfinite(LSE_ref)
    assert torch.equal(fin, torch.isfinite(lse))
    lse_err = (lse.double() - LSE_ref)[fin].abs()
    assert (lse_err <= a + u * sabs(q, kc, scale)[fin]).all(), lse_err.max().item()
    assert fo.rel_fro(O_dflt, o) > FAR
