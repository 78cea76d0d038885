"""The sliding-window (fa_*_local), grouped-query (fa_*_gqa, packed varlen included) kernels against fp64, block by block.

The method of tests/test_gpu_persistent.py, at the sizes these kernels run at: every (batch, head, 128-row block) of O and
dQ and every (batch, K/V head, 128-key block) of dK and dV is compared with an fp64 reference computed on the device
(fa_oracle.attention_fp64_chunked with window= and H_kv heads), LSE row by row within a + u * SABS, delta against
rowsum(dO * O) of the kernel's own O.  A whole-tensor norm cannot see one wrong block at these sizes.

Every output of the raw C entry points (O, LSE, dQ, delta, dK, dV and, for bf16, the q_scaled workspace) is filled with
NaN before its launch, so an element a kernel skips stays NaN; bf16 runs once without and once with the workspace.  Each
case also runs once through the autograd function.

Neighbouring heads differ on purpose: Q is scaled per query head by 0.3, 1, 2.5 in turn; V = 0 on every 7th K/V head
(when there is more than one), so O, dQ and dK of its query heads are exactly 0 and dV is not; dO = 0 on all query heads
of every 5th K/V head (from the 4th), so its dK and dV are exactly 0; and dO = 0 on one single query head elsewhere, so
its dQ is exactly 0.  Wherever the fp64 reference has an exactly zero row -- those heads, rows that see no key, keys outside
every band, empty sequences -- the kernel's row must be exactly zero (it was NaN before the launch).

Rows that see fewer than FEW keys are checked row by row instead (FEW_BOUND below).

Per-block relative Frobenius errors measured on an MI355X over every case here, as largest block / largest per-case
median block ("raw" = the C entry points without the workspace; "ws" = with the bf16 q_scaled workspace, which the
autograd path equals bit for bit; fp16 ignores the workspace):

                  fp16 D = 64      fp16 D = 128     bf16 D = 64      bf16 D = 128
    O             3.6e-4/3.0e-4    3.2e-4/2.9e-4    5.9e-3/2.9e-3    4.5e-3/2.9e-3
    dQ            6.0e-4/3.0e-4    9.3e-4/3.0e-4    7.6e-3/3.0e-3    5.2e-3/2.9e-3
    dK  raw       6.5e-4/3.3e-4    6.7e-4/3.4e-4    2.0e-2/6.8e-3    8.4e-3/5.8e-3
    dK  ws                                          1.2e-2/4.7e-3    5.3e-3/4.3e-3
    dV  raw       3.5e-4/2.9e-4    4.1e-4/2.9e-4    2.0e-2/6.5e-3    9.0e-3/5.4e-3
    dV  ws                                          8.4e-3/4.2e-3    4.4e-3/3.6e-3

The largest block is at most 3.1x the median of its group; LSE is within 0.3 of its bound a + u * SABS on every row, delta
within 1.8e-7 relative of rowsum(dO * O).  At g = 32 every dK / dV block of the fp32 group sum is at most 0.98x the error
of the expanded path (median 0.94x).  The bounds below sit about 1.5x above the largest errors."""
import ctypes
import random

import pytest
import torch

import fa_oracle as fo

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
Q_SCALES = (0.3, 1.0, 2.5)

# (B, H, H_kv, S_q, S_k, D, dtype, window (wl, wr), id)
CASES = [
    # GQA at H = 32: g = 4, 8, 16, 32; S_q != S_k with ragged tails; full, causal, (1023, 0), (255, 255)
    (1, 32, 8, 2048, 2048, 64, BF16, (-1, -1), "g4-full-bf16-d64"),
    (1, 32, 4, 3001, 2477, 128, F16, (-1, 0), "g8-causal-ragged-fp16-d128"),
    (1, 32, 2, 2177, 4096, 64, F16, (1023, 0), "g16-w1023-ragged-fp16-d64"),
    (2, 32, 1, 4096, 3333, 128, BF16, (255, 255), "g32-w255x255-ragged-bf16-d128"),
    (2, 32, 1, 2048, 2900, 64, F16, (-1, -1), "g32-full-ragged-fp16-d64"),
    (2, 32, 1, 4096, 4096, 64, BF16, (-1, 0), "g32-causal-bf16-d64"),
    # sliding windows at B2 H16 S8192
    (2, 16, 16, 8192, 8192, 64, F16, (1023, 0), "local-w1023-fp16-d64"),
    (2, 16, 16, 8192, 8192, 128, BF16, (511, 511), "local-w511x511-bf16-d128"),
    (2, 16, 16, 8192, 8192, 64, BF16, (255, 0), "local-w255-bf16-d64"),
    (2, 16, 16, 8192, 8192, 128, F16, (255, 255), "local-w255x255-fp16-d128"),
    # exactly as tools/local_bench.py and tools/gqa_bench.py run them
    (4, 32, 32, 16384, 16384, 64, BF16, (1023, 0), "bench-local-w1023"),
    (4, 32, 8, 16384, 16384, 64, BF16, (-1, 0), "bench-gqa-hkv8-causal"),
]


def _lib():
    import _mi355fa as fa
    return fa, fa.lib


def _M():
    import My_FlashAttention_optimized as M
    return M


# ---------------------------------------------------------------- inputs
def special_heads(B, H, Hkv):
    """[B * H_kv] masks of the K/V slices with V = 0 and with dO = 0 on every query head, and the one (batch * H + head)
    query slice with dO = 0 alone (in a K/V slice that is neither; the second head of its group when g > 1)."""
    kv = torch.arange(B * Hkv)
    v0 = (kv % 7 == 0) & (B * Hkv > 1)
    d0 = kv % 5 == 3
    g = H // Hkv
    j = 1 if B * Hkv > 1 else 0
    return v0, d0, j * g + min(1, g - 1)


def make_inputs(B, H, Hkv, Sq, Sk, D, dtype, seed=0):
    """Q, dO [B, H, S_q, D], K, V [B, H_kv, S_k, D] on the device with the per-head differences of the module docstring,
    and the Q-scale class of every (batch, head)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    Q, dO = (torch.randn(B, H, Sq, D, device="cuda", generator=g) for _ in range(2))
    K, V = (torch.randn(B, Hkv, Sk, D, device="cuda", generator=g) for _ in range(2))
    bh = torch.arange(B * H, device="cuda").reshape(B, H)
    Q *= torch.tensor(Q_SCALES, device="cuda")[bh % 3][..., None, None]
    v0, d0, single = special_heads(B, H, Hkv)
    V.view(B * Hkv, Sk, D)[v0.cuda()] = 0
    dO.view(B * Hkv, H // Hkv, Sq, D)[d0.cuda()] = 0
    dO.view(B * H, Sq, D)[single] = 0
    return Q.to(dtype), K.to(dtype), V.to(dtype), dO.to(dtype), bh % 3


# ---------------------------------------------------------------- launches
def launch_raw(Q, K, V, dO, window, workspace, dims=None, varlen=None):
    """fa_*_local (H_kv = H) or fa_*_gqa through ctypes, every output and the workspace NaN-filled first.  dims: (B, H,
    H_kv, S_q, S_k, D) when the tensors are packed; varlen: (cu_q, cu_k) int32 device tensors."""
    fa, lib = _lib()
    B, H, Hkv, Sq, Sk, D = dims or (Q.shape[0], Q.shape[1], K.shape[1], Q.shape[2], K.shape[2], Q.shape[3])
    dt, sc = int(Q.dtype == BF16), D ** -0.5
    wl, wr = window
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()
    nan = lambda t: torch.full_like(t, float("nan"))
    O, dQ, dK, dV = nan(Q), nan(Q), nan(K), nan(V)
    lse_shape = (H, Q.shape[0]) if varlen else (B, H, Sq)
    LSE = torch.full(lse_shape, float("nan"), device="cuda")
    delta = torch.full_like(LSE, float("nan"))
    qs = nan(Q) if workspace else None
    kw = {}
    if varlen:
        kw = dict(cu_seqlens_q=P(varlen[0]), cu_seqlens_k=P(varlen[1]), total_q=Q.shape[0], total_k=K.shape[0])
    of = fa.Opts.make(**kw)
    ob = fa.Opts.make(q_scaled=P(qs) if qs is not None else None, **kw)
    of, ob = ctypes.byref(of), ctypes.byref(ob)
    if Hkv == H:
        fa.check(lib.fa_fwd_local(P(Q), P(K), P(V), P(O), P(LSE), B, H, Sq, Sk, D, dt, sc, wl, wr, of, st), "fa_fwd_local")
        fa.check(lib.fa_bwd_dq_local(P(Q), P(K), P(V), P(O), P(dO), P(LSE), P(dQ), P(delta), B, H, Sq, Sk, D, dt, sc, wl, wr,
                                     ob, st), "fa_bwd_dq_local")
        fa.check(lib.fa_bwd_dkv_local(P(Q), P(K), P(V), P(dO), P(LSE), P(delta), P(dK), P(dV), B, H, Sq, Sk, D, dt, sc, wl,
                                      wr, ob, st), "fa_bwd_dkv_local")
    else:
        fa.check(lib.fa_fwd_gqa(P(Q), P(K), P(V), P(O), P(LSE), B, H, Hkv, Sq, Sk, D, dt, sc, wl, wr, of, st), "fa_fwd_gqa")
        fa.check(lib.fa_bwd_dq_gqa(P(Q), P(K), P(V), P(O), P(dO), P(LSE), P(dQ), P(delta), B, H, Hkv, Sq, Sk, D, dt, sc, wl,
                                   wr, ob, st), "fa_bwd_dq_gqa")
        fa.check(lib.fa_bwd_dkv_gqa(P(Q), P(K), P(V), P(dO), P(LSE), P(delta), P(dK), P(dV), B, H, Hkv, Sq, Sk, D, dt, sc,
                                    wl, wr, ob, st), "fa_bwd_dkv_gqa")
    torch.cuda.synchronize()
    out = dict(O=O, LSE=LSE, delta=delta, dQ=dQ, dK=dK, dV=dV)
    if qs is not None:
        assert not torch.isnan(qs).any(), "the dQ launch left q_scaled rows unwritten"
    return out


def launch_autograd(Q, K, V, dO, window, varlen=None, max_seqlen=None):
    """flash_attention_local (H_kv = H, fixed length) or flash_attention_gqa, and its backward."""
    M = _M()
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    if varlen:
        o = M.flash_attention_gqa(q, k, v, window_size=window, cu_seqlens_q=varlen[0], cu_seqlens_k=varlen[1],
                                  max_seqlen_q=max_seqlen[0], max_seqlen_k=max_seqlen[1])
    elif K.shape[1] == Q.shape[1]:
        o = M.flash_attention_local(q, k, v, *window)
    else:
        o = M.flash_attention_gqa(q, k, v, window_size=window)
    o.backward(dO)
    torch.cuda.synchronize()
    return dict(O=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)


def same_bits(a, b):
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.view(iv), b.view(iv))


# ---------------------------------------------------------------- the checks
# Per-block relative Frobenius error bounds by (dtype, output), about 1.5x the largest block error measured on an MI355X
# over every case in this file (module docstring); the limit against the median block error of the same Q scale is
# RATIO x median + FLOOR.  bf16 dK / dV without the workspace fold the softmax scale into K (a second rounding of the
# exponent argument whose error grows with the score magnitude, include/mi355fa.h): "raw" has its own bound there.
BLOCK_BOUND = {
    (F16, "O"): 6e-4, (F16, "dQ"): 1.4e-3, (F16, "dK"): 1e-3, (F16, "dV"): 6.5e-4,
    (BF16, "O"): 9e-3, (BF16, "dQ"): 1.15e-2, (BF16, "dK"): 1.8e-2, (BF16, "dV"): 1.3e-2,
}
BLOCK_BOUND_RAW_BF16_DKV = 3e-2
# Rows that see fewer than FEW keys (and keys seen only by such rows): there dQ (dK) is a near-cancellation -- a row that
# sees one key has P = 1 and dS = P (dP - delta) = 0 exactly in fp64, while the kernel's delta comes from the 16-bit O --
# so a relative error means nothing.  Those rows are left out of the block check and held, each on its own, to FEW_BOUND
# relative to the larger of their own norm and the RMS row norm of their (batch, head).  The error there is that of delta
# (rowsum(dO * O) of the 16-bit O, as in the reference) against a small dS; measured up to 4.8e-3 (fp16) and 5.2e-2
# (bf16), roughly in the ratio of the two formats' unit roundoffs.
FEW = 8
FEW_BOUND = {F16: 7.5e-3, BF16: 8e-2}
RATIO, FLOOR = 4.0, 1e-5
LSE_BOUND = {F16: (1e-4, 0.0), BF16: (1e-3, 2.0 ** -8)}     # |LSE - logsumexp| <= a + u * SABS, per row
DELTA_BOUND = 1e-6                                          # |delta - rowsum(dO * O)| / rowsum(|dO * O|), per row
# the fp32 group sum against repeat_interleave + flash_attention + autograd's sum, per block (test_gpu_gqa.py's margin)
GROUP_SUM_MARGIN = 1.05


def few_rows(vis):
    """[S_q] rows that see fewer than FEW keys but at least one, [S_k] keys seen by such rows only, from a visibility mask."""
    nq = vis.sum(1)
    few_q = (nq > 0) & (nq < FEW)
    few_k = vis.any(0) & ~(vis & (nq >= FEW)[:, None]).any(0)
    return few_q, few_k


def structural_zeros(n, gt, dO, V):
    """[B, H(_kv), S] rows of output n that are exactly 0 by construction: O where fp64 O is 0 (V = 0 heads, rows without a
    key); dQ there and where dO = 0; dV where fp64 dV is 0 (dO = 0 groups, keys no query sees); dK there and on V = 0
    heads."""
    if n in ("O", "dV"):
        return (gt[n] == 0).all(-1)
    if n == "dQ":
        return (gt["O"] == 0).all(-1) | (dO == 0).all(-1)
    return (gt["dV"] == 0).all(-1) | (V == 0).flatten(2).all(-1)[..., None]


def check_outputs(tag, gt, got, dO, groups, kv_groups, dtype, mode, check=True, V=None, few=None):
    """Block-check every output in `got` against the fp64 `gt` (all [B, H(_kv), S, D] / [B, H, S]); exact zeros where
    they are structural; no NaN.  few: ([S_q], [S_k]) bool rows of few_rows, checked absolutely.  Returns one record per
    output."""
    recs = []
    for n in ("O", "dQ", "dK", "dV"):
        if n not in got:
            continue
        t = got[n]
        zero_rows = structural_zeros(n, gt, dO, V) if V is not None else (gt[n] == 0).all(-1)
        recs.append(dict(tag=tag, out=n, nan=bool(torch.isnan(t).any()),
                         zeros_ok=bool((t[zero_rows] == 0).all()), n_zero_rows=int(zero_rows.sum())))
        bound = BLOCK_BOUND[dtype, n]
        if mode == "raw" and dtype == BF16 and n in ("dK", "dV"):
            bound = BLOCK_BOUND_RAW_BF16_DKV
        r = gt[n]
        rows = None if few is None or n not in ("dQ", "dK") else few[0 if n == "dQ" else 1].to(r.device)
        if rows is not None and bool(rows.any()):
            rms = r.square().sum(-1).mean(-1).sqrt()[..., None]               # [B, H(_kv), 1]
            scale = torch.maximum(r[..., rows, :].norm(dim=-1), rms)
            aerr = (t.double()[..., rows, :] - r[..., rows, :]).norm(dim=-1) / scale.clamp_min(1e-300)
            aerr = torch.where(torch.isnan(aerr), float("inf"), aerr)
            recs[-1].update(few_rows=int(rows.sum()), few_max=aerr.max().item())
            if check:
                assert aerr.max() <= FEW_BOUND[dtype], (tag, n, "a row with few keys is off by %.3e" % aerr.max())
            keep = ~rows
            r, t = r[..., keep, :], t[..., keep, :]
        st = fo.block_stats(r, t, groups if n in ("O", "dQ") else kv_groups)
        recs[-1].update(max=st["max"], median=st["median"], max_ratio=st["max_ratio"], worst=st["worst"])
        if check:
            assert not recs[-1]["nan"], (tag, n, "NaN")
            assert recs[-1]["zeros_ok"], (tag, n, "a row that is exactly 0 in fp64 is not exactly 0")
            fo.assert_blocks("%s %s" % (tag, n), st, bound, RATIO, FLOOR)
    if "LSE" in got:
        L, R = got["LSE"].double(), gt["LSE"]
        inf_ok = torch.equal(torch.isneginf(L), torch.isneginf(R))
        fin = torch.isfinite(R)
        err = torch.where(fin, (L - R).abs(), torch.zeros_like(R))
        err = torch.where(torch.isnan(L), float("inf"), err)
        a, u = LSE_BOUND[dtype]
        excess = err / (a + u * gt["SABS"])
        at = tuple(int(x) for x in torch.unravel_index(excess.argmax(), err.shape))
        recs.append(dict(tag=tag, out="LSE", max=err.max().item(), max_excess=excess.max().item(), worst=at, inf_ok=inf_ok))
        if check:
            assert inf_ok, (tag, "LSE = -inf exactly on the rows without a visible key, and only there")
            assert excess.max() <= 1, "%s LSE: row %s off by %.3e (bound %.3e)" % (
                tag, at, err[at].item(), a + u * gt["SABS"][at].item())
    if "delta" in got:
        prod = dO.double() * got["O"].double()
        err = (got["delta"].double() - prod.sum(-1)).abs() / prod.abs().sum(-1).clamp_min(1e-30)
        err = torch.where(torch.isnan(err), float("inf"), err)
        recs.append(dict(tag=tag, out="delta", max=err.max().item()))
        if check:
            assert err.max() <= DELTA_BOUND, "%s delta: off by %.3e" % (tag, err.max().item())
    return recs


def kv_groups_of(B, H, Hkv, groups):
    """block_stats groups of dK / dV: the Q-scale class when g = 1, else one group (every K/V head mixes the scales)."""
    return groups if H == Hkv else None


def run_case(case, check=True, seed=0):
    B, H, Hkv, Sq, Sk, D, dtype, window, tag = case
    Q, K, V, dO, groups = make_inputs(B, H, Hkv, Sq, Sk, D, dtype, seed)
    gt = fo.attention_fp64_chunked(Q, K, V, dO, window=window)
    kvg = kv_groups_of(B, H, Hkv, groups)
    few = few_rows(fo.visible_mask(Sq, Sk, window, "cuda"))
    cw = dict(check=check, V=V, few=few)
    recs = []
    raw = launch_raw(Q, K, V, dO, window, workspace=False)
    recs += check_outputs(tag + " raw", gt, raw, dO, groups, kvg, dtype, "raw", **cw)
    ref_bits = raw
    if dtype == BF16:
        ws = launch_raw(Q, K, V, dO, window, workspace=True)
        recs += check_outputs(tag + " ws", gt, ws, dO, groups, kvg, dtype, "ws", **cw)
        for n in ("O", "LSE", "delta", "dQ"):
            assert same_bits(raw[n], ws[n]), (tag, n, "the workspace changes only dK / dV")
        ref_bits = ws
    ag = launch_autograd(Q, K, V, dO, window)
    recs += check_outputs(tag + " autograd", gt, ag, dO, groups, kvg, dtype, "ws", **cw)
    for n in ("O", "dQ", "dK", "dV"):
        assert same_bits(ag[n], ref_bits[n]), (tag, n, "autograd and the raw launch")
    for r in recs:
        r.update(dtype="bf16" if dtype == BF16 else "fp16", D=D)
    return recs


@pytest.mark.parametrize("case", [pytest.param(c, id=c[-1]) for c in CASES])
def test_blocks_against_fp64(case):
    run_case(case)


# ---------------------------------------------------------------- packed variable-length batch
def packed_lengths(n=32, cap=4096, seed=5):
    """n (S_q, S_k) pairs up to `cap`: ragged, with an empty sequence on either side and a few at the cap."""
    rnd = random.Random(seed)
    lens = [(rnd.randint(1, cap), rnd.randint(1, cap)) for _ in range(n)]
    lens[3] = (0, 700)
    lens[11] = (913, 0)
    lens[17] = (cap, cap)
    lens[24] = (1, cap)
    lens[29] = (cap, 129)
    return lens


def packed_reference(Q, K, V, dO, cu_q, cu_k, window):
    """Per-sequence attention_fp64_chunked, assembled into packed [1, H, T, D] (O, dQ), [1, H_kv, T_k, D] (dK, dV),
    [1, H, T] (LSE, SABS); a sequence without keys: O = 0, LSE = -inf, dQ = 0; without queries: dK = dV = 0."""
    Tq, H, D = Q.shape
    Tk, Hkv, _ = K.shape
    f64 = dict(dtype=torch.float64, device="cuda")
    out = dict(O=torch.zeros(1, H, Tq, D, **f64), dQ=torch.zeros(1, H, Tq, D, **f64), dK=torch.zeros(1, Hkv, Tk, D, **f64),
               dV=torch.zeros(1, Hkv, Tk, D, **f64), LSE=torch.full((1, H, Tq), float("-inf"), **f64),
               SABS=torch.zeros(1, H, Tq, **f64))
    sl = lambda t, a, e: t[a:e].transpose(0, 1).unsqueeze(0)
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = cu_q[b], cu_q[b + 1], cu_k[b], cu_k[b + 1]
        if q1 == q0 or k1 == k0:
            continue
        r = fo.attention_fp64_chunked(sl(Q, q0, q1), sl(K, k0, k1), sl(V, k0, k1), sl(dO, q0, q1), window=window)
        for n in ("O", "dQ", "LSE", "SABS"):
            out[n][:, :, q0:q1] = r[n]
        for n in ("dK", "dV"):
            out[n][:, :, k0:k1] = r[n]
    return out


PACKED = [(32, 8, 128, F16, (511, 0), "packed-g4-w511-fp16-d128"),
          (32, 2, 64, BF16, (255, 255), "packed-g16-w255x255-bf16-d64")]


def run_packed(case, check=True):
    H, Hkv, D, dtype, window, tag = case
    lens = packed_lengths()
    cu_q = [0]
    cu_k = [0]
    for lq, lk in lens:
        cu_q.append(cu_q[-1] + lq)
        cu_k.append(cu_k[-1] + lk)
    Tq, Tk = cu_q[-1], cu_k[-1]
    # the [B, H, S, D] inputs of make_inputs with B = 1 and S = total, seen packed [T, H, D]
    Q4, K4, V4, dO4, groups = make_inputs(1, H, Hkv, Tq, Tk, D, dtype, seed=3)
    pk = lambda t: t[0].transpose(0, 1).contiguous()
    up = lambda t: t.transpose(0, 1).unsqueeze(0)
    Q, K, V, dO = pk(Q4), pk(K4), pk(V4), pk(dO4)
    cq = torch.tensor(cu_q, dtype=torch.int32, device="cuda")
    ck = torch.tensor(cu_k, dtype=torch.int32, device="cuda")
    mq, mk = max(l[0] for l in lens), max(l[1] for l in lens)
    gt = packed_reference(Q, K, V, dO, cu_q, cu_k, window)
    assert (gt["O"][:, :, cu_q[11]:cu_q[12]] == 0).all() and torch.isneginf(gt["LSE"][:, :, cu_q[11]:cu_q[12]]).all()
    assert (gt["dK"][:, :, cu_k[3]:cu_k[4]] == 0).all()
    kvg = kv_groups_of(1, H, Hkv, groups)
    few_q = torch.zeros(Tq, dtype=torch.bool, device="cuda")
    few_k = torch.zeros(Tk, dtype=torch.bool, device="cuda")
    for b, (lq, lk) in enumerate(lens):
        if lq and lk:
            fq, fk = few_rows(fo.visible_mask(lq, lk, window, "cuda"))
            few_q[cu_q[b]:cu_q[b + 1]], few_k[cu_k[b]:cu_k[b + 1]] = fq, fk
    cw = dict(check=check, V=V4, few=(few_q, few_k))
    dims = (len(lens), H, Hkv, mq, mk, D)
    recs = []
    runs = [("raw", False)] + ([("ws", True)] if dtype == BF16 else [])
    for mode, wsp in runs:
        r = launch_raw(Q, K, V, dO, window, wsp, dims=dims, varlen=(cq, ck))
        got = {n: up(r[n]) for n in ("O", "dQ", "dK", "dV")}
        got.update(LSE=r["LSE"].unsqueeze(0), delta=r["delta"].unsqueeze(0))
        recs += check_outputs("%s %s" % (tag, mode), gt, got, dO4, groups, kvg, dtype, mode, **cw)
    ag = launch_autograd(Q, K, V, dO, window, varlen=(cq, ck), max_seqlen=(mq, mk))
    recs += check_outputs(tag + " autograd", gt, {n: up(t) for n, t in ag.items()}, dO4, groups, kvg, dtype, "ws", **cw)
    for r in recs:
        r.update(dtype="bf16" if dtype == BF16 else "fp16", D=D)
    return recs


@pytest.mark.parametrize("case", [pytest.param(c, id=c[-1]) for c in PACKED])
def test_packed_batch_blocks_against_fp64(case):
    """About 32 packed sequences of ragged lengths up to 4096, an empty one on either side, with GQA and a window."""
    run_packed(case)


# ---------------------------------------------------------------- the fp32 group sum at g = 32
GROUP_SUM_CASE = (2, 32, 1, 4096, 4096, 64, BF16, (-1, 0), "g32-causal-bf16-d64")


def group_sum_errors(case):
    """Per-block dK / dV errors of flash_attention_gqa and of repeat_interleave + flash_attention + autograd's sum."""
    B, H, Hkv, Sq, Sk, D, dtype, window, tag = case
    Q, K, V, dO, _ = make_inputs(B, H, Hkv, Sq, Sk, D, dtype, seed=9)
    gt = fo.attention_fp64_chunked(Q, K, V, dO, window=window)
    ag = launch_autograd(Q, K, V, dO, window)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    g = H // Hkv
    o = _M().flash_attention(q, k.repeat_interleave(g, 1), v.repeat_interleave(g, 1), is_causal=window == (-1, 0))
    o.backward(dO)
    torch.cuda.synchronize()
    ex = dict(dK=k.grad, dV=v.grad)
    return {n: (fo.block_errors(gt[n], ag[n]), fo.block_errors(gt[n], ex[n])) for n in ("dK", "dV")}


def test_group_sum_is_no_less_accurate_than_the_expanded_path_per_block():
    """At g = 32 (multi-query at H = 32) every 128-key block of dK and dV from the kernel's fp32 group sum is at least as
    accurate as the path without GQA (32 bf16 per-head gradients summed by autograd), within test_gpu_gqa.py's 5 %."""
    for n, (e_gqa, e_ex) in group_sum_errors(GROUP_SUM_CASE).items():
        bad = e_gqa > GROUP_SUM_MARGIN * e_ex
        at = tuple(int(x) for x in torch.unravel_index((e_gqa / e_ex.clamp_min(1e-300)).argmax(), e_gqa.shape))
        assert not bad.any(), "%s: block %s %.3e vs %.3e on the expanded path; %d blocks worse" % (
            n, at, e_gqa[at].item(), e_ex[at].item(), int(bad.sum()))
