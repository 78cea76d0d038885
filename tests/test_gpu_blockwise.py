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

import pytest
import torch

import fa_oracle as fo
from blockcheck import check_outputs as check_outputs_with
from blockcheck import FEW, few_rows, kv_groups_of, make_inputs, packed_lengths, packed_reference, same_bits

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16

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
FEW_BOUND = {F16: 7.5e-3, BF16: 8e-2}
RATIO, FLOOR = 4.0, 1e-5
LSE_BOUND = {F16: (1e-4, 0.0), BF16: (1e-3, 2.0 ** -8)}     # |LSE - logsumexp| <= a + u * SABS, per row
DELTA_BOUND = 1e-6                                          # |delta - rowsum(dO * O)| / rowsum(|dO * O|), per row
# the fp32 group sum against repeat_interleave + flash_attention + autograd's sum, per block (test_gpu_gqa.py's margin)
GROUP_SUM_MARGIN = 1.05


BOUNDS = dict(BLOCK_BOUND=BLOCK_BOUND, BLOCK_BOUND_RAW_BF16_DKV=BLOCK_BOUND_RAW_BF16_DKV, FEW_BOUND=FEW_BOUND, RATIO=RATIO,
              FLOOR=FLOOR, LSE_BOUND=LSE_BOUND, DELTA_BOUND=DELTA_BOUND)


def check_outputs(tag, gt, got, dO, groups, kv_groups, dtype, mode, check=True, V=None, few=None):
    """blockcheck.check_outputs with this file's bounds."""
    return check_outputs_with(tag, gt, got, dO, groups, kv_groups, dtype, mode, BOUNDS, check=check, V=V, few=few)


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
# (H, H_kv, D, dtype, window, id[, (n, cap) of packed_lengths: 32 sequences up to 4096 without it])
PACKED = [(32, 8, 128, F16, (511, 0), "packed-g4-w511-fp16-d128"),
          (32, 2, 64, BF16, (255, 255), "packed-g16-w255x255-bf16-d64"),
          # g = 3: in variable-length launches batch_head orders the slices (head, batch) with H / group heads
          (6, 2, 64, BF16, (127, 40), "packed-g3-w127x40-bf16-d64-n8", (8, 512))]


def run_packed(case, check=True):
    H, Hkv, D, dtype, window, tag = case[:6]
    lens = packed_lengths(*case[6]) if len(case) > 6 else packed_lengths()
    no_k = [i for i, (lq, lk) in enumerate(lens) if lq and not lk]     # sequences with queries and no keys, and the reverse
    no_q = [i for i, (lq, lk) in enumerate(lens) if lk and not lq]
    assert no_k and no_q
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
    for i in no_k:
        assert (gt["O"][:, :, cu_q[i]:cu_q[i + 1]] == 0).all() and torch.isneginf(gt["LSE"][:, :, cu_q[i]:cu_q[i + 1]]).all()
    for i in no_q:
        assert (gt["dK"][:, :, cu_k[i]:cu_k[i + 1]] == 0).all()
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


@pytest.mark.parametrize("case", [pytest.param(c, id=c[5]) for c in PACKED])
def test_packed_batch_blocks_against_fp64(case):
    """About 32 packed sequences of ragged lengths up to 4096 (8 up to 512 at g = 3), an empty one on either side, with GQA
    and a window."""
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
