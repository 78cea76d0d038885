"""The persistent schedule family 4 (fa_fwd_v4.hip, fa_bwd_dq_v4.hip, fa_bwd_dkv_v4.hip) against fp64, item by item.

All three kernels launch at most one workgroup per CU (the CU count rounded down to a multiple of 8, N) and walk the work
list blockIdx.x, blockIdx.x + gridDim.x, ... through xcd_remap.  Most of their hand-ordered code runs only when a workgroup
has a NEXT item: the forward's K/V ring runs on into it (CONT) and, at D = 64, stages its Q rows (STAGEQ); the non-causal
dQ and dK/dV kernels stage its rows in their last tile steps (nc_stage); the forward's exact second attempt restarts the ring
while the next pass's tiles are in flight.  Every case here therefore has more items than workgroups (asserted from a
restatement of each launcher's work list, `work`), runs with the family forced to 4 and asserts that the launch really
takes it, and checks every (batch, head, 128-row block) of O, dQ, dK and dV against an fp64 reference computed on the
device (fa_oracle.attention_fp64_chunked), LSE row by row and delta against rowsum(dO * O) of the kernel's own O.  A
whole-tensor norm cannot see one wrong item at these sizes: 1 of 4096 blocks 3 % off moves it by ~5e-4.

Neighbouring items differ on purpose, so that state carried from a workgroup's previous item shows: Q is scaled per (batch,
head) by 0.3, 1, 2.5 in turn; V = 0 in every 7th (batch, head), where O, dQ and dK must come out exactly 0 and dV must not;
dO = 0 in every 11th, where dQ, dK and dV must come out exactly 0.  Per-block errors are compared with the median of the
blocks of the same Q scale.

Per-block relative Frobenius errors measured on an MI355X over CASES and HEADLINE, family-4 launches, as largest block /
median block ("raw" = the C entry points; "ws" = the binding's backward, whose bf16 dK/dV reads the scaled-Q workspace):

                  fp16 D = 64      fp16 D = 128     bf16 D = 64      bf16 D = 128
    fwd  O        3.5e-4/2.9e-4    3.3e-4/2.9e-4    5.4e-3/2.9e-3    4.9e-3/2.8e-3
    dq   dQ       6.9e-4/3.0e-4                     6.8e-3/2.9e-3
    dkv  dK raw   8.0e-4/3.0e-4                     1.3e-2/3.0e-3
    dkv  dK ws    8.0e-4/3.0e-4                     7.7e-3/3.4e-3
    dkv  dV raw   3.6e-4/2.9e-4                     1.4e-2/3.0e-3
    dkv  dV ws    3.6e-4/2.9e-4                     8.2e-3/2.9e-3

Outputs of the kernels that fall back to another family in the same runs (D = 128 backward, fp16 causal dK/dV) reach up
to 1.8e-2 (bf16 raw dK at D = 128, family 2) and are held to the same bounds.  The largest block is at most 3.2x the
median of its Q-scale group; LSE is within 3.6e-6 (fp16) and 2.3e-2 (bf16) of logsumexp, delta within 2e-7 relative of
rowsum(dO * O).  The bounds below sit about 1.5x above the largest errors."""
import ctypes
import math

import pytest
import torch

import fa_oracle as fo
from blockcheck import same_bits

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
FWD, DQ, DKV = 0, 1, 2
KERNEL_NAMES = {FWD: "fwd", DQ: "dq", DKV: "dkv"}
Q_SCALES = (0.3, 1.0, 2.5)


# ---------------------------------------------------------------- the launchers' work lists, restated
def cu_count():
    """N: the device's CU count rounded down to a multiple of 8, the persistent grid cap of the family-4 launchers."""
    n = torch.cuda.get_device_properties(0).multi_processor_count
    return n - n % 8


def xcd_remap(i, n):
    """fa_common.h xcd_remap: work-list position of the item workgroup slot i walks."""
    q, r, x, idx = n >> 3, n & 7, i & 7, i >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + idx


def work(kernel, B, H, Sq, Sk, D, causal, N=256):
    """Work list of one family-4 launch (launch_fwd_v4 / launch_bwd_dq_v4 / launch_bwd_dkv_v4 and their launch4): an item
    is one 256-row query tile (forward, dQ) or 256-key tile (dK/dV), or under the causal mask the tile pair (i, n-1-i).
    The forward always pairs causal tiles and is persistent when causal or when its ring runs on (CONT: whole key tiles,
    at least NBUF - 1 of them); the backward kernels pair when the paired grid still fills 256 CUs and are always
    persistent.  nc_stage: the non-causal backward stages the next item's rows (needs three whole 128-row/key tiles)."""
    if kernel == FWD:
        tiles, pair = -(-Sq // 256), causal
        BN, NBUF = (128, 3) if D == 64 else (64, 4)
        persistent = causal or (Sk % BN == 0 and Sk // BN >= NBUF - 1)
        nc_stage = False
    else:
        tiles = -(-(Sq if kernel == DQ else Sk) // 256)
        pair = causal and ((tiles + 1) // 2) * B * H >= 256
        persistent = True
        nc_stage = not causal and (Sk if kernel == DQ else Sq) // 128 >= 3
    per_bh = (tiles + 1) // 2 if pair else tiles
    n_items = per_bh * B * H
    grid = min(n_items, N) if persistent else n_items
    return dict(tiles=tiles, pair=pair, per_bh=per_bh, n_items=n_items, grid=grid, persistent=persistent, nc_stage=nc_stage)


def walk(kernel, B, H, Sq, Sk, D, causal, N=256):
    """Every item of a launch: its workgroup, its position in that workgroup's sequence, whether another item follows it
    there, its (batch, head) and the tiles of its passes in the order they run."""
    w = work(kernel, B, H, Sq, Sk, D, causal, N)
    n, g, per, nt = w["n_items"], w["grid"], w["per_bh"], w["tiles"]
    for it in range(n):
        bh, idx = divmod(xcd_remap(it, n), per)
        if w["pair"]:
            passes = [nt - 1 - idx] + ([idx] if idx != nt - 1 - idx else [])
            if kernel == DKV:
                passes = passes[::-1]
        else:
            passes = [idx]
        yield dict(item=it, wg=it % g, order=it // g, followed=it + g < n, b=bh // H, h=bh % H, passes=passes)


def check_multi_item(kernel, B, H, Sq, Sk, D, causal, N):
    w = work(kernel, B, H, Sq, Sk, D, causal, N)
    if w["persistent"]:
        assert w["n_items"] > w["grid"], (KERNEL_NAMES[kernel], w)
    else:   # the forward without CONT: one workgroup per item, more of them than CUs
        assert w["grid"] == w["n_items"] > N, (KERNEL_NAMES[kernel], w)
    return w


# (B, H, S_q, S_k, D, causal, kernels that take family 4 (dK/dV: not fp16 under the causal mask), dtypes, what it reaches)
# Item counts at N = 256 in the comments: forward / dQ / dK/dV.
CASES = [
    # forward CONT + STAGEQ with a ragged S_q; dQ nc_stage with a ragged S_q; n_items > 2N, n_items % 8 = 6 (xcd_remap remainder)
    (2, 101, 700, 768, 64, False, (FWD, DQ), (F16, BF16), "ragged-cont"),            # 606 / 606
    # the ADVICE.md shape: rows past S_q staged through empty descriptors while the next item is staged
    (6, 48, 700, 768, 64, False, (FWD, DQ), (F16, BF16), "advice"),                   # 864 / 864
    # S_k exactly at the forward's CONT threshold (NBUF - 1 tiles of 128 keys); dQ without nc_stage, ragged S_q
    (2, 101, 700, 256, 64, False, (FWD, DQ), (F16, BF16), "cont-threshold"),          # 606 / 606
    # forward without CONT (S_k not whole 128-key tiles): non-persistent, grid > N
    (2, 101, 700, 320, 64, False, (FWD,), (F16, BF16), "non-persistent"),            # 606 workgroups
    # dK/dV nc_stage (S_q >= 384), ragged S_q for the forward and dQ
    (2, 101, 640, 768, 64, False, (FWD, DQ, DKV), (F16, BF16), "dkv-stage"),         # 606 / 606 / 606
    # dK/dV without nc_stage (S_q = 256)
    (4, 101, 256, 768, 64, False, (FWD, DQ, DKV), (F16, BF16), "dkv-no-stage"),      # 404 / 404 / 1212
    # causal pairs with an odd tile count (one single-pass item per head); N < n_items < 2N
    (2, 50, 1280, 1280, 64, True, (FWD, DQ, DKV), (F16, BF16), "causal-odd"),        # 300 / 300 / 300
    # causal with S_q < S_k (keys no query sees), ragged S_q
    (4, 50, 1000, 1280, 64, True, (FWD, DQ), (F16, BF16), "causal-sq<sk"),           # 400 / 400
    # dK/dV causal with S_q > S_k (bf16 only: the fp16 causal instance does not exist)
    (2, 64, 1536, 1280, 64, True, (DKV,), (BF16,), "dkv-causal-sq>sk"),              # - / - / 384
    # D = 128 forward (64-key tiles, ring of four, no STAGEQ)
    (2, 101, 700, 768, 128, False, (FWD,), (F16, BF16), "d128-ragged-cont"),         # 606
    (2, 101, 700, 192, 128, False, (FWD,), (F16, BF16), "d128-cont-threshold"),      # 606
    (2, 101, 700, 160, 128, False, (FWD,), (F16, BF16), "d128-non-persistent"),      # 606 workgroups
    (2, 50, 1280, 1280, 128, True, (FWD,), (F16, BF16), "d128-causal-odd"),          # 300
    (4, 50, 1000, 1280, 128, True, (FWD,), (F16, BF16), "d128-causal-sq<sk"),        # 400
]
# what bench.py measures (B4 H32 S4096), under the automatic table
HEADLINE = [
    (4, 32, 4096, 4096, 64, True, (FWD, DQ, DKV), (BF16,), "headline-causal"),       # 1024 / 1024 / 1024
    (4, 32, 4096, 4096, 128, True, (FWD,), (BF16,), "headline-causal-d128"),         # 1024
    (4, 32, 4096, 4096, 64, False, (FWD, DQ, DKV), (BF16,), "headline-full"),        # 2048 / 2048 / 2048
]


def kernels_for(case, dtype):
    B, H, Sq, Sk, D, causal, kernels = case[:7]
    return tuple(k for k in kernels if not (k == DKV and causal and dtype == F16))


def case_params(cases):
    return [pytest.param(c, dt, id="%s-%s" % (c[-1], "bf16" if dt == BF16 else "fp16")) for c in cases for dt in c[7]]


# ---------------------------------------------------------------- library hooks
def _lib():
    import _mi355fa as fa
    lib = fa.lib
    lib.fa_debug_force_impl.argtypes = [ctypes.c_int] * 3
    lib.fa_debug_force_impl.restype = None
    lib.fa_debug_pick.argtypes = [ctypes.c_int] * 8
    lib.fa_debug_set_buffer.argtypes = [ctypes.c_void_p]
    lib.fa_debug_set_buffer.restype = None
    return fa, lib


def _host():
    import My_FlashAttention_optimized as M
    return M


def assert_picks(kernels, D, dtype, causal, B, H, Sq, Sk):
    _, lib = _lib()
    for k in kernels:
        got = lib.fa_debug_pick(k, D, int(dtype == BF16), int(causal), B, H, Sq, Sk)
        assert got == 4, (KERNEL_NAMES[k], got)


# ---------------------------------------------------------------- inputs and launches
def make_inputs(B, H, Sq, Sk, D, dtype, seed=0):
    """Q, K, V, dO on the device with per-(batch, head) differences (module docstring), and the Q-scale class of every
    (batch, head) as the block check's groups."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda S: torch.randn(B, H, S, D, device="cuda", generator=g)
    Q, K, V, dO = mk(Sq), mk(Sk), mk(Sk), mk(Sq)
    bh = torch.arange(B * H, device="cuda").reshape(B, H)
    Q *= torch.tensor(Q_SCALES, device="cuda")[bh % 3][..., None, None]
    V[bh % 7 == 0] = 0
    dO[bh % 11 == 0] = 0
    return Q.to(dtype), K.to(dtype), V.to(dtype), dO.to(dtype), bh % 3


def launch_raw(Q, K, V, dO, causal):
    """The three C entry points in a row, every output filled with NaN first (an unwritten element stays NaN)."""
    fa, lib = _lib()
    B, H, Sq, D = Q.shape
    Sk = K.shape[2]
    dt, c, sc = int(Q.dtype == BF16), int(causal), D ** -0.5
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()
    nan = lambda t: torch.full_like(t, float("nan"))
    O, dQ, dK, dV = nan(Q), nan(Q), nan(K), nan(V)
    LSE = torch.full((B, H, Sq), float("nan"), device="cuda")
    delta = torch.full_like(LSE, float("nan"))
    fa.check(lib.fa_fwd(P(Q), P(K), P(V), P(O), P(LSE), B, H, Sq, Sk, D, dt, c, sc, st), "fa_fwd")
    fa.check(lib.fa_bwd_dq(P(Q), P(K), P(V), P(O), P(dO), P(LSE), P(dQ), P(delta), B, H, Sq, Sk, D, dt, c, sc, st), "fa_bwd_dq")
    fa.check(lib.fa_bwd_dkv(P(Q), P(K), P(V), P(dO), P(LSE), P(delta), P(dK), P(dV), B, H, Sq, Sk, D, dt, c, sc, st),
             "fa_bwd_dkv")
    torch.cuda.synchronize()
    return dict(O=O, LSE=LSE, delta=delta, dQ=dQ, dK=dK, dV=dV)


def launch_autograd(Q, K, V, dO, causal):
    """flash_attention and its backward (bf16: the dK/dV launch reads the dQ kernel's scaled-Q workspace)."""
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    o = _host().flash_attention(q, k, v, causal)
    o.backward(dO)
    torch.cuda.synchronize()
    return dict(O=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)


# ---------------------------------------------------------------- the checks
# Per-block relative Frobenius error bounds by (dtype, output), about 1.5x the largest block error measured on an MI355X
# over every case in this file (module docstring), and the limit against the median block error of the same Q scale:
# RATIO x median + FLOOR (measured: at most 3.2x).  bf16 dK / dV from the C entry points without the scaled-Q workspace
# fold the softmax scale into K, a second rounding of the exponent argument whose error grows with the score magnitude
# ("scale fold"; the 2.5x-scaled heads reach 1.6e-2): "raw" has its own bound there; the binding's
# backward ("workspace") recomputes P from the operand LSE came from.
BLOCK_BOUND = {
    (F16, "O"): 1e-3, (F16, "dQ"): 1.2e-3, (F16, "dK"): 1.2e-3, (F16, "dV"): 1e-3,
    (BF16, "O"): 8e-3, (BF16, "dQ"): 1e-2, (BF16, "dK"): 1.6e-2, (BF16, "dV"): 1.2e-2,
}
BLOCK_BOUND_RAW_BF16_DKV = 2.4e-2
RATIO, FLOOR = 4.0, 1e-5
# |LSE - logsumexp| per row: fp16 scores are exact products summed in fp32; bf16 ones carry the folded scale (one rounding
# of the resident operand, unit roundoff 2^-9), which moves a score, hence the LSE, by at most 2^-9 * SABS -- bounded at 2x
# that, plus a floor
LSE_BOUND = {F16: (1e-4, 0.0), BF16: (1e-3, 2.0 ** -8)}
DELTA_BOUND = 1e-6                            # |delta - rowsum(dO * O)| / rowsum(|dO * O|), per row


def check_outputs(tag, gt, got, dO, groups, dtype, mode="raw", check=True):
    """Block-check every output in `got` against the fp64 `gt`; returns one record per output (max, median, ratio)."""
    recs = []
    for n in ("O", "dQ", "dK", "dV"):
        if n not in got:
            continue
        st = fo.block_stats(gt[n], got[n], groups)
        recs.append(dict(tag=tag, out=n, max=st["max"], median=st["median"], max_ratio=st["max_ratio"], worst=st["worst"]))
        bound = BLOCK_BOUND[dtype, n]
        if mode == "raw" and dtype == BF16 and n in ("dK", "dV"):
            bound = BLOCK_BOUND_RAW_BF16_DKV
        if check:
            fo.assert_blocks("%s %s" % (tag, n), st, bound, RATIO, FLOOR)
    if "LSE" in got:
        err = (got["LSE"].double() - gt["LSE"]).abs()
        err = torch.where(torch.isnan(err), float("inf"), err)
        a, u = LSE_BOUND[dtype]
        excess = err / (a + u * gt["SABS"])
        at = tuple(int(x) for x in torch.unravel_index(excess.argmax(), err.shape))
        recs.append(dict(tag=tag, out="LSE", max=err.max().item(), median=err.median().item(), worst=at,
                         max_excess=excess.max().item()))
        if check:
            assert excess.max() <= 1, "%s LSE: row (b, h, row) %s off by %.3e (bound %.3e)" % (
                tag, at, err[at].item(), a + u * gt["SABS"][at].item())
    if "delta" in got:
        prod = dO.double() * got["O"].double()
        err = (got["delta"].double() - prod.sum(-1)).abs() / prod.abs().sum(-1).clamp_min(1e-30)
        err = torch.where(torch.isnan(err), float("inf"), err)
        at = tuple(int(x) for x in torch.unravel_index(err.argmax(), err.shape))
        recs.append(dict(tag=tag, out="delta", max=err.max().item(), median=err.median().item(), worst=at))
        if check:
            assert err.max() <= DELTA_BOUND, "%s delta: row (b, h, row) %s off by %.3e" % (tag, at, err.max().item())
    return recs


def check_special_heads(tag, got, B, H):
    """V = 0 heads: O, dQ, dK exactly 0, dV not; dO = 0 heads: dQ, dK, dV exactly 0."""
    bh = torch.arange(B * H, device="cuda").reshape(B, H)
    v0, d0 = bh % 7 == 0, bh % 11 == 0
    for n in ("O", "dQ", "dK"):
        assert (got[n][v0] == 0).all(), (tag, n, "V = 0")
    assert (got["dV"][v0 & ~d0] != 0).any(dim=-1).any(dim=-1).all(), (tag, "dV of a V = 0 head")
    for n in ("dQ", "dK", "dV"):
        assert (got[n][d0] == 0).all(), (tag, n, "dO = 0")


def run_case(case, dtype, forced=True, check=True, seed=0):
    """One case: work-list and family assertions, raw launches twice (bit-identical), the autograd path once, and every
    output against fp64.  Returns the error records (check=False: measure only)."""
    B, H, Sq, Sk, D, causal = case[:6]
    kernels = kernels_for(case, dtype)
    N = cu_count()
    for k in kernels:
        check_multi_item(k, B, H, Sq, Sk, D, causal, N)
    Q, K, V, dO, groups = make_inputs(B, H, Sq, Sk, D, dtype, seed)
    gt = fo.attention_fp64_chunked(Q, K, V, dO, causal)
    _, lib = _lib()
    lib.fa_debug_force_impl(*((4, 4, 4) if forced else (0, 0, 0)))
    try:
        assert_picks(kernels, D, dtype, causal, B, H, Sq, Sk)
        raw = launch_raw(Q, K, V, dO, causal)
        raw2 = launch_raw(Q, K, V, dO, causal)
        ag = launch_autograd(Q, K, V, dO, causal)
    finally:
        lib.fa_debug_force_impl(0, 0, 0)
    tag = "%s %s" % (case[-1], "bf16" if dtype == BF16 else "fp16")
    for n in raw:
        assert same_bits(raw[n], raw2[n]), (tag, n, "second launch")
    assert same_bits(raw["O"], ag["O"]) and same_bits(raw["dQ"], ag["dQ"]), tag
    if check:
        check_special_heads(tag + " raw", raw, B, H)
        check_special_heads(tag + " autograd", ag, B, H)
    recs = check_outputs(tag + " raw", gt, raw, dO, groups, dtype, "raw", check)
    recs += check_outputs(tag + " autograd", gt, {n: ag[n] for n in ("dK", "dV")}, dO, groups, dtype, "workspace", check)
    for r in recs:
        r.update(dtype="bf16" if dtype == BF16 else "fp16", D=D, causal=causal, kernels=[KERNEL_NAMES[k] for k in kernels])
    return recs


# ---------------------------------------------------------------- tests
def test_device_fp64_reference_matches_the_cpu_oracle():
    """The device reference every other test here uses, against fa_oracle.attention_fp64 on the CPU for a few (batch,
    head) slices of a multi-item shape, causal and full (slices chosen to include a V = 0 and a dO = 0 head)."""
    B, H, Sq, Sk, D = 2, 101, 700, 768, 64
    Q, K, V, dO, _ = make_inputs(B, H, Sq, Sk, D, BF16)
    for causal in (False, True):
        gt = fo.attention_fp64_chunked(Q, K, V, dO, causal)
        for b, h in ((0, 0), (0, 11), (1, 57)):
            cpu = fo.attention_fp64(*(x[b:b + 1, h:h + 1].cpu() for x in (Q, K, V, dO)), is_causal=causal)
            for n in ("O", "LSE", "dQ", "dK", "dV", "delta"):
                d = gt[n][b:b + 1, h:h + 1].cpu()
                assert (d - cpu[n]).abs().max() <= 1e-10 * max(cpu[n].abs().max().item(), 1e-300), (causal, b, h, n)


@pytest.mark.parametrize("case,dtype", case_params(CASES))
def test_persistent_items_against_fp64(case, dtype):
    run_case(case, dtype)


@pytest.mark.parametrize("case,dtype", case_params(HEADLINE))
def test_headline_shapes_against_fp64(case, dtype):
    """What bench.py measures, under the automatic schedule table (asserted to pick family 4)."""
    run_case(case, dtype, forced=False)


STRIDED = [
    (2, 101, 768, 768, 64, False, (FWD, DQ, DKV), (F16, BF16), "strided-full"),      # 606 / 606 / 606
    (2, 50, 1280, 1280, 64, True, (FWD, DQ, DKV), (BF16,), "strided-causal"),        # 300 / 300 / 300
]


@pytest.mark.parametrize("case,dtype", case_params(STRIDED))
def test_strided_views_take_family4_and_match_the_contiguous_launch(case, dtype):
    """Q/K/V as views of a fused [B, S, 3, H, D] projection, dO as a view of [B, S, H, D]: all three kernels take family 4
    (only family 2 needs contiguous tensors), read the views in place, write the outputs in the views' memory order, and give
    the bits of the contiguous launch; and the block check against fp64."""
    B, H, S, _, D, causal = case[:6]
    kernels = kernels_for(case, dtype)
    N = cu_count()
    for k in kernels:
        check_multi_item(k, B, H, S, S, D, causal, N)
    fa, lib = _lib()
    M = _host()
    Q, K, V, dO, groups = make_inputs(B, H, S, S, D, dtype, seed=1)
    qkv = torch.stack([x.transpose(1, 2) for x in (Q, K, V)], dim=2).contiguous()       # [B, S, 3, H, D]
    Qv, Kv, Vv = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    dOv = dO.transpose(1, 2).contiguous().transpose(1, 2)
    for t in (Qv, Kv, Vv, dOv):
        assert not t.is_contiguous() and fa.strided_ok(t)
    lib.fa_debug_force_impl(4, 4, 4)
    try:
        assert_picks(kernels, D, dtype, causal, B, H, S, S)
        O1, L1 = M.flash_attention_forward(Qv, Kv, Vv, causal)
        g1 = M.flash_attention_backward(Qv, Kv, Vv, O1, dOv, L1, causal)
        O2, L2 = M.flash_attention_forward(Q, K, V, causal)
        g2 = M.flash_attention_backward(Q, K, V, O2, dO, L2, causal)
        torch.cuda.synchronize()
    finally:
        lib.fa_debug_force_impl(0, 0, 0)
    assert O1.transpose(1, 2).is_contiguous() and all(t.transpose(1, 2).is_contiguous() for t in g1)
    for n, a, b in zip(("O", "LSE", "dQ", "dK", "dV"), (O1, L1) + tuple(g1), (O2, L2) + tuple(g2)):
        assert same_bits(a, b), n
    gt = fo.attention_fp64_chunked(Q, K, V, dO, causal)
    check_outputs(case[-1], gt, dict(O=O1, LSE=L1, dQ=g1[0], dK=g1[1], dV=g1[2]), dO, groups, dtype, "workspace")


# forward launches for the overflow redo: (B, H, S_q, S_k, causal) -- multi-item, causal pairs and non-causal CONT
OVERFLOW = [(2, 50, 1280, 1280, True), (2, 101, 700, 768, False)]
SPIKE_SCORE = {F16: 20.0, BF16: 90.0}   # natural-log score of a spiked row at its spike key (row limits: 2^15, 2^100)


def spiked_passes(B, H, Sq, Sk, D, causal, N):
    """(b, h, query tile) passes to spike, chosen on the work list: passes of items that are not their workgroup's first,
    passes followed by another item, and (causal) first passes followed by the pair's second."""
    its = list(walk(FWD, B, H, Sq, Sk, D, causal, N))
    later = [i for i in its if i["order"] > 0]
    followed = [i for i in its if i["followed"]]
    pick = []
    for src, k in ((later, 4), (followed, 4), ([i for i in later if i["followed"]], 3)):
        step = max(1, len(src) // k)
        for i in src[::step][:k]:
            p = i["passes"][-1] if len(pick) % 2 else i["passes"][0]
            pick.append((i["b"], i["h"], p, i["order"], i["followed"]))
    seen, out = set(), []
    for b, h, t, order, followed in pick:
        if (b, h, t) not in seen:
            seen.add((b, h, t))
            out.append((b, h, t, order, followed))
    return out


def overflowing_passes(Q, K, causal, limit):
    """The passes whose row sums exceed the family-4 forward's limit when the row constant is the maximum over the row's
    first 32 keys (fa_fwd_v4.hip, end-of-pass check), evaluated in fp64: set of (b, h, query tile)."""
    B, H, Sq, D = Q.shape
    Sk = K.shape[2]
    out = set()
    hidden = torch.arange(Sq, device="cuda")[:, None] < torch.arange(Sk, device="cuda")[None, :]
    for b in range(B):
        s = torch.matmul(Q[b].double(), K[b].double().transpose(1, 2)) / math.sqrt(D)
        if causal:
            s.masked_fill_(hidden, float("-inf"))
        m = s[..., :32].max(-1, keepdim=True).values
        l = (s - m).exp().sum(-1)
        for h, row in (l > limit).nonzero().tolist():
            out.add((b, h, row // 256))
    return out


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_overflow_second_attempt_across_items(dtype, D):
    """The forward's exact second attempt (a row sum over the limit: the pass is redone with exact row maxima) in passes
    that are not their workgroup's first, and in passes another item follows -- the redo restarts the ring while the next
    pass's tiles are in flight.  Spikes: key j = Q row r scaled so that score(r, j) sits far beyond the limit while no other
    row comes near it (asserted in fp64).  The debug counter equals the number of spiked passes, and every block, those of
    the items after a redo included, holds the bounds of the other tests."""
    fa, lib = _lib()
    N = cu_count()
    counter = torch.zeros(4, dtype=torch.int32, device="cuda")
    for (B, H, Sq, Sk, causal) in OVERFLOW:
        check_multi_item(FWD, B, H, Sq, Sk, D, causal, N)
        spikes = spiked_passes(B, H, Sq, Sk, D, causal, N)
        assert any(o > 0 for *_, o, f in spikes) and any(f for *_, o, f in spikes)
        g = torch.Generator(device="cuda").manual_seed(7)
        Q, K, V = (torch.randn(B, H, S, D, device="cuda", generator=g) for S in (Sq, Sk, Sk))
        keys = set()
        for j, (b, h, t, _, _) in enumerate(spikes):
            row = min(t * 256 + 57 + 11 * j, Sq - 1)
            key = row - 9 if causal else 32 + (row * 37) % (Sk - 32)
            assert key >= 32 and (b, h, key) not in keys
            keys.add((b, h, key))
            q = Q[b, h, row]
            K[b, h, key] = q * (SPIKE_SCORE[dtype] * math.sqrt(D) / q.square().sum())
        Q, K, V = Q.to(dtype), K.to(dtype), V.to(dtype)
        limit = 32768.0 if dtype == F16 else 2.0 ** 100
        assert overflowing_passes(Q, K, causal, limit) == {s[:3] for s in spikes}
        gt = fo.attention_fp64_chunked(Q, K, V, None, causal)
        torch.cuda.synchronize()
        before = int(counter[0].item())
        lib.fa_debug_force_impl(4, 0, 0)
        lib.fa_debug_set_buffer(counter.data_ptr())
        try:
            assert_picks((FWD,), D, dtype, causal, B, H, Sq, Sk)
            O, LSE = _host().flash_attention_forward(Q, K, V, causal)
            torch.cuda.synchronize()
        finally:
            lib.fa_debug_set_buffer(None)
            lib.fa_debug_force_impl(0, 0, 0)
        assert int(counter[0].item()) - before == len(spikes), (causal, int(counter[0].item()) - before, len(spikes))
        check_outputs("overflow %s" % ("causal" if causal else "full"), gt, dict(O=O, LSE=LSE), None, None, dtype)
