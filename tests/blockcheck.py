"""Helpers shared by the per-block fp64 checks of tests/test_gpu_blockwise.py, test_gpu_families.py, test_gpu_varlen.py
and test_gpu_dropout.py (not a test module): the inputs with per-head differences, the block / row / structural-zero check,
the packed-batch reference and the NaN-poisoned launches of the plain fixed-length, packed and dropout kernels.  The
bounds each check holds to stay in the calling file, next to the errors they were measured from."""
import ctypes
import random

import torch

import fa_oracle as fo

F16, BF16 = torch.float16, torch.bfloat16
FWD, DQ, DKV = 0, 1, 2
KERNEL_NAMES = {FWD: "fwd", DQ: "dq", DKV: "dkv"}
Q_SCALES = (0.3, 1.0, 2.5)


def _lib():
    import _mi355fa as fa
    lib = fa.lib
    lib.fa_debug_force_impl.argtypes = [ctypes.c_int] * 3
    lib.fa_debug_force_impl.restype = None
    lib.fa_debug_pick.argtypes = [ctypes.c_int] * 8
    lib.fa_debug_pick_ex.argtypes = [ctypes.c_int] * 11
    return fa, lib


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


def same_bits(a, b):
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.view(iv), b.view(iv))


# ---------------------------------------------------------------- the checks
FEW = 8      # rows that see fewer keys are checked row by row (test_gpu_blockwise.py FEW_BOUND)


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


def check_outputs(tag, gt, got, dO, groups, kv_groups, dtype, mode, bounds, check=True, V=None, few=None):
    """Block-check every output in `got` against the fp64 `gt` (all [B, H(_kv), S, D] / [B, H, S]); exact zeros where
    they are structural; no NaN.  bounds: the calling file's measured limits, a dict of BLOCK_BOUND,
    BLOCK_BOUND_RAW_BF16_DKV, FEW_BOUND, RATIO, FLOOR, LSE_BOUND and DELTA_BOUND.  few: ([S_q], [S_k]) bool rows of
    few_rows, checked absolutely.  Returns one record per output."""
    recs = []
    for n in ("O", "dQ", "dK", "dV"):
        if n not in got:
            continue
        t = got[n]
        zero_rows = structural_zeros(n, gt, dO, V) if V is not None else (gt[n] == 0).all(-1)
        if V is None and few is not None and n in ("dQ", "dK"):   # a few-key row's fp64 0 is a cancellation: checked below
            zero_rows = zero_rows & ~few[0 if n == "dQ" else 1].to(zero_rows.device)
        recs.append(dict(tag=tag, out=n, nan=bool(torch.isnan(t).any()),
                         zeros_ok=bool((t[zero_rows] == 0).all()), n_zero_rows=int(zero_rows.sum())))
        bound = bounds["BLOCK_BOUND"][dtype, n]
        if mode == "raw" and dtype == BF16 and n in ("dK", "dV"):
            bound = bounds["BLOCK_BOUND_RAW_BF16_DKV"]
        r = gt[n]
        rows = None if few is None or n not in ("dQ", "dK") else few[0 if n == "dQ" else 1].to(r.device)
        if rows is not None and bool(rows.any()):
            rms = r.square().sum(-1).mean(-1).sqrt()[..., None]               # [B, H(_kv), 1]
            scale = torch.maximum(r[..., rows, :].norm(dim=-1), rms)
            aerr = (t.double()[..., rows, :] - r[..., rows, :]).norm(dim=-1) / scale.clamp_min(1e-300)
            aerr = torch.where(torch.isnan(aerr), float("inf"), aerr)
            recs[-1].update(few_rows=int(rows.sum()), few_max=aerr.max().item())
            if check:
                assert aerr.max() <= bounds["FEW_BOUND"][dtype], (tag, n, "a row with few keys is off by %.3e" % aerr.max())
            keep = ~rows
            r, t = r[..., keep, :], t[..., keep, :]
        st = fo.block_stats(r, t, groups if n in ("O", "dQ") else kv_groups)
        recs[-1].update(max=st["max"], median=st["median"], max_ratio=st["max_ratio"], worst=st["worst"])
        if check:
            assert not recs[-1]["nan"], (tag, n, "NaN")
            assert recs[-1]["zeros_ok"], (tag, n, "a row that is exactly 0 in fp64 is not exactly 0")
            fo.assert_blocks("%s %s" % (tag, n), st, bound, bounds["RATIO"], bounds["FLOOR"])
    if "LSE" in got:
        L, R = got["LSE"].double(), gt["LSE"]
        inf_ok = torch.equal(torch.isneginf(L), torch.isneginf(R))
        fin = torch.isfinite(R)
        err = torch.where(fin, (L - R).abs(), torch.zeros_like(R))
        err = torch.where(torch.isnan(L), float("inf"), err)
        a, u = bounds["LSE_BOUND"][dtype]
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
            assert err.max() <= bounds["DELTA_BOUND"], "%s delta: off by %.3e" % (tag, err.max().item())
    return recs


def kv_groups_of(B, H, Hkv, groups):
    """block_stats groups of dK / dV: the Q-scale class when g = 1, else one group (every K/V head mixes the scales)."""
    return groups if H == Hkv else None


# ---------------------------------------------------------------- packed variable-length batches
def packed_lengths(n=32, cap=4096, seed=5):
    """n (S_q, S_k) pairs up to `cap`: ragged, with an empty sequence on either side and a few at the cap (at n = 32
    sequences 3, 11, 17, 24 and 29; a smaller n places them at the same fractions of n, a smaller cap clips them)."""
    rnd = random.Random(seed)
    lens = [(rnd.randint(1, cap), rnd.randint(1, cap)) for _ in range(n)]
    for i, (lq, lk) in ((3, (0, 700)), (11, (913, 0)), (17, (cap, cap)), (24, (1, cap)), (29, (cap, 129))):
        lens[i * n // 32] = (min(lq, cap), min(lk, cap))
    return lens


def packed_reference(Q, K, V, dO, cu_q, cu_k, window, dropout=None):
    """Per-sequence attention_fp64_chunked, assembled into packed [1, H, T, D] (O, dQ), [1, H_kv, T_k, D] (dK, dV),
    [1, H, T] (LSE, SABS); a sequence without keys: O = 0, LSE = -inf, dQ = 0; without queries: dK = dV = 0.
    dropout: (p_drop, seed, offset); sequence b takes the keep mask of batch b."""
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
        drop = None if dropout is None else tuple(dropout) + (b,)
        r = fo.attention_fp64_chunked(sl(Q, q0, q1), sl(K, k0, k1), sl(V, k0, k1), sl(dO, q0, q1), window=window,
                                      dropout=drop)
        for n in ("O", "dQ", "LSE", "SABS"):
            out[n][:, :, q0:q1] = r[n]
        for n in ("dK", "dV"):
            out[n][:, :, k0:k1] = r[n]
    return out


# ---------------------------------------------------------------- the plain kernels (families 1-4, packed, dropout)
def launch_plain(Q, K, V, dO, causal, workspace, dims=None, varlen=None, dropout=None):
    """fa_fwd_ex, fa_bwd_dq_ex, fa_bwd_dkv_ex through ctypes, every output and the workspace NaN-filled first (an element
    a kernel skips stays NaN).  dims: (B, H, S_q, S_k, D) when the tensors are packed [T, H, D]; varlen: (cu_q, cu_k)
    int32 device tensors; dropout: (p_drop, seed, offset)."""
    fa, lib = _lib()
    B, H, Sq, Sk, D = dims or (Q.shape[0], Q.shape[1], Q.shape[2], K.shape[2], Q.shape[3])
    dt, c, sc = int(Q.dtype == BF16), int(causal), D ** -0.5
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()
    nan = lambda t: torch.full_like(t, float("nan"))
    O, dQ, dK, dV = nan(Q), nan(Q), nan(K), nan(V)
    LSE = torch.full((H, Q.shape[0]) if varlen else (B, H, Sq), float("nan"), device="cuda")
    delta = torch.full_like(LSE, float("nan"))
    qs = nan(Q) if workspace else None
    kw = {}
    if varlen:
        kw.update(cu_seqlens_q=P(varlen[0]), cu_seqlens_k=P(varlen[1]), total_q=Q.shape[0], total_k=K.shape[0])
    if dropout:
        kw.update(p_drop=dropout[0], seed=dropout[1], offset=dropout[2])
    of = ctypes.byref(fa.Opts.make(**kw))
    ob = ctypes.byref(fa.Opts.make(q_scaled=P(qs) if qs is not None else None, **kw))
    fa.check(lib.fa_fwd_ex(P(Q), P(K), P(V), P(O), P(LSE), B, H, Sq, Sk, D, dt, c, sc, of, st), "fa_fwd_ex")
    fa.check(lib.fa_bwd_dq_ex(P(Q), P(K), P(V), P(O), P(dO), P(LSE), P(dQ), P(delta), B, H, Sq, Sk, D, dt, c, sc, ob, st),
             "fa_bwd_dq_ex")
    fa.check(lib.fa_bwd_dkv_ex(P(Q), P(K), P(V), P(dO), P(LSE), P(delta), P(dK), P(dV), B, H, Sq, Sk, D, dt, c, sc, ob, st),
             "fa_bwd_dkv_ex")
    torch.cuda.synchronize()
    return dict(O=O, LSE=LSE, delta=delta, dQ=dQ, dK=dK, dV=dV, qs=qs)


def launch_plain_autograd(Q, K, V, dO, causal, varlen=None, max_seqlen=None, dropout=None):
    """flash_attention / flash_attention_dropout / flash_attention_varlen and the backward through the binding."""
    import My_FlashAttention_optimized as M
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    p, seed, offset = dropout or (0.0, 0, 0)
    if varlen:
        o = M.flash_attention_varlen(q, k, v, varlen[0], varlen[1], max_seqlen[0], max_seqlen[1], causal, p, seed, offset)
    elif dropout:
        o = M.flash_attention_dropout(q, k, v, causal, p, seed, offset)
    else:
        o = M.flash_attention(q, k, v, causal)
    o.backward(dO)
    torch.cuda.synchronize()
    return dict(O=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)


def assert_family(kernel, expected, D, dtype, causal, B, H, Sq, Sk, varlen=False, contiguous=True, dropout=False):
    """fa_debug_pick_ex: the family the launch really takes."""
    _, lib = _lib()
    got = lib.fa_debug_pick_ex(kernel, D, int(dtype == BF16), int(causal), B, H, Sq, Sk, int(varlen), int(contiguous),
                               int(dropout))
    assert got == expected, (KERNEL_NAMES[kernel], "takes family %d, expected %d" % (got, expected))


def want_pairs(kernel, family, B, H, Sq, Sk, causal):
    """Whether a causal launch of families 1-3 pairs its query / key tiles (i, n-1-i): fa_kernels.h want_pairs with the
    launcher's own tile -- 128 rows or keys, 256 for the dK/dV family 3; the forward family 2 (256-row tiles) pairs every
    causal launch."""
    if not causal:
        return False
    if kernel == FWD and family == 2:
        return True
    tile = 256 if (kernel == DKV and family == 3) else 128
    tiles = -(-(Sk if kernel == DKV else Sq) // tile)
    return ((tiles + 1) // 2) * B * H >= 256


def grid_size(kernel, family, B, H, Sq, Sk, causal):
    """Workgroups of a launch of families 1-3 (fixed length)."""
    tile = 256 if (kernel != DKV and family == 2) or (kernel == DKV and family == 3) else 128
    tiles = -(-(Sk if kernel == DKV else Sq) // tile)
    return ((tiles + 1) // 2 if want_pairs(kernel, family, B, H, Sq, Sk, causal) else tiles) * B * H


def plain_packed_lengths():
    """32 (S_q, S_k) pairs up to 4096 for the plain packed kernels: S_q != S_k in every sequence but the empty ones, an empty
    sequence on either side, one of length 1, and lengths one row either side of 128 / 256 multiples."""
    lens = [(a, b if b != a else b + 1) for a, b in packed_lengths(32, 4096, seed=11)]
    lens[2], lens[3], lens[7], lens[11] = (0, 700), (1, 257), (129, 127), (913, 0)
    lens[13], lens[17], lens[19], lens[23] = (255, 257), (4096, 4095), (4095, 4096), (2049, 2047)
    lens[27], lens[30] = (511, 513), (3841, 383)
    return lens


def run_packed_plain(H, D, dtype, causal, forced, bounds, dropout=None, check=True, seed=3):
    """A packed batch of plain_packed_lengths through fa_*_ex with cu_seqlens, once per entry of `forced` ((fwd, dQ, dK/dV)
    families for fa_debug_force_impl, (0, 0, 0) = the automatic rule; fa_debug_pick_ex(varlen=1) names the family each
    launch takes), then the autograd function once.  The tensors carry rows past the last sequence (cu_seqlens[batch] <
    total): their NaN bits must survive every launch.  Returns the error records and the families taken."""
    fa, lib = _lib()
    lens = plain_packed_lengths()
    cu_q, cu_k = [0], [0]
    for lq, lk in lens:
        cu_q.append(cu_q[-1] + lq)
        cu_k.append(cu_k[-1] + lk)
    Tq, Tk = cu_q[-1] + 37, cu_k[-1] + 45                       # rows no sequence owns
    Q4, K4, V4, dO4, groups = make_inputs(1, H, H, Tq, Tk, D, dtype, seed)
    pk = lambda t: t[0].transpose(0, 1).contiguous()
    up = lambda t: t.transpose(0, 1).unsqueeze(0)
    Q, K, V, dO = pk(Q4), pk(K4), pk(V4), pk(dO4)
    cq = torch.tensor(cu_q, dtype=torch.int32, device="cuda")
    ck = torch.tensor(cu_k, dtype=torch.int32, device="cuda")
    mq, mk = max(l[0] for l in lens), max(l[1] for l in lens)
    window = (-1, 0) if causal else None
    gt = packed_reference(Q, K, V, dO, cu_q, cu_k, window, dropout)
    for n in ("O", "dQ", "LSE"):                                 # unowned rows: nothing to compare
        gt[n] = gt[n][:, :, :cu_q[-1]]
    for n in ("dK", "dV"):
        gt[n] = gt[n][:, :, :cu_k[-1]]
    gt["SABS"] = gt["SABS"][:, :, :cu_q[-1]]
    few_q = torch.zeros(cu_q[-1], dtype=torch.bool, device="cuda")
    few_k = torch.zeros(cu_k[-1], dtype=torch.bool, device="cuda")
    for b, (lq, lk) in enumerate(lens):
        if lq and lk:
            fq, fk = few_rows(fo.visible_mask(lq, lk, window or (-1, -1), "cuda"))
            few_q[cu_q[b]:cu_q[b + 1]], few_k[cu_k[b]:cu_k[b + 1]] = fq, fk
    cw = dict(check=check, V=None if dropout else V4[:, :, :cu_k[-1]], few=(few_q, few_k))
    dOc = dO4[:, :, :cu_q[-1]]
    nanq = torch.full((Tq - cu_q[-1], H, D), float("nan"), dtype=dtype, device="cuda")
    nank = torch.full((Tk - cu_k[-1], H, D), float("nan"), dtype=dtype, device="cuda")
    nanl = torch.full((H, Tq - cu_q[-1]), float("nan"), device="cuda")
    dims = (len(lens), H, mq, mk, D)
    recs, taken = [], []
    tag = "packed H%d D%d %s %s" % (H, D, "bf16" if dtype == BF16 else "fp16", "causal" if causal else "full")
    runs = [(f, False) for f in forced] + ([(forced[0], True)] if dtype == BF16 else [])
    try:
        for f, wsp in runs:
            lib.fa_debug_force_impl(*f)
            fams = tuple(lib.fa_debug_pick_ex(k, D, int(dtype == BF16), int(causal), len(lens), H, mq, mk, 1, 0, int(bool(dropout)))
                         for k in (FWD, DQ, DKV))
            taken.append(fams)
            r = launch_plain(Q, K, V, dO, causal, wsp, dims=dims, varlen=(cq, ck), dropout=dropout)
            t = "%s forced %s -> %s%s" % (tag, f, fams, " ws" if wsp else "")
            for n, nanrows in (("O", nanq), ("dQ", nanq), ("dK", nank), ("dV", nank)):
                assert same_bits(r[n][(cu_k if n in ("dK", "dV") else cu_q)[-1]:], nanrows), (t, n, "rows past the last sequence")
            for n in ("LSE", "delta"):
                assert same_bits(r[n][:, cu_q[-1]:], nanl), (t, n, "rows past the last sequence")
            got = {n: up(r[n][:(cu_k if n in ("dK", "dV") else cu_q)[-1]]) for n in ("O", "dQ", "dK", "dV")}
            got.update(LSE=r["LSE"][:, :cu_q[-1]].unsqueeze(0), delta=r["delta"][:, :cu_q[-1]].unsqueeze(0))
            recs += check_outputs(t, gt, got, dOc, groups, groups, dtype, "ws" if wsp else "raw", bounds, **cw)
    finally:
        lib.fa_debug_force_impl(0, 0, 0)
    sl = lambda t, n: t[:n].contiguous()
    Qa, Ka, Va, dOa = sl(Q, cu_q[-1]), sl(K, cu_k[-1]), sl(V, cu_k[-1]), sl(dO, cu_q[-1])
    ag = launch_plain_autograd(Qa, Ka, Va, dOa, causal, varlen=(cq, ck), max_seqlen=(mq, mk), dropout=dropout)
    recs += check_outputs(tag + " autograd", gt, {n: up(x) for n, x in ag.items()}, dOc, groups, groups, dtype, "ws", bounds, **cw)
    for r in recs:
        r.update(dtype="bf16" if dtype == BF16 else "fp16", D=D, causal=causal)
    return recs, taken
