"""Helpers shared by the tests of the three score transforms -- soft-capping, ALiBi and attention sinks
(tests/test_gpu_softcap.py, test_gpu_alibi.py, test_gpu_sink.py and their test_host_* twins; not a test module): the
inputs, the autograd and C-ABI runs, the training check (relFro, blocks, LSE rows, structural zeros, "the transform must
matter"), the packed batch, the decode loop over forced split counts, the graph replay, and the host-side entry-point
calls with the refusals every variant shares.  A test file passes in what differs: a callable, the C arguments spliced in
after `scale`, the keywords of attn_ref.attention_fp64, and its own bounds, which stay in that file next to the errors
they were measured from (no bound has a default here).  tests/test_host_variantcheck.py checks on the CPU that the
training check still refuses a wrong block, row or LSE."""
import ctypes
import math
import re

import pytest
import torch

import attn_ref as ar
import blockcheck as bc
import fa_oracle as fo

F16, BF16 = torch.float16, torch.bfloat16


def M():
    import My_FlashAttention_optimized as M
    return M


# ---------------------------------------------------------------- training (GPU)
def inputs(B, H, Hkv, Sq, Sk, D, dtype, seed, amp=1.0):
    """Q (x amp), K, V, dO drawn in this order from one device generator, then cast."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    Q = torch.randn(B, H, Sq, D, device="cuda", generator=g) * amp
    K, V = (torch.randn(B, Hkv, Sk, D, device="cuda", generator=g) for _ in range(2))
    dO = torch.randn(B, H, Sq, D, device="cuda", generator=g)
    return Q.to(dtype), K.to(dtype), V.to(dtype), dO.to(dtype)


def autograd_run(call, Q, K, V, dO, extra=None):
    """call(q, k, v) -- or call(q, k, v, extra) -- on fresh leaves, then the backward: O, dQ, dK, dV, and dz when extra
    requires grad."""
    q, k, v = (x.detach().clone().requires_grad_(True) for x in (Q, K, V))
    o = call(q, k, v) if extra is None else call(q, k, v, extra)
    o.backward(dO)
    if Q.is_cuda:
        torch.cuda.synchronize()
    out = dict(O=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)
    if extra is not None and extra.requires_grad:
        out["dz"] = extra.grad
    return out


def raw_run(names, extra_args, Q, K, V, dO, window, scale, workspace, dsink=None, bufs=None, stages=None, packed=None):
    """The C ABI directly (contiguous inputs): the (fwd, dQ, dK/dV) entry points `names` with extra_args spliced in after
    the scale, with or without the bf16 q_scaled workspace; LSE and delta start as NaN.  dsink: the sinks of the sink
    variant, whose backward is the plain GQA pair (extra_args go to the forward only) and then fa_bwd_dsink into a
    NaN-filled dz (overwritten, not accumulated).  The fa_*_local entry points take no H_kv.
    bufs: tensors to use for O, LSE, dQ, dK, dV, delta, qs, dz instead of fresh ones (the caller fills them; a stage reads
    what an earlier call left in them); stages: the launches to make, of "fwd", "dq", "dkv", "dsink" (all by default) --
    with `stages` given nothing waits for the device (tests/racecheck.py).  packed: (cu_seqlens_q, cu_seqlens_k, batch,
    the longest S_q, the longest S_k) for packed Q, dO [T_q, H, D], K, V [T_k, H_kv, D]; LSE and delta are [H, T_q]."""
    import _mi355fa as fa
    if packed is None:
        B, H, Sq, D = Q.shape
        Hkv, Sk = K.shape[1], K.shape[2]
        lse_shape, kw = (B, H, Sq), {}
    else:
        cu_q, cu_k, B, Sq, Sk = packed
        (Tq, H, D), (Tk, Hkv) = Q.shape, K.shape[:2]
        lse_shape = (H, Tq)
        kw = dict(cu_seqlens_q=cu_q.data_ptr(), cu_seqlens_k=cu_k.data_ptr(), total_q=Tq, total_k=Tk)
    dt = fa.BF16 if Q.dtype == BF16 else fa.FP16
    bufs = dict(bufs or {})
    get = lambda n, make: bufs[n] if n in bufs else make()
    O = get("O", lambda: torch.empty_like(Q))
    LSE = get("LSE", lambda: torch.full(lse_shape, float("nan"), device="cuda", dtype=torch.float32))
    dQ, dK, dV = get("dQ", lambda: torch.empty_like(Q)), get("dK", lambda: torch.empty_like(K)), get("dV", lambda: torch.empty_like(V))
    delta = get("delta", lambda: torch.full_like(LSE, float("nan")))
    qs = get("qs", lambda: torch.empty_like(Q)) if workspace else None
    of = ctypes.byref(fa.Opts.make(**kw)) if kw else None
    ob = ctypes.byref(fa.Opts.make(q_scaled=qs.data_ptr(), **kw)) if workspace else of
    p = lambda t: t.data_ptr()
    fwd, dq, dkv = (getattr(fa.lib, n) for n in names)
    heads = (H,) if names[0].endswith("_local") else (H, Hkv)
    dims = (B, *heads, Sq, Sk, D, dt, scale)
    bwd_args = () if dsink is not None else tuple(extra_args)
    run = ("fwd", "dq", "dkv", "dsink") if stages is None else stages
    if "fwd" in run:
        fa.check(fwd(p(Q), p(K), p(V), p(O), p(LSE), *dims, *extra_args, *window, of, None), names[0])
    if "dq" in run:
        fa.check(dq(p(Q), p(K), p(V), p(O), p(dO), p(LSE), p(dQ), p(delta), *dims, *bwd_args, *window, ob, None), names[1])
    if "dkv" in run:
        fa.check(dkv(p(Q), p(K), p(V), p(dO), p(LSE), p(delta), p(dK), p(dV), *dims, *bwd_args, *window, ob, None), names[2])
    out = dict(O=O, LSE=LSE, dQ=dQ, dK=dK, dV=dV)
    if stages is not None:
        out.update(delta=delta, qs=qs)
    if dsink is not None and "dsink" in run:
        out["dz"] = get("dz", lambda: torch.full((H,), float("nan"), device="cuda"))
        fa.check(fa.lib.fa_bwd_dsink(p(LSE), p(delta), p(dsink), p(out["dz"]), B, H, Sq, None, None), "fa_bwd_dsink")
    if stages is None:
        torch.cuda.synchronize()
    return out


def check_training(tag, gt, got, dO, dtype, mode, rel, raw_bf16_dkv, bounds, far_from=None, matters=None, few=None,
                   rel_floor=None, show_bounds=False, report=None):
    """relFro per output against rel[dtype] (raw_bf16_dkv for bf16 dK / dV in mode "raw"; rel_floor: per-output bounds
    that may only raise them), then blockcheck.check_outputs under `bounds`: blocks, few-key rows, LSE rows, structural
    zeros.  far_from: the untransformed O, from which got["O"] must be at least `matters` away (relFro).  Prints one line
    of errors -- report(errs, records) prints it instead when a file's line holds more; show_bounds: a line per output
    with its bound first.  Returns the relFro errors."""
    errs = {}
    for n in ("O", "dQ", "dK", "dV"):
        if n in got:
            errs[n] = fo.rel_fro(gt[n], got[n])
            bound = raw_bf16_dkv if (mode == "raw" and dtype == BF16 and n in ("dK", "dV")) else rel[dtype]
            bound = max(bound, (rel_floor or {}).get(n, 0.0))
            if show_bounds:
                print(tag, n, "relFro %.3e (bound %.1e)" % (errs[n], bound))
            assert errs[n] <= bound, "%s %s relFro %.3e > %.1e" % (tag, n, errs[n], bound)
    recs = bc.check_outputs(tag, gt, got, dO, None, None, dtype, mode, bounds, few=few)
    if report is not None:
        report(errs, recs)
    else:
        print(tag, " ".join("%s=%.2e" % kv for kv in errs.items()),
              " ".join("%s:blk%.2e" % (r["out"], r["max"]) for r in recs))
    if far_from is not None:
        far = fo.rel_fro(far_from, got["O"])
        assert far >= matters, "%s: O is within %.3e of the untransformed attention" % (tag, far)
    return errs


def packed_case(call, truth_kw, skip, lens, dtype, D, H, Hkv, seed, amp=1.0, extra=None, scale=None, device="cuda"):
    """A causal packed batch of (S_q, S_k) `lens` through call(q, k, v[, extra], **the packed keywords) and its backward.
    Returns the outputs, the fp64 truth assembled per sequence -- truth_kw(i, S_q, S_k): attention_fp64's keywords for
    sequence i; skip(S_q, S_k): the sequences that leave zeros; dz and den summed over the others -- and (Q, K, V, dO,
    the packed keywords).  scale: None is D ** -0.5 and no softmax_scale is passed; otherwise the call gets
    softmax_scale=scale, the truth is taken at it, and the truth's O at D ** -0.5 comes back as gt["O_DEFAULT"]."""
    g = torch.Generator(device=device).manual_seed(seed)
    tq, tk = sum(a for a, _ in lens), sum(b for _, b in lens)
    Q = (torch.randn(tq, H, D, device=device, generator=g) * amp).to(dtype)
    K, V = (torch.randn(tk, Hkv, D, device=device, generator=g).to(dtype) for _ in range(2))
    dO = torch.randn(tq, H, D, device=device, generator=g).to(dtype)
    cu_q = torch.tensor([0] + [sum(a for a, _ in lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=device)
    cu_k = torch.tensor([0] + [sum(b for _, b in lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=device)
    kw = dict(is_causal=True, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=max(a for a, _ in lens),
              max_seqlen_k=max(b for _, b in lens))
    if scale is not None:
        kw["softmax_scale"] = scale
    got = autograd_run(lambda *a: call(*a, **kw), Q, K, V, dO, extra)
    gt = {n: torch.zeros(t.shape, dtype=torch.float64, device=device) for n, t in (("O", Q), ("dQ", Q), ("dK", K), ("dV", V))}
    gt.update(dz=torch.zeros(H, dtype=torch.float64, device=device), den=torch.zeros(H, dtype=torch.float64, device=device))
    if scale is not None:
        gt["O_DEFAULT"] = torch.zeros_like(gt["O"])
    for i, (a, b) in enumerate(lens):
        if skip(a, b):
            continue
        sq, sk = slice(int(cu_q[i]), int(cu_q[i + 1])), slice(int(cu_k[i]), int(cu_k[i + 1]))
        per = lambda t, s: t[s].permute(1, 0, 2)[None]
        r = ar.attention_fp64(per(Q, sq), per(K, sk), per(V, sk), per(dO, sq), D ** -0.5 if scale is None else scale,
                              ar.visible(a, b, -1, 0, device), **truth_kw(i, a, b))
        if scale is not None:
            gt["O_DEFAULT"][sq] = ar.attention_fp64(per(Q, sq), per(K, sk), per(V, sk), None, D ** -0.5,
                                                    ar.visible(a, b, -1, 0, device), **truth_kw(i, a, b))["O"][0].permute(1, 0, 2)
        for n, s in (("O", sq), ("dQ", sq), ("dK", sk), ("dV", sk)):
            gt[n][s] = r[n][0].permute(1, 0, 2)
        gt["dz"] += r["dz"]
        gt["den"] += r["den"]
    return got, gt, (Q, K, V, dO, kw)


def check_packed(got, gt, bound):
    """relFro of packed_case's O, dQ, dK, dV within `bound`, and the structural zeros: queries without a key (O = dQ = 0),
    keys without a query (dK = dV = 0)."""
    for n in ("O", "dQ", "dK", "dV"):
        err = fo.rel_fro(gt[n], got[n])
        assert err <= bound, (n, err)
        zero = (gt["O"] == 0).all(-1) if n in ("O", "dQ") else (gt["dV"] == 0).all(-1)
        assert (got[n][zero] == 0).all(), (n, "structural zeros")


# ---------------------------------------------------------------- decoding (GPU)
def splits(n):
    """Force the decode kernels' split count (0: the formula)."""
    import _mi355fa as fa
    fn = fa.lib.fa_debug_kvcache_splits
    fn.argtypes = [ctypes.c_int]
    fn.restype = None
    fn(n)


@pytest.fixture
def formula_splits():
    yield
    splits(0)


DECODE_CACHE = 700   # decode_case's cache rows


def decode_case(call, truth_kw, dtype, D, Sq, window, rel, matters, lse_bound, amp=1.0, scale=None, device="cuda", report=None):
    """B 3, H 8, H_kv 2 over a DECODE_CACHE-row cache at fill levels 0 / 300 / 650 with 2 appended keys, at forced split
    counts 0 (the formula) / 1 / 3 / 7.  call(q, k_cache, v_cache, cache_seqlens, k_new=, v_new=, window_size=, return_lse=True);
    truth_kw(Ls): attention_fp64's keywords for the key counts Ls.  Every count is accurate and repeats its own bits (it
    sets the order in which the partial sums are merged), the append lands in the cache, O is at least `matters` from
    the untransformed attention, LSE is -inf exactly on the keyless rows.  Returns (splits, O relFro, largest LSE error)
    per count.

    scale: None is D ** -0.5 and no softmax_scale is passed.  Otherwise the call gets softmax_scale=scale, the truth is
    taken at it, and the scale must matter and enter as a product (tests/test_gpu_scale_variants.py): over the sequences of
    at least quantcapcheck.MATTERS_FROM keys the fp64 truth, and then every count's O, is at least test_gpu_scale.FAR from
    the fp64 truth at D ** -0.5 on the same inputs; and 2 q at scale / 2 returns the bits of q at scale, O and LSE.
    report(splits, O relFro, LSE error, the truth's FAR figure, O's FAR figure) is called per count."""
    B, H, Hkv, Sc, Snew = 3, 8, 2, DECODE_CACHE, 2
    dflt = D ** -0.5
    kw = {}
    if scale is not None:
        kw["softmax_scale"] = scale
    else:
        scale = dflt
    g = torch.Generator(device=device).manual_seed(D + Sq)
    q = (torch.randn(B, H, Sq, D, device=device, generator=g) * amp).to(dtype)
    kc, vc = (torch.randn(B, Hkv, Sc, D, device=device, generator=g).to(dtype) for _ in range(2))
    kn, vn = (torch.randn(B, Hkv, Snew, D, device=device, generator=g).to(dtype) for _ in range(2))
    sl = torch.tensor([0, 300, 650], dtype=torch.int32, device=device)
    sync = torch.cuda.synchronize if device == "cuda" else (lambda: None)
    # the reference's cache: k_new / v_new at rows [seqlens[b], seqlens[b] + S_new)
    kr, vr = kc.clone(), vc.clone()
    for b in range(B):
        s0 = int(sl[b])
        kr[b, :, s0:s0 + Snew], vr[b, :, s0:s0 + Snew] = kn[b], vn[b]
    Ls = [int(sl[b]) + Snew for b in range(B)]
    vis = torch.stack([ar.visible(Sq, Sc, window[0], window[1], device, L=L) for L in Ls])[:, None]
    gt = ar.attention_fp64(q, kr, vr, None, scale, vis, **truth_kw(Ls))
    plain = ar.attention_fp64(q, kr, vr, None, scale, vis)["O"]
    ref_far = None
    if kw:
        from quantcapcheck import MATTERS_FROM
        from test_gpu_scale import FAR
        long = [b for b, L in enumerate(Ls) if L >= MATTERS_FROM]
        at_default = ar.attention_fp64(q, kr, vr, None, dflt, vis, **truth_kw(Ls))["O"][long]
        ref_far = fo.rel_fro(at_default, gt["O"][long])
        assert ref_far >= FAR, "a weak input: the fp64 truth at scale %g is within %.3e of the one at D ** -0.5" % (scale, ref_far)
    fin = torch.isfinite(gt["LSE"])
    a, u = lse_bound
    res = []
    for n in (0, 1, 3, 7):
        splits(n)
        runs = []
        for _ in range(2):
            k_, v_ = kc.clone(), vc.clone()
            runs.append(call(q, k_, v_, sl, k_new=kn, v_new=vn, window_size=window, return_lse=True, **kw))
            sync()
            assert torch.equal(k_, kr) and torch.equal(v_, vr)
        (o, lse), (o2, lse2) = runs
        assert bc.same_bits(o, o2) and bc.same_bits(lse, lse2), n
        err = fo.rel_fro(gt["O"], o)
        assert err <= rel, (n, err)
        assert fo.rel_fro(plain, o) >= matters, n
        assert torch.equal(torch.isneginf(lse), ~fin), n
        lerr = (lse.double() - gt["LSE"]).abs()[fin]
        assert (lerr <= a + u * gt["SABS"][fin]).all(), n
        assert (o[(gt["O"] == 0).all(-1)] == 0).all(), n
        far = None
        if kw:
            far = fo.rel_fro(at_default, o[long])
            assert far >= FAR, "%d splits: O is within %.3e of the attention at D ** -0.5" % (n, far)
            o3, lse3 = call(q * 2, kc.clone(), vc.clone(), sl, k_new=kn, v_new=vn, window_size=window, return_lse=True,
                            softmax_scale=scale / 2)
            sync()
            assert bc.same_bits(o, o3) and bc.same_bits(lse, lse3), "%d splits: 2 q at scale / 2 changes bits" % n
        if report is not None:
            report(n, err, lerr.max().item(), ref_far, far)
        res.append((n, err, lerr.max().item()))
    return res


def graph_replay(call, seqlens, steps, extra=None):
    """One decode step call(extra) -> O captured in a graph, then replayed once per (cache_seqlens, extra's new values or
    None) of `steps`, both written in place: each replay has the bits of an eager call with the new values (the host
    never reads either)."""
    call(extra)   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(extra)
    for lens, value in steps:
        seqlens.copy_(torch.tensor(lens, dtype=torch.int32))
        if value is not None:
            extra.copy_(value)
        graph.replay()
        torch.cuda.synchronize()
        eager = call(None if extra is None else extra.clone())
        torch.cuda.synchronize()
        assert bc.same_bits(out, eager), lens


# ---------------------------------------------------------------- the C boundary and the reference (CPU)
def header_functions(path):
    """(the header's text, the same without comments, the sorted names of the fa_* functions it declares)"""
    txt = open(path).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return txt, body, sorted(set(re.findall(r"\b(fa_[a-z0-9_]+)\s*\(", body)))


def aligned_ptr():
    """(the buffer to keep alive, a 16-byte aligned address inside it)"""
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def entry_calls(lib, names, p, B):
    """name -> f(scale, extra, H, H_kv, wl, opts): one otherwise well-formed call per entry point (S = 8, D = 64, bf16,
    every pointer p), `extra` being the tuple of arguments spliced in after the scale.  The name tells the argument list:
    fa_fwd_kvcache_fp8*, fa_fwd_kvcache*, fa_bwd_* or fa_fwd_*."""
    import _mi355fa as fa
    S, D, dt = 8, 64, fa.BF16

    def one(name):
        fn = getattr(lib, name)
        if name.startswith("fa_fwd_kvcache_fp8"):
            return lambda s, x, H, Hkv, wl, o: fn(p, p, p, None, None, p, None, None, 0, p, p, p, 1 << 12, B, H, Hkv, 1, S, 0,
                                                  D, dt, fa.KV_FP8_E4M3, s, *x, wl, 0, o, None)
        if name.startswith("fa_fwd_kvcache"):
            return lambda s, x, H, Hkv, wl, o: fn(p, p, p, None, None, p, p, p, p, 1 << 12, B, H, Hkv, 1, S, 0, D, dt, s, *x,
                                                  wl, 0, o, None)
        n = 8 if name.startswith("fa_bwd_") else 5
        return lambda s, x, H, Hkv, wl, o: fn(*[p] * n, B, H, Hkv, S, S, D, dt, s, *x, wl, 0, o, None)
    return {name: one(name) for name in names}


def check_spliced_signatures(table, bases, spliced_types):
    """table[name] is the base signature with spliced_types inserted after the scale, for every (name, base signature)."""
    for name, base in bases:
        a, b = table[name][1], base[1]
        i = b.index(ctypes.c_float)
        assert a == b[:i + 1] + list(spliced_types) + b[i + 1:], name


def check_common_refusals(calls, good_extra):
    """What every variant refuses with the code the GQA calls give, good_extra being well-formed spliced arguments: a bad
    scale (MI355FA_ERR_SHAPE), a window below -1, H_kv = 0, H % H_kv != 0, dropout (MI355FA_ERR_SHAPE).  Returns
    name -> the error texts after the H % H_kv and the dropout calls, for what a file asserts on top."""
    import _mi355fa as fa
    drop = fa.Opts.make(p_drop=0.25, seed=1)
    texts = {}
    for name, f in calls.items():
        for s in (0.0, -0.125, math.nan, math.inf):
            assert f(s, good_extra, 4, 2, -1, None) == -2, (name, s)
            assert b"scale" in fa.lib.fa_last_error()
        assert f(0.125, good_extra, 4, 2, -2, None) == fa.ERR_WINDOW, name
        assert f(0.125, good_extra, 4, 0, -1, None) == fa.ERR_GROUP, name
        assert f(0.125, good_extra, 6, 4, -1, None) == fa.ERR_GROUP, name
        group = fa.lib.fa_last_error()
        assert f(0.125, good_extra, 4, 2, -1, ctypes.byref(drop)) == -2, name
        texts[name] = dict(group=group, dropout=fa.lib.fa_last_error())
        assert b"dropout" in texts[name]["dropout"]
    return texts


def reference_agrees_with_autograd(dims, scale, window, L, truth_kw, amp=1.0):
    """attn_ref.attention_fp64's closed-form gradients (dz with sinks) against autograd through attn_ref.attention_eager,
    in fp64 on the CPU, for dims = (B, H, H_kv, S_q, S_k, D) seeded by their sum and L the bottom-right key count (None:
    training).  Returns Q, K, V, dO, the mask and the truth."""
    B, H, Hkv, Sq, Sk, D = dims
    g = torch.Generator().manual_seed(sum(dims))
    Q = torch.randn(B, H, Sq, D, generator=g, dtype=torch.float64) * amp
    K, V = (torch.randn(B, Hkv, Sk, D, generator=g, dtype=torch.float64) for _ in range(2))
    dO = torch.randn(B, H, Sq, D, generator=g, dtype=torch.float64)
    vis = ar.visible(Sq, Sk, window[0], window[1], "cpu", L=L)
    gt = ar.attention_fp64(Q, K, V, dO, scale, vis, **truth_kw)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    kw, grads = dict(truth_kw), [("dQ", q), ("dK", k), ("dV", v)]
    if "sinks" in kw:
        kw["sinks"] = kw["sinks"].clone().requires_grad_(True)
        grads.append(("dz", kw["sinks"]))
    o = ar.attention_eager(q, k, v, scale, vis, **kw)
    o.backward(dO)
    for n, t in [("O", o.detach())] + [(n, x.grad) for n, x in grads]:
        assert torch.allclose(gt[n], t, rtol=1e-10, atol=1e-10), (n, (gt[n] - t).abs().max().item())
    return Q, K, V, dO, vis, gt
