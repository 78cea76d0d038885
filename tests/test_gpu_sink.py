"""GPU tests of the attention sinks (include/mi355fa_sink.h): O, LSE, dQ, dK, dV and dz of the sink forward, the GQA
backward kernels run on its O / LSE and the sink-gradient kernel, and O / LSE of the sink decode kernels over 16-bit and
e4m3 caches, against the fp64 reference of tests/attn_ref.py computed on the device.

Every training case is checked as in test_gpu_alibi.py: relFro per output against the suite's per-feature bounds (1e-3
fp16, 8e-3 bf16; bf16 dK / dV without the q_scaled workspace: RAW_BF16_DKV), block by block with
blockcheck.check_outputs (bounds below), LSE row by row, exact zeros where fp64 has them, and dz per head relative to
den_h = sum |p0 delta| (the terms of dz cancel).  Every case also requires the kernel's O to be far from the sink-less
attention of the same inputs (relFro >= BIAS_MATTERS) after requiring the same of the fp64 reference at REF_MATTERS, so a
kernel that ignores the sinks fails.  Sinks of -inf must give the bits of flash_attention_gqa."""
import pytest
import torch

import attn_ref as sr
import blockcheck as bc
import fa_oracle as fo
import variantcheck as vck
from variantcheck import formula_splits   # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
REL = {F16: 1e-3, BF16: 8e-3}
RAW_BF16_DKV = 3e-2
BIAS_MATTERS = 0.05
REF_MATTERS = 0.1
# per-block bounds (blockcheck.check_outputs): about 1.5x the largest block error measured on an MI355X over every case in
# this file (fp16 O 3.03e-4, dQ 3.25e-4, dK 3.16e-4, dV 3.11e-4; bf16 O 3.54e-3, dQ 5.44e-3, dK 4.23e-3, dV 3.50e-3; bf16
# dK / dV without the workspace 4.18e-3).  They sit at test_gpu_alibi.py's values except bf16 dQ: 5.44e-3 is the
# softmax_scale = 0.2 case at D = 64 (scores 1.6x the default scale's, a sharper softmax, more cancellation in dS); at the
# default scale the largest is 4.29e-3 against ALiBi's 4.11e-3.
BLOCK_BOUND = {
    (F16, "O"): 4.5e-4, (F16, "dQ"): 4.9e-4, (F16, "dK"): 4.7e-4, (F16, "dV"): 4.7e-4,
    (BF16, "O"): 5.3e-3, (BF16, "dQ"): 8.2e-3, (BF16, "dK"): 6.3e-3, (BF16, "dV"): 5.3e-3,
}
# LSE per row: |LSE - fp64| <= a + u * max |logit| of the row (the visible scores and the sink): the suite's LSE_BOUND
# (largest row error measured: bf16 3.30e-3, fp16 and every decode case below 1.1e-6)
BOUNDS = dict(BLOCK_BOUND=BLOCK_BOUND, BLOCK_BOUND_RAW_BF16_DKV=6.3e-3, FEW_BOUND={F16: 1e-2, BF16: 1e-1}, RATIO=4.0,
              FLOOR=1e-5, LSE_BOUND={F16: (2e-4, 2.0 ** -16), BF16: (1.5e-2, 2.0 ** -8)}, DELTA_BOUND=1e-6)
# dz per head: |dz_h - dz_h(fp64)| / den_h, about 1.5x the largest value measured on an MI355X over every case in this file
# (fp16 8.83e-5, bf16 1.23e-3).  A constant LSE error e moves dz by at most e * den_h; bf16 stays below its LSE error
# (3.3e-3 here), fp16 is above its own (1e-6) and the reason is not the sink kernel: delta = dO . O is formed from the O
# the forward STORED, rounded to 16 bits (the delta every backward kernel of the library uses), and the fp64 reference
# uses the unrounded O.  A row's delta is a cancelling sum of D products, so O's rounding (2^-11 relative in fp16) moves
# it by a few 1e-4 of |delta|, with random sign over the rows of a head: 1e-5 to 1e-4 of den_h at these sizes.  Against
# the same fp64 sum over dO . O of the stored O ("dz-on-stored-O" in the printed line) the kernel is within 5.4e-8 in
# fp16 and 2.5e-4 in bf16 (there the rest is the bf16 forward's LSE error).
DZ_BOUND = {F16: 1.3e-4, BF16: 1.9e-3}


def _sinks(H, lo=0.0, hi=8.0):
    return torch.linspace(lo, hi, H, device="cuda", dtype=torch.float32)


def _autograd(Q, K, V, dO, sinks, window, scale=None, fn=None):
    if fn is None:
        fn = lambda q, k, v, z: vck.M().flash_attention_sink(q, k, v, z, window_size=window, softmax_scale=scale)
    return vck.autograd_run(fn, Q, K, V, dO, sinks.detach().clone().requires_grad_(True))


def _raw(Q, K, V, dO, sinks, window, scale, workspace):
    """fa_fwd_sink, the GQA backward pair on its O / LSE, fa_bwd_dsink."""
    return vck.raw_run(("fa_fwd_sink", "fa_bwd_dq_gqa", "fa_bwd_dkv_gqa"), (sinks.data_ptr(),), Q, K, V, dO, window, scale,
                       workspace, dsink=sinks)


def _dz_err(gt, dz):
    return ((dz.double() - gt["dz"]).abs() / gt["den"].clamp_min(1e-300)).max().item()


def _check(tag, gt, got, dO, dtype, mode, unb=None, few=None):
    """vck.check_training under this file's bounds, and dz; the sink must matter, in the fp64 reference first.  Returns
    the errors."""
    if unb is not None:
        ref_far = fo.rel_fro(unb, gt["O"])
        assert ref_far >= REF_MATTERS, "%s: a weak input, the fp64 sink moves O by %.3e only" % (tag, ref_far)
    dz, own = {}, ""
    if "dz" in got:
        dz["dz"] = _dz_err(gt, got["dz"])
        # the same sum in fp64 over the delta the kernels see, dO . O with the 16-bit O they stored: what is left of the
        # error is the sink-gradient kernel's own (p0 from the fp32 LSE, the fp32 sum)
        d16 = (dO.double() * got["O"].double()).sum(-1)
        own = "dz-on-stored-O=%.2e" % ((got["dz"].double() + (gt["P0"] * d16).sum((0, 2))).abs() / gt["den"]).max().item()

    def report(errs, recs):
        print(tag, own, " ".join("%s=%.2e" % kv for kv in {**errs, **dz}.items()),
              " ".join("%s:blk%.2e" % (r["out"], r["max"]) for r in recs),
              "|dz|/den min %.3f" % (gt["dz"].abs() / gt["den"].clamp_min(1e-300)).min().item())
    errs = vck.check_training(tag, gt, got, dO, dtype, mode, REL, RAW_BF16_DKV, BOUNDS, unb, BIAS_MATTERS, few, report=report)
    if dz:
        assert dz["dz"] <= DZ_BOUND[dtype], "%s dz error %.3e > %.1e" % (tag, dz["dz"], DZ_BOUND[dtype])
    return {**errs, **dz}


# dtype, D, H, H_kv, S_q, S_k, window, strided
CASES = [
    ("fp16-d64-mha-full", F16, 64, 4, 4, 256, 256, (-1, -1), False),
    ("bf16-d64-gqa8-causal", BF16, 64, 8, 1, 256, 256, (-1, 0), False),
    ("bf16-d64-gqa4-causal-ragged", BF16, 64, 8, 2, 200, 333, (-1, 0), False),
    ("fp16-d128-mqa-w127", F16, 128, 4, 1, 384, 384, (127, 0), False),
    ("bf16-d64-gqa8-w127", BF16, 64, 16, 2, 300, 300, (127, 0), False),
    ("bf16-d128-gqa4-w64x64", BF16, 128, 8, 2, 256, 256, (64, 64), False),
    ("fp16-d128-gqa4-causal-strided", F16, 128, 8, 2, 300, 300, (-1, 0), True),
    ("bf16-d64-mqa-full-sq<sk", BF16, 64, 4, 1, 128, 200, (-1, -1), False),
    ("fp16-d64-gqa4-w127-sq>sk", F16, 64, 4, 1, 333, 200, (127, 0), False),      # rows 328.. see no key
    ("bf16-d128-gqa8-w40x10-sq>sk", BF16, 128, 8, 1, 400, 300, (40, 10), False),  # rows 341.. see no key
    ("bf16-d128-mha-full", BF16, 128, 4, 4, 256, 256, (-1, -1), False),
    ("fp16-d64-gqa8-causal", F16, 64, 8, 1, 512, 512, (-1, 0), False),
    # head groups that are no power of two: g = 3, and g = 7 as multi-query -- seven distinct sinks through the dK / dV loop
    # over a group's heads and fa_bwd_dsink at a head count that is no power of two (dz per head: DZ_BOUND)
    ("fp16-d64-g3-w64x40-ragged", F16, 64, 6, 2, 301, 211, (64, 40), False),                # rows 275.. see no key
    ("bf16-d128-g7-causal-ragged", BF16, 128, 7, 1, 233, 333, (-1, 0), False),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sink_matches_fp64(case):
    tag, dtype, D, H, Hkv, Sq, Sk, window, strided = case
    scale = D ** -0.5
    B = 2
    Q, K, V, dO = vck.inputs(B, H, Hkv, Sq, Sk, D, dtype, seed=Sq + Sk + D)
    sinks = _sinks(H)
    vis = sr.visible(Sq, Sk, window[0], window[1], "cuda")
    gt = sr.attention_fp64(Q, K, V, dO, scale, vis, sinks=sinks)
    unb = sr.attention_fp64(Q, K, V, None, scale, vis)["O"]
    keyless = ~vis.any(-1)
    if Sq > Sk:
        assert keyless.any() and (gt["LSE"][:, :, keyless] == sinks.double()[None, :, None]).all()
    if strided:   # [B, S, H, D] buffers seen as [B, H, S, D]: read in place, the same bits as contiguous tensors
        Qs, Ks, Vs = (x.transpose(1, 2).contiguous().transpose(1, 2) for x in (Q, K, V))
        got = _autograd(Qs, Ks, Vs, dO, sinks, window)
        ref = _autograd(Q, K, V, dO, sinks, window)
        for n in got:
            assert bc.same_bits(got[n], ref[n]), (tag, n)
    few = bc.few_rows(vis)
    got = _autograd(Q, K, V, dO, sinks, window)
    _check(tag + " autograd", gt, got, dO, dtype, "ws", unb, few)
    again = _autograd(Q, K, V, dO, sinks, window)
    assert bc.same_bits(got["dz"], again["dz"]), (tag, "dz is not the same bits on a repeated call")
    raw = _raw(Q, K, V, dO, sinks, window, scale, workspace=False)
    _check(tag + " raw", gt, raw, dO, dtype, "raw", unb, few)
    assert bc.same_bits(raw["O"], got["O"]) and bc.same_bits(raw["dQ"], got["dQ"])
    # a keyless row: O = 0 and LSE = z exactly (the fp16 path keeps z / scale; the bf16 path z * log2e)
    if keyless.any():
        assert (raw["O"][:, :, keyless] == 0).all() and (raw["dQ"][:, :, keyless] == 0).all()
        assert (raw["LSE"][:, :, keyless].double() - sinks.double()[None, :, None]).abs().max() <= 1e-5
    if dtype == BF16:
        ws = _raw(Q, K, V, dO, sinks, window, scale, workspace=True)
        _check(tag + " ws", gt, ws, dO, dtype, "ws", unb, few)
        assert bc.same_bits(ws["O"], raw["O"]) and bc.same_bits(ws["dz"], raw["dz"])   # the workspace: dK / dV only
        for n in ("dQ", "dK", "dV", "dz"):
            assert bc.same_bits(ws[n], got[n]), (tag, n)    # autograd takes the workspace path


def test_python_twin_and_softmax_scale():
    """FlashAttentionSinkFunction launches what flash_attention_sink launches; a non-default scale is honoured (the sink
    is not scaled)."""
    M = vck.M()
    dtype, D, H, Hkv, S = BF16, 64, 8, 2, 200
    Q, K, V, dO = vck.inputs(2, H, Hkv, S, S, D, dtype, seed=11)
    sinks = _sinks(H)
    vis = sr.visible(S, S, -1, 0, "cuda")
    gt = sr.attention_fp64(Q, K, V, dO, 0.2, vis, sinks=sinks)
    a = _autograd(Q, K, V, dO, sinks, (-1, 0), scale=0.2)
    _check("scale0.2", gt, a, dO, dtype, "ws", sr.attention_fp64(Q, K, V, None, 0.2, vis)["O"])
    b = _autograd(Q, K, V, dO, sinks, None, fn=lambda q, k, v, z: M.FlashAttentionSinkFunction.apply(q, k, v, z, -1, 0, 0.2))
    for n in a:
        assert bc.same_bits(a[n], b[n]), n


@pytest.mark.parametrize("dtype,D", [(F16, 64), (BF16, 64), (F16, 128), (BF16, 128)])
def test_minus_inf_sinks_give_the_gqa_bits(dtype, D):
    """sinks = -inf reproduce flash_attention_gqa bit for bit: O, LSE, dQ, dK and dV; dz = 0.  S_q > S_k under the window
    has keyless rows (LSE = -inf on both sides)."""
    M = vck.M()
    H = 8
    Q, K, V, dO = vck.inputs(2, H, 2, 333, 300, D, dtype, seed=D + 1)
    ninf = torch.full((H,), float("-inf"), device="cuda")
    for window in ((-1, -1), (-1, 0), (100, 20), (20, 5)):
        a = _autograd(Q, K, V, dO, ninf, window)
        q, k, v = (x.detach().clone().requires_grad_(True) for x in (Q, K, V))
        o = M.flash_attention_gqa(q, k, v, window_size=window)
        o.backward(dO)
        torch.cuda.synchronize()
        for n, t in (("O", o.detach()), ("dQ", q.grad), ("dK", k.grad), ("dV", v.grad)):
            assert bc.same_bits(a[n], t), (dtype, D, window, n)
        assert (a["dz"] == 0).all(), (dtype, D, window, a["dz"])
        wl, wr = window
        la = M.flash_attention_sink_forward(Q, K, V, ninf, wl, wr)[1]
        lg = M.flash_attention_gqa_forward(Q, K, V, wl, wr)[1]
        torch.cuda.synchronize()
        assert bc.same_bits(la, lg), (dtype, D, window, "LSE")
        if window == (20, 5):
            assert torch.isneginf(la[:, :, 330:]).all()


def test_packed_batch_with_an_empty_sequence():
    M = vck.M()
    dtype, D, H, Hkv = BF16, 64, 4, 2
    lens = [(130, 70), (0, 50), (64, 0), (257, 300), (5, 5)]
    sinks = _sinks(H)
    z = sinks.clone().requires_grad_(True)
    got, gt, (Q, K, V, dO, kw) = vck.packed_case(M.flash_attention_sink, lambda i, a, b: dict(sinks=sinks), lambda a, b: a == 0,
                                                 lens, dtype, D, H, Hkv, seed=7, extra=z)
    again = _autograd(Q, K, V, dO, sinks, None, fn=lambda q, k, v, z: M.flash_attention_sink(q, k, v, z, **kw))
    assert bc.same_bits(got["dz"], again["dz"])
    vck.check_packed(got, gt, REL[dtype])
    e = _dz_err(gt, got["dz"])
    print("packed dz err %.2e" % e)
    assert e <= DZ_BOUND[dtype], e
    # the sequence with queries and no keys: LSE = z on its rows
    cu_q, cu_k, tq = kw["cu_seqlens_q"], kw["cu_seqlens_k"], Q.shape[0]
    lse = M.flash_attention_sink_forward(Q, K, V, sinks, -1, 0, None, cu_q, cu_k, kw["max_seqlen_q"], kw["max_seqlen_k"])[1]
    torch.cuda.synchronize()
    assert lse.shape == (H, tq)
    assert (lse[:, int(cu_q[2]):int(cu_q[3])].double() - sinks.double()[:, None]).abs().max() <= 1e-5


def test_sinks_without_grad_launch_no_dsink():
    M = vck.M()
    Q, K, V, dO = vck.inputs(1, 4, 2, 128, 128, 64, F16, seed=9)
    q = Q.clone().requires_grad_(True)
    z = _sinks(4)
    o = M.flash_attention_sink(q, K, V, z, is_causal=True)
    o.backward(dO)
    assert q.grad is not None and z.grad is None
    r = M.flash_attention_sink_backward(Q, K, V, o.detach(), dO, M.flash_attention_sink_forward(Q, K, V, z, -1, 0)[1], z, -1, 0,
                                        need_dsinks=False)
    assert r[3] is None and bc.same_bits(r[0], q.grad)
    # only the sinks require grad
    zg = z.clone().requires_grad_(True)
    M.flash_attention_sink(Q, K, V, zg, is_causal=True).backward(dO)
    r = M.flash_attention_sink_backward(Q, K, V, o.detach(), dO, M.flash_attention_sink_forward(Q, K, V, z, -1, 0)[1], z, -1, 0)
    torch.cuda.synchronize()
    assert zg.grad is not None and zg.grad.dtype == torch.float32 and zg.grad.shape == (4,) and bc.same_bits(zg.grad, r[3])


# ---- decoding -----------------------------------------------------------------------------------------------------------
def _decode_call(fp8, q, kc, vc, sl, sinks, kd, vd, **kw):
    M = vck.M()
    if fp8:
        return M.flash_attention_kvcache_fp8_sink(q, kc, vc, sl, sinks, kd, vd, return_lse=True, **kw)
    return M.flash_attention_kvcache_sink(q, kc, vc, sl, sinks, return_lse=True, **kw)


def _decode_case(fp8, dtype, D, Sq, window, lens, Sc, Snew, B, H, Hkv, sinks, splits, seed):
    """One decode shape at several split counts: the caches are padded with NaN (0x7F) past the fill level, k_new / v_new
    are appended, every call runs twice (same bits), and O / LSE are checked against fp64 on the (dequantised) cache the
    kernel left behind."""
    M = vck.M()
    scale = D ** -0.5
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, H, Sq, D, device="cuda", generator=g).to(dtype)
    kf, vf = (torch.randn(B, Hkv, Sc, D, device="cuda", generator=g) for _ in range(2))
    kn, vn = (torch.randn(B, Hkv, max(Snew, 1), D, device="cuda", generator=g).to(dtype) for _ in range(2))
    if Snew == 0:
        kn = vn = None
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    kd = vd = None
    if fp8:
        kc, kd = M.quantize_kv_fp8(kf)
        vc, vd = M.quantize_kv_fp8(vf * 1.7)
    else:
        kc, vc = kf.to(dtype), vf.to(dtype)
    for b, L in enumerate(lens):   # padding past the fill level (the appended rows overwrite their part of it)
        if fp8:
            kc.view(torch.uint8)[b, :, L:] = 0x7F
            vc.view(torch.uint8)[b, :, L:] = 0x7F
        else:
            kc[b, :, L:] = float("nan")
            vc[b, :, L:] = float("nan")
    Ls = [L + Snew for L in lens]
    vis = torch.stack([sr.visible(Sq, Sc, window[0], window[1], "cuda", L=L) for L in Ls])[:, None]
    a, u = BOUNDS["LSE_BOUND"][dtype]
    gt = None
    for n in splits:
        vck.splits(n)
        runs = []
        for _ in range(2):
            k_, v_ = kc.clone(), vc.clone()
            runs.append(_decode_call(fp8, q, k_, v_, sl, sinks, kd, vd, k_new=kn, v_new=vn, window_size=window))
            torch.cuda.synchronize()
        (o, lse), (o2, lse2) = runs
        assert bc.same_bits(o, o2) and bc.same_bits(lse, lse2), n
        if gt is None:   # the cache after the append, dequantised, the padding zeroed (it is masked)
            deq = lambda x, d: x.double() * (d.double().reshape(-1, Hkv, 1, 1) if d is not None else 1.0)
            kr, vr = torch.nan_to_num(deq(k_, kd), nan=0.0), torch.nan_to_num(deq(v_, vd), nan=0.0)
            for b, L in enumerate(Ls):
                assert not torch.isnan(k_[b, :, :L].double()).any()
                assert L == Sc or torch.isnan(k_[b, :, L:].double()).all()      # the padding is still there
            gt = sr.attention_fp64(q, kr, vr, None, scale, vis, sinks=sinks)
            unb = sr.attention_fp64(q, kr, vr, None, scale, vis)["O"]
            nokey = ~vis.expand(B, H, Sq, Sc).any(-1)
            ref_far = fo.rel_fro(unb, gt["O"])
            assert ref_far >= REF_MATTERS, ref_far
        assert torch.isfinite(o).all() and torch.isfinite(lse).all(), n
        err = fo.rel_fro(gt["O"], o)
        assert err <= REL[dtype], (n, err)
        assert fo.rel_fro(unb, o) >= BIAS_MATTERS, n
        lerr = (lse.double() - gt["LSE"]).abs()
        assert (lerr <= a + u * gt["SABS"]).all(), (n, lerr.max().item())
        assert (o[nokey] == 0).all(), n                                           # O = 0 and LSE = z without a key
        zrow = sinks.double()[None, :, None].expand(B, H, Sq)
        assert (lse.double()[nokey] - zrow[nokey]).abs().max().item() <= 1e-5 if nokey.any() else True, n
        print("decode", "fp8" if fp8 else "16b", dtype, D, Sq, window, "splits", n,
              "O relFro %.2e LSE max %.2e sink moves O %.2f" % (err, lerr.max().item(), ref_far))
    return nokey


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("dtype,D,Sq,window", [(F16, 128, 1, (-1, -1)), (BF16, 64, 4, (-1, 0)), (BF16, 128, 3, (200, 0)),
                                               (F16, 64, 4, (-1, 0))])
def test_decode_matches_fp64(fp8, dtype, D, Sq, window, formula_splits):
    nokey = _decode_case(fp8, dtype, D, Sq, window, lens=[0, 300, 650, 1], Sc=704, Snew=2, B=4, H=8, Hkv=2,
                         sinks=_sinks(8), splits=(0, 1, 3, 7), seed=D + Sq)
    # sequence 0 holds the two appended keys only: with S_q = 3 / 4 its first 1 / 2 queries sit at negative positions and
    # see no key under window_right = 0 (O = 0, LSE = z, checked in _decode_case); every other row of these cases sees one
    assert bool(nokey.any()) == (window[1] == 0 and Sq > 2), (Sq, window)


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_decode_empty_sequences_give_lse_z(fp8, dtype, formula_splits):
    """cache_seqlens 0 and no append: L_b = 0 gives O = 0 and LSE = z; S_q = 4 causal over L_b = 2 has two keyless rows."""
    nokey = _decode_case(fp8, dtype, 64, 4, (-1, 0), lens=[0, 2, 500, 77], Sc=512, Snew=0, B=4, H=8, Hkv=1,
                         sinks=_sinks(8), splits=(0, 1, 5), seed=3)
    assert nokey[0].all() and nokey[1, :, :2].all() and not nokey[2:].any()


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_decode_long_context(fp8, formula_splits):
    """gpt-oss-like heads at L >= 4096 (sinks linspace(2, 10, H): at 4096 keys a sink near 0 is one key among thousands), at
    the rule's split count and at forced counts."""
    _decode_case(fp8, BF16, 64, 1, (-1, -1), lens=[4096, 5000], Sc=5120, Snew=1, B=2, H=64, Hkv=8, sinks=_sinks(64, 2.0, 10.0),
                 splits=(0, 1, 4), seed=21)
    _decode_case(fp8, BF16, 64, 1, (127, 0), lens=[4096, 5000], Sc=5120, Snew=1, B=2, H=64, Hkv=8, sinks=_sinks(64),
                 splits=(0, 2), seed=22)


@pytest.mark.parametrize("dtype,D", [(F16, 64), (BF16, 128)])
def test_decode_without_cache_offset_agrees_with_the_training_forward(dtype, D, formula_splits):
    """S_q = L: bottom-right and top-left alignment coincide, so flash_attention_kvcache_sink and flash_attention_sink's
    forward compute the same attention on the same tensors."""
    M = vck.M()
    B, H, Hkv, S = 2, 8, 2, 200
    Q, K, V, _ = vck.inputs(B, H, Hkv, S, S, D, dtype, seed=5)
    sinks = _sinks(H)
    sl = torch.full((B,), S, dtype=torch.int32, device="cuda")
    for window in ((-1, 0), (50, 0), (-1, -1)):
        o1, l1 = M.flash_attention_sink_forward(Q, K, V, sinks, window[0], window[1])
        o2, l2 = M.flash_attention_kvcache_sink(Q, K, V, sl, sinks, window_size=window, return_lse=True)
        torch.cuda.synchronize()
        gt = sr.attention_fp64(Q, K, V, None, D ** -0.5, sr.visible(S, S, window[0], window[1], "cuda"), sinks=sinks)
        for o in (o1, o2):
            assert fo.rel_fro(gt["O"], o) <= REL[dtype]
        assert fo.rel_fro(o1.double(), o2) <= 2 * REL[dtype], window
        a, u = BOUNDS["LSE_BOUND"][dtype]
        assert ((l1.double() - l2.double()).abs() <= 2 * (a + u * gt["SABS"])).all(), window


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_decode_graph_replay(fp8):
    """One captured decode step, replayed after cache_seqlens and the sinks change in place: each replay matches an eager
    call with the new values (the host never reads either)."""
    M = vck.M()
    B, H, Hkv, Sq, Sc, D = 2, 8, 2, 1, 1024, 128
    g = torch.Generator(device="cuda").manual_seed(5)
    q = torch.randn(B, H, Sq, D, device="cuda", generator=g).to(BF16)
    kc, vc = (torch.randn(B, Hkv, Sc, D, device="cuda", generator=g) for _ in range(2))
    kd = vd = None
    if fp8:
        kc, kd = M.quantize_kv_fp8(kc)
        vc, vd = M.quantize_kv_fp8(vc)
    else:
        kc, vc = kc.to(BF16), vc.to(BF16)
    sl = torch.tensor([700, 1000], dtype=torch.int32, device="cuda")
    call = lambda z: _decode_call(fp8, q, kc, vc, sl, z, kd, vd)[0]
    steps = [(lens, _sinks(H) + shift) for lens, shift in (([700, 1000], 0.0), ([300, 1024], 2.0), ([0, 512], -3.0))]
    vck.graph_replay(call, sl, steps, extra=_sinks(H))
