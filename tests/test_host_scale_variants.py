"""CPU tests of tests/test_gpu_scale_variants.py and of the `scale` keyword of tests/variantcheck.py (no GPU, no kernel).

  * the coverage pin: every public function of the package that takes softmax_scale is named by a row of the GPU module's
    TABLE (the plain flash_attention_kvcache: by tests/test_gpu_scale.py), each function family is reached at both of
    test_gpu_scale.SCALES, and the paged and packed calls get each transform keyword in some row.  A new entry point
    without a scale case fails here.
  * the reference-only half of the FAR condition, for every row, with the row's recipe on the CPU (far_on): the fp64
    truth at the scale is at least FAR from the fp64 truth at D ** -0.5.
  * the helper edit: decode_case and packed_case with scale=None build the inputs and the truth they built before (a
    copy of the old arithmetic below), pass no softmax_scale, and a call that returns that truth passes.
  * sensitivity: held() and check_seqs -- and the training files' _check -- refuse four outputs that each carry one wrong
    use of the scale (slope * scale, a sink scaled by the scale, a cap coefficient without k_descale, LSE from
    m * D ** -0.5), and accept the truth rounded to the dtype."""
import inspect
import re

import pytest
import torch

import attn_ref as ar
import blockcheck as bc
import test_gpu_alibi as tal
import test_gpu_scale_variants as sv
import test_gpu_sink as tsk
import test_gpu_softcap as tsc
import variantcheck as vck
from test_gpu_scale import FAR, SCALES

F16, BF16 = torch.float16, torch.bfloat16
MODULES = ("My_FlashAttention_optimized", "paged_kvcache", "ragged_kvcache", "fp4_kvcache", "fp4_ragged_kvcache",
           "fp8_token_kvcache", "quant_softcap_kvcache")


def scaled_functions():
    """the names of the public functions that take softmax_scale, per module"""
    out = {}
    for name in MODULES:
        mod = __import__(name)
        out[name] = sorted(n for n, f in vars(mod).items() if inspect.isfunction(f) and not n.startswith("_")
                           and f.__module__ == name and "softmax_scale" in inspect.signature(f).parameters)
    return out


def family(fn):
    """a function's family: its name without the layer (_forward / _backward) and geometry (_paged / _ragged) suffixes"""
    return re.sub(r"_(forward|backward|paged|ragged)$", "", fn)


# ---------------------------------------------------------------- the coverage pin
def test_every_function_that_takes_a_scale_has_a_case_at_both_scales():
    fns = scaled_functions()
    assert all(fns[m] for m in MODULES), fns                     # the signature walk finds something in every module
    assert len(fns["My_FlashAttention_optimized"]) >= 15 and len(fns["quant_softcap_kvcache"]) == 3
    plain = open(__import__("test_gpu_scale").__file__).read()
    named = {}
    for r in sv.TABLE:
        for f in r["fns"]:
            named.setdefault(f, set()).add(r["scale"])
    reached = {}
    for mod, names in fns.items():
        for f in names:
            if f not in named:
                assert f == "flash_attention_kvcache" and "flash_attention_kvcache(" in plain and "softmax_scale=scale" in plain, \
                    "%s.%s takes softmax_scale and no row of test_gpu_scale_variants.TABLE names it" % (mod, f)
                reached.setdefault(family(f), set()).update(SCALES)
            reached.setdefault(family(f), set()).update(named.get(f, ()))
    for fam, scales in reached.items():
        assert scales >= set(SCALES), "%s is reached at %s only" % (fam, sorted(scales))
    every = {f for names in fns.values() for f in names}
    assert set(named) <= every, sorted(set(named) - every)       # and the table names nothing that does not exist
    for f in ("flash_attention_kvcache_paged", "flash_attention_kvcache_ragged"):
        mods = {m for r in sv.TABLE if f in r["fns"] for m in r.get("mods", ())}
        assert mods >= {"softcap", "alibi_slopes", "sinks", "k_descale", "v_descale"}, (f, mods)
        assert any(f in r["fns"] and r.get("mods") == () for r in sv.TABLE), (f, "no row without a transform")


def test_a_new_entry_point_without_a_case_fails_the_pin(monkeypatch):
    import paged_kvcache as P

    def flash_attention_kvcache_new(q, softmax_scale=None):
        return q
    flash_attention_kvcache_new.__module__ = "paged_kvcache"
    monkeypatch.setattr(P, "flash_attention_kvcache_new", flash_attention_kvcache_new, raising=False)
    with pytest.raises(AssertionError, match="flash_attention_kvcache_new"):
        test_every_function_that_takes_a_scale_has_a_case_at_both_scales()


def test_table_rows_are_distinct_and_use_the_shared_scales():
    ids = [r["id"] for r in sv.TABLE]
    assert len(set(ids)) == len(ids)
    assert {r["scale"] for r in sv.TABLE} == set(SCALES)
    assert {r["section"] for r in sv.TABLE} == set("abcdefg")
    for geometry in ("paged", "packed"):                          # d: both scales on both geometries
        assert {r["scale"] for r in sv.TABLE if r["section"] == "d" and r["id"].startswith(geometry)} == set(SCALES)


# ---------------------------------------------------------------- the FAR condition, reference only
@pytest.mark.parametrize("r", sv.TABLE, ids=[r["id"] for r in sv.TABLE])
def test_the_scale_matters_in_the_reference(r):
    far = sv.far_on(r, "cpu")
    assert far >= FAR, "%s: the fp64 truth at scale %g is within %.3e of the one at D ** -0.5" % (r["id"], r["scale"], far)


# ---------------------------------------------------------------- the helper edit
def _old_decode_inputs(dtype, D, Sq, window, amp, truth_kw):
    """decode_case's inputs and truth as it built them before it took a scale (a copy), on the CPU"""
    B, H, Hkv, Sc, Snew = 3, 8, 2, vck.DECODE_CACHE, 2
    scale = D ** -0.5
    g = torch.Generator(device="cpu").manual_seed(D + Sq)
    q = (torch.randn(B, H, Sq, D, device="cpu", generator=g) * amp).to(dtype)
    kc, vc = (torch.randn(B, Hkv, Sc, D, device="cpu", generator=g).to(dtype) for _ in range(2))
    kn, vn = (torch.randn(B, Hkv, Snew, D, device="cpu", generator=g).to(dtype) for _ in range(2))
    sl = torch.tensor([0, 300, 650], dtype=torch.int32)
    kr, vr = kc.clone(), vc.clone()
    for b in range(B):
        s0 = int(sl[b])
        kr[b, :, s0:s0 + Snew], vr[b, :, s0:s0 + Snew] = kn[b], vn[b]
    Ls = [int(sl[b]) + Snew for b in range(B)]
    vis = torch.stack([ar.visible(Sq, Sc, window[0], window[1], "cpu", L=L) for L in Ls])[:, None]
    gt = ar.attention_fp64(q, kr, vr, None, scale, vis, **truth_kw(Ls))
    return q, kc, vc, kn, vn, sl, kr, vr, gt


@pytest.mark.parametrize("dtype,D,Sq,window", [(F16, 128, 1, (-1, -1)), (BF16, 64, 4, (200, 0))])
def test_decode_case_without_a_scale_builds_what_it_built_before(dtype, D, Sq, window):
    sinks = torch.linspace(0.0, 8.0, 8)
    truth_kw = lambda Ls: dict(sinks=sinks)
    q0, kc0, vc0, kn0, vn0, sl0, kr, vr, gt = _old_decode_inputs(dtype, D, Sq, window, 1.5, truth_kw)
    seen = []

    def call(q, k_, v_, sl, k_new, v_new, window_size, return_lse, **kw):
        assert not kw, "no softmax_scale without a scale: %s" % sorted(kw)
        for a, b in ((q, q0), (k_, kc0), (v_, vc0), (k_new, kn0), (v_new, vn0), (sl, sl0)):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert window_size == window and return_lse
        k_.copy_(kr)
        v_.copy_(vr)
        seen.append(1)
        return gt["O"].float(), gt["LSE"].float()
    res = vck.decode_case(call, truth_kw, dtype, D, Sq, window, 1e-6, 0.05, (1e-5, 0.0), amp=1.5, device="cpu")
    assert len(seen) == 8 and [n for n, _, _ in res] == [0, 1, 3, 7] and max(e for _, e, _ in res) <= 1e-6


def test_decode_case_with_a_scale_passes_it_on_and_asserts_the_conditions():
    dtype, D, Sq, window, scale = F16, 64, 2, (-1, 0), 0.02
    amp = D ** -0.5 / scale
    truth_kw = lambda Ls: dict(sinks=torch.linspace(0.0, 8.0, 8))
    _, _, _, _, _, _, kr, vr, _ = _old_decode_inputs(dtype, D, Sq, window, amp, truth_kw)
    Ls = [2, 302, 652]
    vis = torch.stack([ar.visible(Sq, vck.DECODE_CACHE, -1, 0, "cpu", L=L) for L in Ls])[:, None]

    def stub(wrong):
        def call(q, k_, v_, sl, k_new, v_new, window_size, return_lse, softmax_scale):
            k_.copy_(kr)
            v_.copy_(vr)
            s = D ** -0.5 if wrong == "ignored" else softmax_scale
            r = ar.attention_fp64(q, kr, vr, None, s, vis, **truth_kw(Ls))
            lse = r["LSE"] + (1e-3 if wrong == "inexact" and softmax_scale != scale else 0.0)
            return r["O"].to(dtype), lse.float()
        return call
    args = (truth_kw, dtype, D, Sq, window, tsk.REL[dtype], tsk.BIAS_MATTERS, tsk.BOUNDS["LSE_BOUND"][dtype])
    figures = []
    vck.decode_case(stub(None), *args, amp=amp, scale=scale, device="cpu", report=lambda *a: figures.append(a))
    assert len(figures) == 4 and all(f[3] >= FAR and f[4] >= FAR for f in figures)
    for wrong in ("ignored", "inexact"):
        with pytest.raises(AssertionError):
            vck.decode_case(stub(wrong), *args, amp=amp, scale=scale, device="cpu")
    with pytest.raises(AssertionError, match="weak input"):         # unit-variance q at 1/sqrt(D) passed as "a scale"
        vck.decode_case(stub(None), *args, amp=1.0, scale=D ** -0.5 * 1.01, device="cpu")


def test_packed_case_without_a_scale_builds_what_it_built_before():
    dtype, D, H, Hkv, seed, amp = BF16, 64, 4, 2, 7, 1.25
    lens = [(130, 70), (0, 50), (64, 0), (257, 300), (5, 5)]
    sinks = torch.linspace(0.0, 8.0, H)
    # the old arithmetic (a copy), on the CPU
    g = torch.Generator(device="cpu").manual_seed(seed)
    tq, tk_ = sum(a for a, _ in lens), sum(b for _, b in lens)
    Q = (torch.randn(tq, H, D, generator=g) * amp).to(dtype)
    K, V = (torch.randn(tk_, Hkv, D, generator=g).to(dtype) for _ in range(2))
    dO = torch.randn(tq, H, D, generator=g).to(dtype)
    cu_q = [0] + [sum(a for a, _ in lens[:i + 1]) for i in range(len(lens))]
    cu_k = [0] + [sum(b for _, b in lens[:i + 1]) for i in range(len(lens))]
    old = {n: torch.zeros(t.shape, dtype=torch.float64) for n, t in (("O", Q), ("dQ", Q), ("dK", K), ("dV", V))}
    per = lambda t, s: t[s].permute(1, 0, 2)[None]
    for i, (a, b) in enumerate(lens):
        if a == 0:
            continue
        sq, sk = slice(cu_q[i], cu_q[i + 1]), slice(cu_k[i], cu_k[i + 1])
        r = ar.attention_fp64(per(Q, sq), per(K, sk), per(V, sk), per(dO, sq), D ** -0.5, ar.visible(a, b, -1, 0, "cpu"), sinks=sinks)
        for n, s in (("O", sq), ("dQ", sq), ("dK", sk), ("dV", sk)):
            old[n][s] = r[n][0].permute(1, 0, 2)

    def call(q, k, v, z, **kw):
        assert "softmax_scale" not in kw and kw["is_causal"] and kw["max_seqlen_q"] == 257 and kw["max_seqlen_k"] == 300
        assert kw["cu_seqlens_q"].tolist() == cu_q and kw["cu_seqlens_k"].tolist() == cu_k
        for a, b in ((q, Q), (k, K), (v, V)):
            assert a.dtype == b.dtype and torch.equal(a, b)
        out = []
        for i, (a, b) in enumerate(lens):
            sq, sk = slice(cu_q[i], cu_q[i + 1]), slice(cu_k[i], cu_k[i + 1])
            if a:
                o = ar.attention_eager(per(q, sq).double(), per(k, sk).double(), per(v, sk).double(), D ** -0.5,
                                       ar.visible(a, b, -1, 0, "cpu"), sinks=z.double())
                out.append(o[0].permute(1, 0, 2))
        return torch.cat(out).to(dtype)
    got, gt, (q1, k1, v1, do1, kw) = vck.packed_case(call, lambda i, a, b: dict(sinks=sinks), lambda a, b: a == 0, lens, dtype, D, H, Hkv,
                                                     seed=seed, amp=amp, extra=sinks.clone().requires_grad_(True), device="cpu")
    assert torch.equal(do1, dO) and "O_DEFAULT" not in gt and "softmax_scale" not in kw
    for n in ("O", "dQ", "dK", "dV"):
        assert torch.equal(gt[n], old[n]), n
    vck.check_packed(got, gt, tsk.REL[dtype])
    # and with a scale: passed on, used in the truth, the truth at D ** -0.5 beside it
    seen = {}

    def scaled(q, k, v, **kw):
        seen.update(kw)
        return q * 1.0
    _, gt2, _ = vck.packed_case(scaled, lambda i, a, b: dict(sinks=sinks), lambda a, b: a == 0, lens, dtype, D, H, Hkv, seed=seed,
                                amp=amp, extra=None, scale=0.02, device="cpu")
    assert seen["softmax_scale"] == 0.02 and torch.equal(gt2["O_DEFAULT"], old["O"]) and not torch.equal(gt2["O"], old["O"])


# ---------------------------------------------------------------- sensitivity
def _decode_problem(dtype, scale, D=64, Sq=2, fmt=None, seed=3):
    """q per sequence and an fp64 cache (fmt "e4m3": bytes and per-(B, H_kv) descales of about 0.01 beside it), on the CPU"""
    g = torch.Generator().manual_seed(seed)
    B, H, Hkv = 3, 8, 2
    amp = tsc._amp(30.0, scale, D) if fmt else D ** -0.5 / scale
    qs = [(torch.randn(1, H, Sq, D, generator=g) * amp).to(dtype) for _ in range(B)]
    k, v = (torch.randn(B, Hkv, sv.SC, D, generator=g) for _ in range(2))
    if fmt is None:
        return qs, k.to(dtype).double(), v.to(dtype).double(), None, None
    k8, kd = vck.M().quantize_kv_fp8(k)
    return qs, k8.double() * kd.double()[:, :, None, None], v.to(dtype).double(), k8.double(), kd


WRONG = ["slope * scale", "sink * scale", "cap coefficient without kd", "LSE from m * D ** -0.5"]


# (at scale 1.0 a slope or a sink times the scale is the slope or the sink: those two are errors at 0.02 only)
WRONG_AT = [(w, s) for w in [None] + WRONG for s in SCALES if not (w in WRONG[:2] and s == 1.0)]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("wrong,scale", WRONG_AT)
def test_held_refuses_each_wrong_use_of_the_scale(wrong, scale, dtype):
    """held() with check_seqs under the variant's bounds on the CPU: the rounded fp64 truth passes, and an output that is the
    fp64 arithmetic of one wrong use of the scale, rounded the same way, is refused"""
    D, lens = 64, sv.LENS
    variant = {None: "alibi", WRONG[0]: "alibi", WRONG[1]: "sink", WRONG[2]: "softcap", WRONG[3]: "plain"}[wrong]
    qs, K, V, k8, kd = _decode_problem(dtype, scale, fmt="e4m3" if variant == "softcap" else None)
    slopes = vck.M().alibi_slopes(8, device="cpu") / 8
    sinks = torch.linspace(0.0, 8.0, 8)
    mods = dict(alibi=dict(slopes=slopes), sink=dict(sinks=sinks), softcap=dict(cap=30.0), plain={})[variant]
    truth = lambda s: sv.truth_seqs(qs, K, V, lens, s, -1, 0, **mods)

    def run(m, s):
        q2 = [q * m for q in qs]
        if wrong == WRONG[0]:
            out = sv.truth_seqs(q2, K, V, lens, s, -1, 0, slopes=slopes * s)
        elif wrong == WRONG[1]:
            out = sv.truth_seqs(q2, K, V, lens, s, -1, 0, sinks=sinks * s)
        elif wrong == WRONG[2]:            # tanh(scale * s / softcap) on the bytes' scores: k_descale left out of the coefficient
            out = sv.truth_seqs(q2, k8, V, lens, s, -1, 0, cap=30.0)
        else:
            out = sv.truth_seqs(q2, K, V, lens, s, -1, 0, **mods)
        if wrong == WRONG[3]:              # LSE = m * D ** -0.5 + log l for m * scale + log l, m the row's largest raw score
            for t in out:
                fin = torch.isfinite(t["LSE"])
                m_raw = torch.where(fin, t["SABS"] / s, torch.zeros_like(t["SABS"]))   # (an upper bound of it: enough here)
                t["LSE"] = t["LSE"] + m_raw * (D ** -0.5 - s)
        return [(t["O"].to(dtype), t["LSE"].float()) for t in out]
    check = lambda res, gt, n: sv.check_seqs("cpu", res, gt, dtype, sv.RELS[variant][dtype], sv.LSE_BOUNDS[variant][dtype])
    r = dict(id="cpu-%s" % wrong, section="host", dtype=dtype, scale=scale, D=D)
    args = (r, run, truth, check, sv._o_list, sv._t_list, [1, 2], (1,))
    if wrong is None:
        sv.held(*args)
    else:
        with pytest.raises(AssertionError):
            sv.held(*args)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("scale", SCALES)
def test_training_checks_refuse_each_wrong_use_of_the_scale(scale, dtype):
    """the ALiBi and sink files' _check as the GPU module calls it: slope * scale for slope / a sink scaled by the scale in
    O and the gradients, and an LSE stored as m * D ** -0.5 + log l, in the style of tests/test_host_variantcheck.py"""
    B, H, Hkv, Sq, Sk, D, window = 1, 6, 2, 101, 75, 64, (20, 10)
    g = torch.Generator().manual_seed(Sq + Sk + D)
    Q = (torch.randn(B, H, Sq, D, generator=g) * (D ** -0.5 / scale)).to(dtype)
    K, V = (torch.randn(B, Hkv, Sk, D, generator=g).to(dtype) for _ in range(2))
    dO = torch.randn(B, H, Sq, D, generator=g).to(dtype)
    vis = ar.visible(Sq, Sk, window[0], window[1], "cpu")
    few = bc.few_rows(vis)
    plain = ar.attention_fp64(Q, K, V, None, scale, vis)["O"]
    slopes = 2.0 ** -(torch.arange(H, dtype=torch.float64) + 1)
    sinks = torch.linspace(0, 8, H)
    for mod, kw, bad in ((tal, dict(slopes=slopes, dist=ar.distance(Sq, Sk, "cpu")), dict(slopes=slopes * scale)),
                         (tsk, dict(sinks=sinks), dict(sinks=sinks * scale))):
        gt = ar.attention_fp64(Q, K, V, dO, scale, vis, **kw)

        def rounded(t):
            got = {n: t[n].to(dtype) for n in ("O", "dQ", "dK", "dV")}
            got["LSE"] = t["LSE"].float()
            return got
        mod._check("good", gt, rounded(gt), dO, dtype, "ws", plain, few)
        if scale != 1.0:                   # (times 1.0 is no error)
            with pytest.raises(AssertionError):
                mod._check("wrong transform", gt, rounded(ar.attention_fp64(Q, K, V, dO, scale, vis, **dict(kw, **bad))), dO, dtype,
                           "ws", plain, few)
        got = rounded(gt)
        fin = torch.isfinite(gt["LSE"])
        raw_max = torch.where(fin, gt["SABS"] / scale, torch.zeros_like(gt["SABS"]))
        got["LSE"] = (gt["LSE"] + raw_max * (D ** -0.5 - scale)).float()
        with pytest.raises(AssertionError):
            mod._check("wrong LSE", gt, got, dO, dtype, "ws", plain, few)
