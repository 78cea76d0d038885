"""Every score transform, cache format and decode geometry at a softmax scale other than 1/sqrt(D), against the fp64
reference at that scale (tests/attn_ref.py; for a quantised cache on the fp64 dequantised cache).

tests/test_gpu_scale.py covers the plain entry points.  This module covers what takes the scale in another form: the
family-1 forward under ALiBi (fp16: slope / scale), sinks (fp16: z / scale; log2 units under the soft cap) and the soft
cap (scale / softcap), with their LSE (m * scale + log l) and backward kernels; and the decode body (c2 = scale * kd *
log2 e, the capped coefficient scale * kd / softcap, the per-token K scale in front of the tanh, ALiBi behind s * c2, the
sink never scaled, D = 256's two half-contractions) on the padded, paged and packed launch paths over 16-bit, per-tensor
e4m3, per-token e4m3 and MXFP4 caches.

Scales: test_gpu_scale.SCALES (0.02 and 1.0), in that file's moderate regime: the Q amplitude of the variant's own test is
multiplied by D ** -0.5 / scale (soft-capped cases: test_gpu_softcap._amp at the scale), so scale * q.k has the
distribution it has in the variant's file and that file's bounds apply unchanged -- every bound here is imported from
the variant's file, none is new.  Every case asserts that the scale matters, twice, by test_gpu_scale.FAR: the fp64 truth
at the scale is at least FAR (relFro) from the fp64 truth at D ** -0.5 on the same inputs, and so is the kernel's O;
decode cases take both over the sequences of at least quantcapcheck.MATTERS_FROM keys.  Every decode call also passes an
exactness check: 2 q at scale / 2 returns the bits of q at scale, O and LSE (doubling is exact in fp16 / bf16 and in the
fp32 accumulation, and every use of the scale in csrc/fa_decode_body.inc is a product with the score).

TABLE lists every (case, dtype, scale) with the functions it calls and the recipe of its inputs;
tests/test_host_scale_variants.py pins on the CPU that every public function taking softmax_scale is in it and that the
reference-only half of the FAR condition holds for every row.  One line of measured errors per row goes to the file
MI355FA_SCALE_VARIANTS_ERRORS names, if any (profiles/scale_variants_errors.jsonl).  Measured on an MI355X over every row:
the largest O relFro 3.8e-4 fp16 / 3.4e-3 bf16 (bounds 1e-3 / 8e-3), the largest LSE row error 1.0e-5 fp16 / 1.5e-2 bf16
(the bf16 soft-cap training case, at its bound's a = 1.5e-2 plus 2^-8 of the row's largest logit), the smallest FAR
figure 0.55 for the truth and for the kernel alike; no case needed the eager yardstick, and no variant failed the
exactness check.  A scratch build with any one of these altered fails cases here: the fp16 alibi_k factor or the fp16
sink_m factor of csrc/fa_fwd_body.inc taken at 1/sqrt(D) (the fp16 ALiBi / sink training cases), k_descale left out of the
capped decode coefficient (every per-tensor e4m3 soft-capped case), the per-token K scale applied behind the tanh (every
per-token soft-capped case)."""
import json
import os

import pytest
import torch

import attn_ref as ar
import blockcheck as bc
import fa_oracle as fo
import fp8tokencheck as tk
import pagedcheck as pc
import quantcapcheck as qc
import raggedcheck as rc
import test_gpu_alibi as tal
import test_gpu_kvcache as tkv
import test_gpu_kvcache_fp4 as t4
import test_gpu_kvcache_quant_softcap as tqs
import test_gpu_paged as tpg
import test_gpu_ragged as trg
import test_gpu_ragged_fp4 as tr4
import test_gpu_ragged_quant_softcap as trqs
import test_gpu_scale as tsl
import test_gpu_sink as tsk
import test_gpu_softcap as tsc
import variantcheck as vck
from quantcapcheck import MATTERS_FROM
from test_gpu_scale import FAR, SCALES

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
NAME = {F16: "fp16", BF16: "bf16"}
DTYPES = [F16, BF16]
SC, PAGE = 704, 32                        # decode cache rows, keys per page (22 pages per sequence)
LENS = [2, 302, 652]                      # decode key counts: one below MATTERS_FROM, two above


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


# ---------------------------------------------------------------- the case table
TABLE = []


def row(section, fns, tag, dtype, scale, **recipe):
    """One (case, dtype, scale): the public functions it calls and the recipe of its inputs (far_on rebuilds them on any
    device).  recipe: kind "train" (B, H, Hkv, Sq, Sk, window, top-left aligned) or "decode" (H, Hkv, S: the query count
    per sequence, lens, window (wl, wr), bottom-right aligned); D, amp (Q), kamp (K and V before a quantiser), fmt (None: a
    16-bit cache; "e4m3", "token", "fp4": that format's own quantiser; "rows": fp8tokencheck.rows of amax 2^-span .. 2^span
    (6: twelve octaves) under the per-token quantiser; "nibbles": test_gpu_kvcache_fp4.make4's bytes), descale_mul, cap,
    slopes, sinks, mods (the transform keywords a paged / packed call is given), seed."""
    r = dict(section=section, fns=tuple(fns), id="%s-%s-s%g" % (tag, NAME[dtype], scale), dtype=dtype, scale=scale, **recipe)
    TABLE.append(r)
    return r


def _slopes(spec, B, H, device, g):
    """the ALiBi slopes of a recipe: a kind of test_gpu_alibi._slopes, or "rand" (test_gpu_paged.Case's, (H,); "randB":
    test_gpu_ragged.Step's, (B, H))"""
    if spec is None:
        return None
    if spec in ("rand", "randB"):
        return torch.rand(*((B, H) if spec == "randB" else (H,)), generator=g, device=device) * 0.5 + 0.01
    s = vck.M().alibi_slopes(H, device=device)
    return {"geo": s, "steep": s * 2, "neg": -s / 16,
            "batch": (s[None, :] * torch.linspace(0.25, 2.0, B, device=device)[:, None]).contiguous()}[spec]


def _sinks(spec, H, device, g):
    if spec is None:
        return None
    return torch.randn(H, generator=g, device=device) if spec == "randn" else \
        torch.linspace(spec[0], spec[1], H, device=device, dtype=torch.float32)


def _cache64(r, shape, device, g):
    """K and V [B, H_kv, S, D] in fp64 as the row's format holds them"""
    fmt, dtype, kamp = r.get("fmt"), r["dtype"], r.get("kamp", 1.0)
    out = []
    for _ in range(2):
        if fmt == "nibbles":
            ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g, device=device, dtype=torch.int32).to(torch.uint8)
            out.append(qc._F4().dequantize_kv_mxfp4(ri(0, 256, *shape[:-1], shape[-1] // 2), ri(121, 134, *shape[:-1], shape[-1] // 32),
                                                     torch.float64))
            continue
        if fmt == "rows":
            x = torch.randn(*shape, generator=g, device=device)
            e = (torch.rand(*shape[:-1], 1, generator=g, device=device) * 2.0 - 1.0) * r.get("span", 6.0)
            x = x / x.abs().amax(dim=-1, keepdim=True) * torch.exp2(e)
        else:
            x = torch.randn(*shape, generator=g, device=device) * kamp
        if fmt is None:
            out.append(x.to(dtype).double())
        elif fmt == "fp4":
            out.append(qc._F4().dequantize_kv_mxfp4(*qc._F4().quantize_kv_mxfp4(x), torch.float64))
        elif fmt in ("token", "rows"):
            out.append(tk.deq64(*tk.T().quantize_kv_fp8_per_token(x)))
        else:
            x8, d = vck.M().quantize_kv_fp8(x)
            out.append(x8.double() * (d.double() * r.get("descale_mul", 1.0)).reshape(shape[0], shape[1], 1, 1))
    return out


def far_on(r, device):
    """The reference-only half of the FAR condition for one row of TABLE, with the row's recipe on `device`: relFro of the
    fp64 truth at the row's scale against the fp64 truth at D ** -0.5 on the same inputs (decode rows: over the sequences
    with queries and at least MATTERS_FROM keys).  No kernel is involved."""
    g = torch.Generator(device=device).manual_seed(r.get("seed", 0))
    D, H, Hkv, scale, dtype = r["D"], r["H"], r["Hkv"], r["scale"], r["dtype"]
    rnd = lambda *s: torch.randn(*s, generator=g, device=device)
    both = lambda f: (f(scale), f(D ** -0.5))
    if r["kind"] == "train":
        B, Sq, Sk, (wl, wr) = r["B"], r["Sq"], r["Sk"], r["window"]
        Q = (rnd(B, H, Sq, D) * r["amp"]).to(dtype)
        K, V = (rnd(B, Hkv, Sk, D).to(dtype) for _ in range(2))
        kw = dict(cap=r.get("cap"), sinks=_sinks(r.get("sinks"), H, device, g))
        if r.get("slopes"):
            kw.update(slopes=_slopes(r["slopes"], B, H, device, g), dist=ar.distance(Sq, Sk, device))
        a, b = both(lambda s: ar.attention_fp64(Q, K, V, None, s, ar.visible(Sq, Sk, wl, wr, device), **kw)["O"])
        return fo.rel_fro(b, a)
    S, lens, (wl, wr) = r["S"], r["lens"], r["window"]
    B = len(lens)
    qs = [(rnd(1, H, s, D) * r["amp"]).to(dtype) for s in S]
    if r.get("packed_train"):               # a packed training batch: top-left aligned, every sequence counts
        num = den = 0.0
        slopes, sinks = _slopes(r.get("slopes"), B, H, device, g), _sinks(r.get("sinks"), H, device, g)
        for b, q in enumerate(qs):
            k, v = (rnd(1, Hkv, lens[b], D).to(dtype) for _ in range(2))
            kw = dict(sinks=sinks)
            if slopes is not None:
                kw.update(slopes=slopes[b], dist=ar.distance(S[b], lens[b], device))
            a, b_ = both(lambda s: ar.attention_fp64(q, k, v, None, s, ar.visible(S[b], lens[b], wl, wr, device), **kw)["O"])
            num, den = num + float((a - b_).square().sum()), den + float(b_.square().sum())
        return (num / den) ** 0.5
    K, V = _cache64(r, (B, Hkv, max(lens), D), device, g)
    slopes = _slopes(r.get("slopes"), B, H, device, g)
    mods = dict(cap=r.get("cap"), slopes=None if slopes is None else slopes / r.get("slopes_div", 1.0),
                sinks=_sinks(r.get("sinks"), H, device, g))
    long = [b for b in range(B) if S[b] and lens[b] >= MATTERS_FROM]
    assert long, r["id"]
    a, b = both(lambda s: _cat([t and t["O"] for t in truth_seqs(qs, K, V, lens, s, wl, wr, **mods)], long))
    return fo.rel_fro(b, a)


# ---------------------------------------------------------------- the truth and the checks of the decode cases
def truth_seqs(qs, K, V, lens, scale, wl, wr, cap=None, slopes=None, sinks=None):
    """[dict(O [1, H, S_b, D], LSE, SABS [1, H, S_b]) or None (no query)] in fp64: sequence b's queries qs[b] over the first
    lens[b] rows of K, V [B, H_kv, S, D] (fp64), bottom-right aligned; slopes (H,) or (B, H)."""
    out = []
    for b, q in enumerate(qs):
        _, H, Sq, D = q.shape
        L = lens[b]
        if Sq == 0:
            out.append(None)
            continue
        kw = {}
        if slopes is not None:
            kw = dict(slopes=slopes if slopes.dim() == 1 else slopes[b], dist=ar.distance(Sq, L, q.device, L=L))
        r = ar.attention_fp64(q, K[b:b + 1, :, :L], V[b:b + 1, :, :L], None, scale, ar.visible(Sq, L, wl, wr, q.device, L=L),
                              cap=cap, sinks=sinks, **kw)
        out.append({n: r[n] for n in ("O", "LSE", "SABS")})
    return out


def _cat(parts, which):
    return torch.cat([parts[b].reshape(-1) for b in which])


def split_batch(res):
    """(O [B, H, S_q, D], LSE [B, H, S_q]) -> [(O [1, ...], LSE [1, ...])] per sequence"""
    return [(res[0][b:b + 1], res[1][b:b + 1]) for b in range(res[0].shape[0])]


def same_results(a, b):
    return len(a) == len(b) and all(x is None and y is None or (bc.same_bits(x[0], y[0]) and bc.same_bits(x[1], y[1]))
                                    for x, y in zip(a, b))


def check_seqs(tag, res, gt, dtype, rel, lse_bound):
    """the whole O (every sequence with queries) within relFro `rel`, LSE row by row within a + u * SABS and -inf exactly
    where the truth is, exact zeros where the truth has them.  Returns (O relFro, the worst sequence's relFro, the largest
    LSE row error)."""
    have = [b for b, t in enumerate(gt) if t is not None]
    err = fo.rel_fro(_cat([gt[b]["O"] for b in have], range(len(have))), _cat([res[b][0] for b in have], range(len(have))))
    assert err <= rel, (tag, "O relFro", err, rel)
    a, u = lse_bound
    worst, lmax = 0.0, 0.0
    for b in have:
        (o, lse), t = res[b], gt[b]
        assert o.shape == t["O"].shape and o.dtype == dtype and lse.dtype == torch.float32, (tag, b)
        worst = max(worst, fo.rel_fro(t["O"], o) if t["O"].abs().sum() > 0 else 0.0)
        fin = torch.isfinite(t["LSE"])
        assert torch.equal(torch.isneginf(lse), ~fin), (tag, b, "LSE = -inf exactly on the keyless rows")
        lerr = (lse.double() - t["LSE"]).abs()[fin]
        assert (lerr <= a + u * t["SABS"][fin]).all(), (tag, b, "LSE", lerr.max().item())
        assert (o[(t["O"] == 0).all(-1)] == 0).all(), (tag, b, "structural zeros")
        lmax = max(lmax, lerr.max().item() if lerr.numel() else 0.0)
    return err, worst, lmax


def record(r, figures, ref_far, far):
    """one line of profiles/scale_variants_errors.jsonl: appended to the file MI355FA_SCALE_VARIANTS_ERRORS names, if any"""
    num = lambda x: None if x is None else float("%.4g" % x)
    line = dict(case=r["id"], section=r["section"], dtype=NAME[r["dtype"]], scale=r["scale"], o_rel_fro=num(figures[0]),
                worst_block=num(figures[1]), worst_lse_row=num(figures[2]), far_truth=num(ref_far), far_kernel=num(far))
    print(json.dumps(line))
    path = os.environ.get("MI355FA_SCALE_VARIANTS_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def held(r, run, truth, check, o_parts, t_parts, long, counts, exact=True):
    """The conditions every decode case meets at every forced split count of `counts`.  run(qmul, scale) -> the result of
    the call on qmul * q; truth(scale) -> the fp64 truth; check(result, truth, n) -> (O relFro, worst block, worst LSE
    row) asserts the variant's own bounds; o_parts(result) / t_parts(truth): O as a list per sequence, of which `long` have
    at least MATTERS_FROM keys.  Asserted here: the truth at the scale is FAR from the truth at D ** -0.5, so is the
    result, and 2 q at scale / 2 gives the result's bits."""
    scale = r["scale"]
    gt, dflt = truth(scale), truth(r["D"] ** -0.5)
    ref_far = fo.rel_fro(_cat(t_parts(dflt), long), _cat(t_parts(gt), long))
    assert ref_far >= FAR, "%s: a weak input, the fp64 truth at the scale is within %.3e of the one at D ** -0.5" % (r["id"], ref_far)
    worst, far_min = (0.0, 0.0, 0.0), float("inf")
    for n in counts:
        vck.splits(n)
        res = run(1.0, scale)
        _sync()
        worst = tuple(max(a, b) for a, b in zip(worst, check(res, gt, n)))
        far = fo.rel_fro(_cat(t_parts(dflt), long), _cat(o_parts(res), long))
        assert far >= FAR, "%s, %d splits: O is within %.3e of the attention at D ** -0.5" % (r["id"], n, far)
        far_min = min(far_min, far)
        if exact:
            twice = run(2.0, scale / 2)
            _sync()
            assert all(bc.same_bits(x, y) for x, y in zip(o_parts(res), o_parts(twice))), \
                "%s, %d splits: 2 q at scale / 2 changes bits of O" % (r["id"], n)
            assert all(bc.same_bits(x, y) for x, y in zip(lse_parts(res), lse_parts(twice))), \
                "%s, %d splits: 2 q at scale / 2 changes bits of LSE" % (r["id"], n)
    record(r, worst, ref_far, far_min)


def lse_parts(res):
    return [p[1] for p in res if p is not None] if isinstance(res, list) else [res[1]]


def pair_o(res):
    return [res[0][b] for b in range(res[0].shape[0])]


def list_o(res):
    return [p[0] for p in res]


# ================================================================ a, b. training: ALiBi, sinks, the soft cap
def _picks(cases):
    """the first fp16 case, the first bf16 case and the g = 7 case of a variant file's CASES"""
    return [next(c for c in cases if c[1] == F16), next(c for c in cases if c[1] == BF16),
            next(c for c in cases if c[3] == 7 * c[4])]


def _train_recipe(D, H, Hkv, Sq, Sk, window, amp, **kw):
    return dict(kind="train", B=2, D=D, H=H, Hkv=Hkv, Sq=Sq, Sk=Sk, window=window, amp=amp, seed=Sq + Sk + D, **kw)


TRAIN = []
for _c in _picks(tal.CASES):
    for _s in SCALES:
        TRAIN.append(("alibi", _c, _s, row("a", ("flash_attention_alibi", "flash_attention_alibi_forward", "flash_attention_alibi_backward"),
                                           "train-alibi-" + _c[0], _c[1], _s,
                                           **_train_recipe(*_c[2:8], amp=_c[2] ** -0.5 / _s, slopes=_c[8]))))
for _c in _picks(tsk.CASES):
    for _s in SCALES:
        TRAIN.append(("sink", _c, _s, row("a", ("flash_attention_sink", "flash_attention_sink_forward", "flash_attention_sink_backward"),
                                          "train-sink-" + _c[0], _c[1], _s,
                                          **_train_recipe(*_c[2:8], amp=_c[2] ** -0.5 / _s, sinks=(0.0, 8.0)))))
for _c in _picks(tsc.CASES)[:2]:          # b: 0.02 is below anything in test_gpu_softcap.py, where fp16's scale / softcap is smallest
    for _s in SCALES:
        TRAIN.append(("softcap", _c, _s, row("b", ("flash_attention_softcap", "flash_attention_softcap_forward",
                                                   "flash_attention_softcap_backward"), "train-softcap-" + _c[0], _c[1], _s,
                                             **_train_recipe(*_c[2:8], amp=tsc._amp(_c[8], _s, _c[2]), cap=_c[8]))))


def _train_figures(gt, got):
    blk = fo.block_errors(gt["O"], got["O"])
    lse = None
    if "LSE" in got:
        fin = torch.isfinite(gt["LSE"])
        lse = (got["LSE"].double() - gt["LSE"]).abs()[fin].max().item()
    return fo.rel_fro(gt["O"], got["O"]), blk[torch.isfinite(blk)].max().item(), lse


@pytest.mark.parametrize("variant,case,scale,r", TRAIN, ids=[t[3]["id"] for t in TRAIN])
def test_training_variants_match_fp64_at_the_scale(variant, case, scale, r):
    """autograd, the raw C ABI without the q_scaled workspace and (bf16) with it, as the variant's own file runs them: O,
    dQ, dK, dV, LSE rows, blocks, structural zeros (and dz) through that file's _check; the *_forward / *_backward
    functions at the scale launch what autograd launches."""
    M = vck.M()
    tag, dtype, D, H, Hkv, Sq, Sk, window = case[:8]
    Q, K, V, dO = vck.inputs(2, H, Hkv, Sq, Sk, D, dtype, seed=Sq + Sk + D, amp=r["amp"])
    vis = ar.visible(Sq, Sk, window[0], window[1], "cuda")
    few = bc.few_rows(vis)
    if variant == "alibi":
        x = tal._slopes(case[8], 2, H)
        kw = dict(slopes=x, dist=ar.distance(Sq, Sk, "cuda"))
        auto = lambda: vck.autograd_run(lambda q, k, v: M.flash_attention_alibi(q, k, v, x, window_size=window, softmax_scale=scale),
                                        Q, K, V, dO)
        raw = lambda ws: tal._raw(Q, K, V, dO, x, window, scale, ws)
        check, fwd, bwd = tal._check, M.flash_attention_alibi_forward, M.flash_attention_alibi_backward
    elif variant == "sink":
        x = tsk._sinks(H)
        kw = dict(sinks=x)
        auto = lambda: tsk._autograd(Q, K, V, dO, x, window, scale=scale)
        raw = lambda ws: tsk._raw(Q, K, V, dO, x, window, scale, ws)
        check, fwd, bwd = tsk._check, M.flash_attention_sink_forward, M.flash_attention_sink_backward
    else:
        x = case[8]
        kw = dict(cap=x)
        auto = lambda: vck.autograd_run(tsc._call(x, window, scale), Q, K, V, dO)
        raw = lambda ws: tsc._raw(Q, K, V, dO, x, window, scale, ws)
        check, fwd, bwd = tsc._check, M.flash_attention_softcap_forward, M.flash_attention_softcap_backward
    gt = ar.attention_fp64(Q, K, V, dO, scale, vis, **kw)
    at_default = ar.attention_fp64(Q, K, V, None, D ** -0.5, vis, **kw)["O"]
    untransformed = ar.attention_fp64(Q, K, V, None, scale, vis)["O"]
    ref_far = fo.rel_fro(at_default, gt["O"])
    assert ref_far >= FAR, "%s: a weak input, the fp64 truth at the scale is within %.3e of the one at D ** -0.5" % (tag, ref_far)
    runs = [("autograd", auto(), "ws"), ("raw", raw(False), "raw")] + ([("ws", raw(True), "ws")] if dtype == BF16 else [])
    figures, far_min = None, float("inf")
    for name, got, mode in runs:
        check("%s s%g %s" % (tag, scale, name), gt, got, dO, dtype, mode, untransformed, few)
        far = fo.rel_fro(at_default, got["O"])
        assert far >= FAR, "%s %s: O is within %.3e of the attention at D ** -0.5" % (tag, name, far)
        far_min = min(far_min, far)
        if "LSE" in got and figures is None:
            figures = _train_figures(gt, got)
    record(r, figures, ref_far, far_min)
    # the Python twins of the two launches
    o, lse = fwd(Q, K, V, x, window[0], window[1], scale)[:2]
    back = bwd(Q, K, V, o, dO, lse, x, window[0], window[1], scale)
    torch.cuda.synchronize()
    auto_got = runs[0][1]
    assert bc.same_bits(o, auto_got["O"]) and bc.same_bits(lse, runs[1][1]["LSE"]), "forward"
    for n, t in zip(("dQ", "dK", "dV"), back):
        assert bc.same_bits(t, auto_got[n]), n


PACKED_TRAIN = [(v, s, row("a", (f,), "packed-train-" + v, BF16, s, kind="decode", D=64, H=4, Hkv=2, S=[130, 257, 5],
                           lens=[70, 300, 5], window=(-1, 0), amp=64 ** -0.5 / s, seed=7, packed_train=True, **kw))
                for v, f, kw in (("alibi", "flash_attention_alibi", dict(slopes="batch")),
                                 ("sink", "flash_attention_sink", dict(sinks=(0.0, 8.0)))) for s in SCALES]


@pytest.mark.parametrize("variant,scale,r", PACKED_TRAIN, ids=[t[2]["id"] for t in PACKED_TRAIN])
def test_packed_training_batch_at_the_scale(variant, scale, r):
    """the packed batch of the variant's file (an empty sequence, one without keys) through packed_case(scale=...)"""
    M = vck.M()
    dtype, D, H, Hkv = BF16, 64, 4, 2
    lens = [(130, 70), (0, 50), (64, 0), (257, 300), (5, 5)]
    if variant == "alibi":
        slopes = tal._slopes("batch", len(lens), H)
        call = lambda q, k, v, **kw: M.flash_attention_alibi(q, k, v, slopes, **kw)
        got, gt, _ = vck.packed_case(call, lambda i, a, b: dict(slopes=slopes[i], dist=ar.distance(a, b, "cuda")),
                                     lambda a, b: a == 0 or b == 0, lens, dtype, D, H, Hkv, seed=7, amp=r["amp"], scale=scale)
        rel = tal.REL[dtype]
    else:
        sinks = tsk._sinks(H)
        got, gt, _ = vck.packed_case(M.flash_attention_sink, lambda i, a, b: dict(sinks=sinks), lambda a, b: a == 0, lens, dtype, D,
                                     H, Hkv, seed=7, amp=r["amp"], extra=sinks.clone().requires_grad_(True), scale=scale)
        rel = tsk.REL[dtype]
        e = tsk._dz_err(gt, got["dz"])
        assert e <= tsk.DZ_BOUND[dtype], e
    vck.check_packed(got, gt, rel)
    ref_far, far = fo.rel_fro(gt["O_DEFAULT"], gt["O"]), fo.rel_fro(gt["O_DEFAULT"], got["O"])
    assert ref_far >= FAR and far >= FAR, (ref_far, far)
    record(r, (fo.rel_fro(gt["O"], got["O"]), None, None), ref_far, far)


# ================================================================ c. padded decoding under the transforms
def _rows_of(mod):
    """the (dtype, D, S_q, window) rows of a variant file's test_decode_matches_fp64, its first three"""
    mark = next(m for m in mod.test_decode_matches_fp64.pytestmark if m.name == "parametrize" and m.args[0].startswith("dtype"))
    return [tuple(v) for v in mark.args[1]][:3]


def _decode_recipe(D, Sq, window, amp, **kw):
    return dict(kind="decode", D=D, H=8, Hkv=2, S=[Sq] * 3, lens=LENS, window=window, amp=amp, seed=D + Sq, **kw)


DECODE = []
for _v, _mod, _fn in (("softcap", tsc, "flash_attention_kvcache_softcap"), ("alibi", tal, "flash_attention_kvcache_alibi"),
                      ("sink", tsk, "flash_attention_kvcache_sink"), ("fp8_sink", tsk, "flash_attention_kvcache_fp8_sink")):
    for _row in _rows_of(_mod):
        _dt, _D, _Sq, _w = _row[:4]
        for _s in SCALES:
            _kw = dict(cap=30.0, amp=tsc._amp(30.0, _s, _D)) if _v == "softcap" else dict(amp=_D ** -0.5 / _s)
            if _v == "alibi":
                _kw.update(slopes=_row[4], slopes_div=8.0)
            if _v.endswith("sink"):
                _kw["sinks"] = (0.0, 8.0)
            if _v == "fp8_sink":
                _kw.update(fmt="e4m3", kamp=1.0)
            DECODE.append((_v, _row, _s, row("c", (_fn,), "decode-%s-d%d-sq%d-w%s" % (_v, _D, _Sq, "x".join(map(str, _w))), _dt, _s,
                                             **_decode_recipe(_D, _Sq, _w, **_kw))))


@pytest.mark.parametrize("variant,case,scale,r", DECODE, ids=[t[3]["id"] for t in DECODE])
def test_padded_decode_variants_match_fp64_at_the_scale(variant, case, scale, r):
    """decode_case(scale=...) at the rows of the variant's file, forced splits 0 / 1 / 3 / 7; the fp8 + sink call over a
    cache with distinct per-(B, H_kv) descales through held()."""
    M = vck.M()
    dtype, D, Sq, window = case[:4]
    worst = [0.0, 0.0, None, None]

    def report(n, err, lerr, ref_far, far):
        worst[:] = [max(worst[0], err), max(worst[1], lerr), ref_far, far if worst[3] is None else min(worst[3], far)]
    if variant != "fp8_sink":
        if variant == "softcap":
            call = lambda q, kc, vc, sl, **kw: M.flash_attention_kvcache_softcap(q, kc, vc, sl, 30.0, **kw)
            args = (lambda Ls: dict(cap=30.0), dtype, D, Sq, window, tsc.REL[dtype], tsc.CAP_MATTERS, tsc.BOUNDS["LSE_BOUND"][dtype])
        elif variant == "alibi":
            slopes = tal._slopes(case[4], 3, 8) / 8
            call = lambda q, kc, vc, sl, **kw: M.flash_attention_kvcache_alibi(q, kc, vc, sl, slopes, **kw)
            dist = lambda Ls: torch.stack([ar.distance(Sq, vck.DECODE_CACHE, "cuda", L=L) for L in Ls])[:, None]
            args = (lambda Ls: dict(slopes=slopes, dist=dist(Ls)), dtype, D, Sq, window, tal.REL[dtype], tal.BIAS_MATTERS,
                    tal.BOUNDS["LSE_BOUND"][dtype])
        else:
            sinks = tsk._sinks(8)
            call = lambda q, kc, vc, sl, **kw: M.flash_attention_kvcache_sink(q, kc, vc, sl, sinks, **kw)
            args = (lambda Ls: dict(sinks=sinks), dtype, D, Sq, window, tsk.REL[dtype], tsk.BIAS_MATTERS, tsk.BOUNDS["LSE_BOUND"][dtype])
        vck.decode_case(call, *args, amp=r["amp"], scale=scale, report=report)
        record(r, (worst[0], None, worst[1]), worst[2], worst[3])
        return
    g = torch.Generator(device="cuda").manual_seed(D + Sq)
    q = (torch.randn(3, 8, Sq, D, device="cuda", generator=g) * r["amp"]).to(dtype)
    kf, vf = (torch.randn(3, 2, SC, D, device="cuda", generator=g) for _ in range(2))
    (k8, kd), (v8, vd) = M.quantize_kv_fp8(kf), M.quantize_kv_fp8(vf * 1.7)
    assert kd.shape == (3, 2) and kd.unique().numel() == 6
    for b, L in enumerate(LENS):
        k8.view(torch.uint8)[b, :, L:] = 0x7F
        v8.view(torch.uint8)[b, :, L:] = 0x7F
    sl, sinks = qc.sl_of(LENS), tsk._sinks(8)
    K, V = (torch.nan_to_num(x.double() * d.double().reshape(3, 2, 1, 1), nan=0.0) for x, d in ((k8, kd), (v8, vd)))
    wl, wr = window
    qs = [q[b:b + 1] for b in range(3)]
    truth = lambda s: truth_seqs(qs, K, V, LENS, s, wl, wr, sinks=sinks)
    plain = _cat([t["O"] for t in truth_seqs(qs, K, V, LENS, scale, wl, wr)], range(3))

    def check(res, gt, n):
        assert fo.rel_fro(plain, _cat(list_o(res), range(3))) >= tsk.BIAS_MATTERS, n
        return check_seqs("fp8 sink n%d" % n, res, gt, dtype, tsk.REL[dtype], tsk.BOUNDS["LSE_BOUND"][dtype])
    run = lambda m, s: split_batch(M.flash_attention_kvcache_fp8_sink(q * m, k8, v8, sl, sinks, kd, vd, window_size=window,
                                                                      softmax_scale=s, return_lse=True))
    held(r, run, truth, check, list_o, lambda gt: [t["O"] for t in gt], [1, 2], (0, 1, 3, 7))


# ================================================================ d, e. paged and packed decoding, D = 256
PAGED_FNS = {"plain": "flash_attention_kvcache", "softcap": "flash_attention_kvcache_softcap", "alibi": "flash_attention_kvcache_alibi",
             "sink": "flash_attention_kvcache_sink", "fp8": "flash_attention_kvcache_fp8", "fp8_sink": "flash_attention_kvcache_fp8_sink"}
MODS = {"plain": (), "softcap": ("softcap",), "alibi": ("alibi_slopes",), "sink": ("sinks",), "fp8": ("k_descale", "v_descale"),
        "fp8_sink": ("sinks", "k_descale", "v_descale")}
P_S, P_LENS = [1, 0, 5, 3], [302, 64, 652, 2]     # packed: query counts and key counts; sequence 1 brings no query
LSE_BOUNDS = {"plain": tsl.LSE_BOUND, "fp8": tsl.LSE_BOUND, "softcap": tsc.BOUNDS["LSE_BOUND"], "alibi": tal.BOUNDS["LSE_BOUND"],
              "sink": tsk.BOUNDS["LSE_BOUND"], "fp8_sink": tsk.BOUNDS["LSE_BOUND"]}
RELS = {"plain": tsl.TOL, "fp8": tsl.TOL, "softcap": tsc.REL, "alibi": tal.REL, "sink": tsk.REL, "fp8_sink": tsk.REL}


def _geometry_recipe(geometry, variant, D, Sq, scale):
    fp8 = variant.startswith("fp8")
    amp = tsc._amp(15.0, scale, D) if variant == "softcap" else D ** -0.5 / scale
    kw = dict(cap=15.0) if variant == "softcap" else {}
    if variant == "alibi":
        kw["slopes"] = "rand" if geometry == "paged" else "randB"
    if variant.endswith("sink"):
        kw["sinks"] = "randn"
    if fp8:
        kw.update(fmt="e4m3", kamp=2.0)
    S, lens = ([Sq] * 3, LENS) if geometry != "packed" else (P_S, P_LENS)
    return dict(kind="decode", D=D, H=8, Hkv=2, S=S, lens=lens, window=(-1, 0), amp=amp, seed=D + len(variant), mods=MODS[variant], **kw)


GEOM = []
for _i, _v in enumerate(tpg.VARIANTS):
    for _dt in DTYPES:
        _D = 64 if _dt == F16 else 128
        GEOM.append(("paged", _v, _dt, SCALES[_i % 2], row("d", ("flash_attention_kvcache_paged", PAGED_FNS[_v]), "paged-" + _v, _dt,
                                                           SCALES[_i % 2], **_geometry_recipe("paged", _v, _D, 3, SCALES[_i % 2]))))
        GEOM.append(("packed", _v, _dt, SCALES[(_i + 1) % 2], row("d", ("flash_attention_kvcache_ragged", "flash_attention_kvcache_paged"),
                                                                  "packed-" + _v, _dt, SCALES[(_i + 1) % 2],
                                                                  **_geometry_recipe("packed", _v, _D, 0, SCALES[(_i + 1) % 2]))))


def _dequantised(c, kc, vc):
    """K, V in fp64 of a Case's or a Step's padded cache (NaN past each length)"""
    K, V = torch.nan_to_num(kc.double(), nan=0.0), torch.nan_to_num(vc.double(), nan=0.0)
    if "k_descale" in c.mods:
        K = K * c.mods["k_descale"].double()[:, :, None, None]
        V = V * c.mods["v_descale"].double()[None, :, None, None]
    return K, V


def _truth_mods(c):
    return dict(cap=c.mods.get("softcap"), slopes=c.mods.get("alibi_slopes"), sinks=c.mods.get("sinks"))


def paged_case(r, variant, dtype, Sq, lens=LENS, page=PAGE):
    """a test_gpu_paged.Case at the row's amplitude: (the case, run, the padded twin of run, truth)"""
    c = tpg.Case(variant, dtype, r["D"], 8, 2, Sq, page, lens, seed=r["seed"], amp=r["amp"], max_pages=SC // page)
    q0 = c.q
    K, V = _dequantised(c, c.kc, c.vc)

    def call(f):
        def run(m, s):
            c.q = q0 * m
            try:
                return split_batch(f(is_causal=True, softmax_scale=s))
            finally:
                c.q = q0
        return run
    truth = lambda s: truth_seqs([q0[b:b + 1] for b in range(len(lens))], K, V, lens, s, -1, 0, **_truth_mods(c))
    return c, call(c.paged), call(c.padded), truth


def packed_step(r, variant, dtype, S=P_S, lens=P_LENS, page=PAGE):
    """a test_gpu_ragged.Step at the row's amplitude: (the step, run, the per-sequence paged twin of run, truth)"""
    st = trg.Step(variant, dtype, r["D"], 8, 2, S, page, lens, seed=r["seed"], max_pages=SC // page)
    q0 = [(x.float() * r["amp"]).to(dtype) for x in st.qs]
    K, V = _dequantised(st, pc.gather(st.kp, st.table), pc.gather(st.vp, st.table))

    def use(m):
        st.qs = [x * m for x in q0]
        st.q = rc.pack(st.qs, st.total)

    def run(m, s):
        use(m)
        o, lse = st.ragged(is_causal=True, softmax_scale=s)
        assert (o[sum(S):] == trg.SENT).all()
        return [(a, b) if a.shape[2] else None for a, b in zip(rc.unpack(o, S), rc.unpack_lse(lse, S))]

    def twin(m, s):
        use(m)
        return st.per_sequence(is_causal=True, softmax_scale=s)
    truth = lambda s: truth_seqs(q0, K, V, lens, s, -1, 0, **_truth_mods(st))
    return st, run, twin, truth


def _o_list(res):
    return [p[0] if p is not None else torch.empty(0) for p in res]


def _t_list(gt):
    return [t["O"] if t is not None else torch.empty(0) for t in gt]


@pytest.mark.parametrize("geometry,variant,dtype,scale,r", GEOM, ids=[t[4]["id"] for t in GEOM])
def test_paged_and_packed_variants_at_the_scale(geometry, variant, dtype, scale, r):
    """pages of 32 keys under a permuted table: the paged call has the bits of the padded call at the same scale on the
    gathered cache, the packed call those of the paged call on each sequence alone, and both meet the truth"""
    if geometry == "paged":
        _, run, twin, truth = paged_case(r, variant, dtype, 3)
        long = [1, 2]
    else:
        _, run, twin, truth = packed_step(r, variant, dtype)
        long = [0, 2]

    def check(res, gt, n):
        assert same_results(res, twin(1.0, scale)), (geometry, variant, n, "the bits of the call it must reproduce")
        return check_seqs("%s %s n%d" % (geometry, variant, n), res, gt, dtype, RELS[variant][dtype], LSE_BOUNDS[variant][dtype])
    held(r, run, truth, check, _o_list, _t_list, long, (0, 1, 3, 7))


D256 = []
for _g, _fns in (("padded", None), ("paged", ("flash_attention_kvcache_paged",)), ("packed", ("flash_attention_kvcache_ragged",))):
    for _v in ("plain", "fp8"):
        for _dt in DTYPES:
            for _s in SCALES:
                D256.append((_g, _v, _dt, _s, row("e", _fns or (PAGED_FNS[_v],), "d256-%s-%s" % (_g, _v), _dt, _s,
                                                  **_geometry_recipe(_g, _v, 256, 11, _s))))


@pytest.mark.parametrize("geometry,variant,dtype,scale,r", D256, ids=[t[4]["id"] for t in D256])
def test_d256_decoding_at_the_scale(geometry, variant, dtype, scale, r):
    """S_q 1 and 11 (packed: 1, 0, 5, 3), forced splits 1 and 3, against the truth under test_gpu_decode_d256.py's bounds:
    test_gpu_kvcache.tol (bf16: PyTorch's SDPA at the same scale) and check_lse, on the dequantised cache for e4m3"""
    for Sq in ((1, 11) if geometry != "packed" else (0,)):
        if geometry == "packed":
            c, run, _, truth = packed_step(r, variant, dtype)
            qs, lens, long = [(x.float() * r["amp"]).to(dtype) for x in c.qs], P_LENS, [0, 2]
            K, V = _dequantised(c, pc.gather(c.kp, c.table), pc.gather(c.vp, c.table))
        else:
            c, paged, padded, truth = paged_case(dict(r, S=[Sq] * 3), variant, dtype, Sq)
            run = paged if geometry == "paged" else padded
            qs, lens, long = [c.q[b:b + 1] for b in range(3)], LENS, [1, 2]
            K, V = _dequantised(c, c.kc, c.vc)
        tol = {}

        def check(res, gt, n):
            worst, lmax = 0.0, 0.0
            for b, (p, t) in enumerate(zip(res, gt)):
                if t is None:
                    continue
                if b not in tol:
                    one = (qs[b], K[b:b + 1].to(dtype), V[b:b + 1].to(dtype), [lens[b]], -1, 0)
                    tol[b] = tkv.tol(dtype, *one, t["O"], scale=scale)
                err = tkv.rel(p[0], t["O"])
                assert err < tol[b], (geometry, variant, Sq, n, b, err, tol[b])
                tkv.check_lse(p[1], t["LSE"])
                assert (p[0][torch.isinf(t["LSE"])] == 0).all()
                worst = max(worst, err)
                lmax = max(lmax, (p[1].double() - t["LSE"]).abs()[torch.isfinite(t["LSE"])].max().item())
            return worst, worst, lmax
        held(dict(r, id="%s-sq%d" % (r["id"], Sq)), run, truth, check, _o_list, _t_list, long, (1, 3))


# ================================================================ f. per-token e4m3 and MXFP4 pools
# per-token rows of amax 2^-2 .. 2^2 here: over twelve octaves (section g has them) a handful of keys carries every row's
# softmax at either scale, and the two truths of the FAR condition sit 0.1 to 0.3 apart, too close to hold for every seed
F_SPAN = 2.0
POOLS = []
for _fmt, _fn in (("token", "flash_attention_kvcache_fp8_token"), ("fp4", "flash_attention_kvcache_fp4")):
    for _sk in (None, (-1.0, 3.0)):
        for _dt in DTYPES:
            for _s in SCALES:
                _r = row("f", (_fn + "_paged", _fn), "%s-paged-%s" % (_fmt, "sinks" if _sk else "plain"), _dt, _s, kind="decode",
                         D=128, H=8, Hkv=2, S=[2] * 3, lens=LENS, window=(-1, 0), amp=(1.0 if _fmt == "token" else 0.03) * 128 ** -0.5 / _s,
                         fmt="rows" if _fmt == "token" else "nibbles", span=F_SPAN, sinks=_sk, seed=128)
                POOLS.append((_fmt, "paged", _sk, _dt, _s, _r))
for _dt in DTYPES:
    for _s in SCALES:
        _r = row("f", ("flash_attention_kvcache_fp4_ragged",), "fp4-packed-d256-sinks", _dt, _s, kind="decode", D=256, H=8, Hkv=2,
                 S=[1, 0, 5], lens=[302, 64, 652], window=(-1, 0), amp=0.03 * 256 ** -0.5 / _s, fmt="nibbles", sinks=(-1.0, 3.0), seed=256)
        POOLS.append(("fp4", "packed", (-1.0, 3.0), _dt, _s, _r))
        _r = row("f", ("flash_attention_kvcache_fp8_token_ragged",), "token-packed-sinks", _dt, _s, kind="decode", D=128, H=8, Hkv=2,
                 S=[1, 0, 5], lens=LENS, window=(-1, 0), amp=128 ** -0.5 / _s, fmt="rows", span=F_SPAN, sinks=(-1.0, 3.0), seed=129)
        POOLS.append(("token", "packed", (-1.0, 3.0), _dt, _s, _r))


@pytest.mark.parametrize("fmt,geometry,sinks,dtype,scale,r", POOLS, ids=[t[5]["id"] for t in POOLS])
def test_per_token_and_mxfp4_pools_at_the_scale(fmt, geometry, sinks, dtype, scale, r):
    """the paged calls of both formats, plain and with sinks (each with the bits of the padded call at the same scale on the
    gathered cache), the packed per-token call and the packed MXFP4 call at D = 256, causal, forced splits 1 and 3, through
    the formats' own checks (fp8tokencheck.held, test_gpu_kvcache_fp4.check)"""
    D, H, Hkv = r["D"], 8, 2
    sk = None if sinks is None else torch.linspace(sinks[0], sinks[1], H, device="cuda", dtype=torch.float32)
    mul = D ** -0.5 / scale
    if fmt == "token":
        S = r["S"]
        q, k8, v8, ks, vs = tk.make(3, H, Hkv, max(S), SC, D, dtype, seed=r["seed"], span=(-F_SPAN, F_SPAN))
        q = (q.float() * mul).to(dtype)
        kp, vp, ksp, vsp, table = tk.scatter(k8, v8, ks, vs, LENS, PAGE, sum(pc.pages_of(L, PAGE) for L in LENS) + 3, SC // PAGE, 5)
        sl = qc.sl_of(LENS)
        K, V = tk.deq64(k8, ks), tk.deq64(v8, vs)
        kw = dict(is_causal=True, sinks=sk)
        if geometry == "packed":
            qs = [q[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)]
            run = lambda m, s: [p if p[0].shape[2] else None
                                for p in tk.packed([x * m for x in qs], kp, vp, ksp, vsp, sl, table, softmax_scale=s, **kw)]
            truth = lambda s: [tk.truth(qs[b], K[b:b + 1], V[b:b + 1], LENS[b:b + 1], True, (-1, -1), s, sk) if S[b] else None
                               for b in range(3)]

            def check(res, gt, n):
                worst = (0.0, 0.0, 0.0)
                for b in range(3):
                    if S[b]:
                        tk.held("token packed n%d b%d" % (n, b), qs[b], *res[b], *gt[b], LENS[b:b + 1])
                        worst = tuple(max(x, y) for x, y in zip(worst, _pool_figures(res[b], gt[b])))
                return worst
            held(r, run, truth, check, _o_list, lambda gt: [t[0] if t is not None else torch.empty(0) for t in gt], [2], (1, 3))
            return
        gathered = (pc.gather(kp, table), pc.gather(vp, table), tk.gather_scales(ksp, table), tk.gather_scales(vsp, table))
        run = lambda m, s: tk.paged(q * m, kp, vp, ksp, vsp, sl, table, softmax_scale=s, **kw)
        truth = lambda s: tk.truth(q, K, V, LENS, True, (-1, -1), s, sk)

        def check(res, gt, n):
            tk.held("token paged n%d" % n, q, *res, *gt, LENS)
            assert tk.same(res, tk.padded(q, *gathered, sl, softmax_scale=scale, **kw)), "paged = padded on the gathered cache"
            return _pool_figures(res, gt)
        held(r, run, truth, check, pair_o, lambda gt: pair_o(gt), [1, 2], (1, 3))
        return
    if geometry == "paged":
        q, kc, vc, ks, vs = t4.make4(3, H, Hkv, 2, SC, D, dtype, seed=r["seed"])
        q = (q.float() * mul).to(dtype)
        pad = [t.clone() for t in (kc, vc, ks, vs)]
        for b, L in enumerate(LENS):
            for t in pad:
                t[b, :, L:] = t4.FF
        pools, table = t4.scatter4(pad, LENS, PAGE, sum(pc.pages_of(L, PAGE) for L in LENS) + 4, SC // PAGE, seed=6)
        sl = qc.sl_of(LENS)
        K, V = t4.deq64(kc, ks), t4.deq64(vc, vs)
        run = lambda m, s: t4._F().flash_attention_kvcache_fp4_paged(q * m, *pools, sl, table, is_causal=True, softmax_scale=s,
                                                                    return_lse=True, sinks=sk)
        truth = lambda s: t4.truth(q, K, V, LENS, -1, 0, sk, s)

        def check(res, gt, n):
            t4.check("fp4 paged n%d" % n, q, *res, *gt)
            padded = t4._F().flash_attention_kvcache_fp4(q, *pad, sl, is_causal=True, softmax_scale=scale, return_lse=True, sinks=sk)
            assert t4.same(res, padded), "paged = padded at the same scale"
            return _pool_figures(res, gt)
        held(r, run, truth, check, pair_o, lambda gt: pair_o(gt), [1, 2], (1, 3))
        return
    S, lens = r["S"], r["lens"]
    st = tr4.step(H, Hkv, D, dtype, PAGE, seed=r["seed"], lens=lens, S=S)
    qs = [(x.float() * mul).to(dtype) for x in st["q_seq"]]
    cu, sl, total = rc.cu_of(S, device="cuda"), qc.sl_of(lens), sum(S) + tr4.PAD
    K, V = t4.deq64(st["pad"][0], st["pad"][2]), t4.deq64(st["pad"][1], st["pad"][3])

    def run(m, s):
        o, lse = tr4._R().flash_attention_kvcache_fp4_ragged(rc.pack([x * m for x in qs], total, fill=0.0), *st["pools"], cu, sl,
                                                            st["table"], is_causal=True, softmax_scale=s, return_lse=True, sinks=sk)
        return [(a, b) if a.shape[2] else None for a, b in zip(rc.unpack(o, S), rc.unpack_lse(lse, S))]
    truth = lambda s: [t4.truth(qs[b], K[b:b + 1], V[b:b + 1], [lens[b]], -1, 0, sk, s) if S[b] else None for b in range(len(S))]

    def check(res, gt, n):
        worst = (0.0, 0.0, 0.0)
        for b in range(len(S)):
            if S[b]:
                t4.check("fp4 packed d256 n%d b%d" % (n, b), qs[b], *res[b], *gt[b])
                worst = tuple(max(x, y) for x, y in zip(worst, _pool_figures(res[b], gt[b])))
        return worst
    held(r, run, truth, check, _o_list, lambda gt: [t[0] if t is not None else torch.empty(0) for t in gt],
         [0, 2], (1, 3))


def _pool_figures(res, gt):
    (o, lse), (O, LSE) = res, gt
    fin = torch.isfinite(LSE)
    return fo.rel_fro(O, o), fo.block_errors(O, o, block=o.shape[2]).max().item(), (lse.double() - LSE).abs()[fin].max().item()


# ================================================================ g. soft-capped quantised decoding
QUANT_FNS = ("flash_attention_kvcache_quant_softcap", "flash_attention_kvcache_quant_softcap_paged")
QUANT = []
for _fmt, _kind in (("e4m3", "natural"), ("e4m3", "times3"), ("token", "natural"), ("token", "rows"), ("fp4", "natural")):
    for _dt in DTYPES:
        for _s in (SCALES if _kind != "rows" else SCALES[:1]):
            for _i in (1, 2):
                _Sq, _H, _Hkv, (_causal, _w), _cap, _n = tqs.COMBOS[_i]
                QUANT.append((_fmt, _kind, _i, _dt, _s, row(
                    "g", QUANT_FNS, "quantcap-%s-%s-combo%d" % (_fmt, _kind, _i), _dt, _s, kind="decode", D=128, H=_H, Hkv=_Hkv,
                    S=[_Sq] * 3, lens=tqs.LENS, window=tkv.window_of(_causal, _w), amp=tsc._amp(_cap, _s, 128), cap=_cap,
                    fmt="rows" if _kind == "rows" else _fmt, descale_mul=3.0 if _kind == "times3" else 1.0, seed=100 * 128 + _i)))
QUANT_PACKED = []
for _fmt in qc.FORMATS:
    for _D in (128, 256):
        for _dt in DTYPES:
            for _s in SCALES:
                for _i in (0, 1):
                    _H, (_causal, _w), _cap, _n = trqs.COMBOS[_i]
                    QUANT_PACKED.append((_fmt, _D, _i, _dt, _s, row(
                        "g", ("flash_attention_kvcache_quant_softcap_ragged",) + (QUANT_FNS[1:] if _D != 256 else ()),
                        "quantcap-packed-%s-d%d-combo%d" % (_fmt, _D, _i), _dt, _s, kind="decode", D=_D, H=_H, Hkv=2, S=trqs.S,
                        lens=trqs.LENS, window=tkv.window_of(_causal, _w), amp=tsc._amp(_cap, _s, _D), cap=_cap, fmt=_fmt,
                        seed=10 * _D + _i)))


def _quant_truth(q, c, lens, cap, causal, window):
    return lambda s: qc.truth(q, c, lens, cap, causal, window, scale=s)


@pytest.mark.parametrize("fmt,kind,combo,dtype,scale,r", QUANT, ids=[t[5]["id"] for t in QUANT])
def test_soft_capped_quantised_decode_at_the_scale(fmt, kind, combo, dtype, scale, r):
    """the padded call against qc.truth(scale=...) through qc.check, and the paged call with its bits on the gathered cache;
    e4m3 with the natural descales and with 3 x them, per-token also over rows spanning twelve octaves"""
    Sq, H, Hkv, (causal, window), cap, n = tqs.COMBOS[combo]
    D, lens = 128, tqs.LENS
    if kind == "rows":
        q, k8, v8, ks, vs = tk.make(tqs.B, H, Hkv, Sq, tqs.SC, D, dtype, seed=r["seed"])
        q, c = (q.float() * r["amp"]).to(dtype), qc.Cache("token", k8, v8, ks, vs)
    else:
        q, c = qc.make(fmt, tqs.B, H, Hkv, Sq, tqs.SC, D, dtype, cap, scale=scale, seed=r["seed"],
                       **(dict(descale_mul=3.0) if kind == "times3" else {}))
    pools, table = qc.scatter(c, lens, PAGE, tqs.SC // PAGE)
    flat = qc.gather(pools, table)
    sl = qc.sl_of(lens)
    kw = dict(is_causal=causal, window_size=window)
    run = lambda m, s: qc.paged(q * m, pools, sl, table, cap, softmax_scale=s, **kw)

    def check(res, gt, k):
        qc.check("%s n%d" % (r["id"], k), q, *res, gt, lens, matters=kind != "rows")
        assert qc.same(res, qc.padded(q, flat, sl, cap, softmax_scale=scale, **kw)), "paged = padded on the gathered cache"
        return _pool_figures(res, (gt["O"], gt["LSE"]))
    held(r, run, _quant_truth(q, c, lens, cap, causal, window), check, pair_o, lambda gt: [gt["O"][b] for b in range(tqs.B)],
         [b for b, L in enumerate(lens) if L >= MATTERS_FROM], (n,))


@pytest.mark.parametrize("fmt,D,combo,dtype,scale,r", QUANT_PACKED, ids=[t[5]["id"] for t in QUANT_PACKED])
def test_soft_capped_quantised_packed_decode_at_the_scale(fmt, D, combo, dtype, scale, r):
    """the packed call against qc.truth(scale=...) per sequence, and (D = 128) the paged call's bits on each sequence alone"""
    H, (causal, window), cap, n = trqs.COMBOS[combo]
    S, lens = trqs.S, trqs.LENS
    q, c = qc.make(fmt, trqs.B, H, 2, max(S), trqs.SC, D, dtype, cap, scale=scale, seed=r["seed"])
    qs = [q[b:b + 1, :, :s].contiguous() for b, s in enumerate(S)]
    pools, table = qc.scatter(c, lens, trqs.PAGE, trqs.SC // trqs.PAGE, seed=r["seed"])
    sl = qc.sl_of(lens)
    kw = dict(is_causal=causal, window_size=window)
    none = lambda res: [p if p[0].shape[2] else None for p in res]
    run = lambda m, s: none(qc.packed([x * m for x in qs], pools, sl, table, cap, total_q=sum(S) + trqs.PAD, softmax_scale=s, **kw))
    truth = lambda s: [qc.truth(qs[b], c.rows(b, trqs.SC), lens[b:b + 1], cap, causal, window, scale=s) if S[b] else None
                       for b in range(len(S))]

    def check(res, gt, k):
        worst = (0.0, 0.0, 0.0)
        for b in range(len(S)):
            if not S[b]:
                continue
            qc.check("%s n%d b%d" % (r["id"], k, b), qs[b], *res[b], gt[b], lens[b:b + 1])
            worst = tuple(max(x, y) for x, y in zip(worst, _pool_figures(res[b], (gt[b]["O"], gt[b]["LSE"]))))
            if D != 256:
                one = qc.paged(qs[b], pools.for_seq(b), sl[b:b + 1], table[b:b + 1], cap, softmax_scale=scale, **kw)
                assert qc.same(res[b], one), ("packed = paged on the sequence alone", b)
        return worst
    held(r, run, truth, check, _o_list, _t_list,
         [b for b, L in enumerate(lens) if S[b] and L >= MATTERS_FROM], (n,))
