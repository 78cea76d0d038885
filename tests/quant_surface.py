"""The quantised-cache and MLA decode calls' surface, pinned: the pybind signature lines of the seven binding functions, and
for each malformed call of the tables below the check that fails FIRST with its exception type and exact message
(tests/golden/quant_errors.json).  tests/paged_surface.py does the same for the 16-bit / per-tensor-FP8 paged calls.

tests/test_host_quant_surface.py and tests/test_gpu_quant_errors.py replay the fixture; this file, run as a script, rewrites
it from the tree it is run in:

    python tests/quant_surface.py            # rewrite
    python tests/quant_surface.py --check    # compare only (exit 1 on a difference)
    python tests/quant_surface.py --out DIR  # write it somewhere else

A call is built by make() / make_mla() from a few named properties (the head dim, a tensor's dtype, how block_table is
malformed, ...); a fault is a small dict of them.  Every table is the ORDERED list of one function's checks, one fault per
check; _table() adds, for neighbours a and b, the case "a+b" that commits both faults, so that the fixture fixes the order
of the checks.  Two faults that set the same property of one tensor cannot be committed together: SAME_PROPERTY names those
properties with the reason, NO_PAIR the other pairs that cannot be built.

cpu_cases() uses CPU tensors only: its calls reach every check in front of the function's first device check (a well-formed
call, "ok", ends at that check).  gpu_cases() holds the checks behind it on device tensors; each is refused before anything
is allocated or launched.  The integer-overflow checks are reached with expanded zero-stride tensors, at no memory cost.
The fixture was recorded from the tree before the quantised bindings were folded onto the shared call path."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = "quant_errors.json"
if PKG not in sys.path:
    sys.path.insert(0, PKG)

F8, F16, BF16, F32, U8, I32 = torch.float8_e4m3fn, torch.float16, torch.bfloat16, torch.float32, torch.uint8, torch.int32
INF, NAN = float("inf"), float("nan")
E4M3, TOKEN, MXFP4 = 0, 1, 2           # quant_softcap_kvcache's formats
FMT_NAMES = {E4M3: "e4m3", TOKEN: "token", MXFP4: "mxfp4"}
B, H = 2, 4

# a property two neighbouring faults both set: no call commits both
SAME_PROPERTY = {
    "q": "q is one tensor: it has one rank, one device, one grad flag",
    "q_dtype": "q has one dtype",
    "D": "q has one head dim",
    "cache": "the caches have one layout",
    "cache_dtype": "the caches have one dtype",
    "cache_D": "the caches' rows have one width",
    "scale": "the scales are one pair of tensors",
    "scale_dtype": "the scales have one dtype",
    "scale_D": "the scales' rows have one width",
    "rows": "the caches have one row count",
    "n": "the caches have one leading size",
    "hk": "the caches have one head count",
    "v_rows": "v_cache has one row count",
    "s_rows": "the scales have one row count",
    "wr": "window_right is one number",
    "is_causal": "is_causal is one flag",
    "sl": "cache_seqlens is one tensor",
    "bt": "block_table is one tensor",
    "cu": "cu_seqlens_q is one tensor",
    "knew": "k_new / v_new are one pair of tensors",
    "sinks": "sinks is one tensor",
    "kd": "k_descale is one tensor",
    "vd": "v_descale is one tensor",
    "out": "out is one tensor",
    "wl": "window_left is one number",
    "window": "window_size is one pair",
    "softcap": "softcap is one number",
    "softmax_scale": "softmax_scale is one number",
    "kv": "kv_cache is one tensor",
    "kvnew": "kv_new is one tensor",
    "format": "format is one number",
}
# (table prefix or "*", a, b): pairs that cannot be built although their properties differ
NO_PAIR = {
    ("*", "q_none", "sl_list"): "the second check (isinstance of cache_seqlens) is the same assert loop as the first",
    ("*", "rank_q", "q_empty"): "q[0] of a packed q has no rows to drop: both faults change q's shape",
}


def _vec(dev, kind, n, two_d_rows=B):
    """an fp32 vector argument (n,), malformed as `kind` says"""
    ones = lambda *s, **k: torch.ones(*s, device=dev, **k)
    return {"ok": lambda: ones(n), "f64": lambda: ones(n).double(), "shape": lambda: ones(n + 1), "2d": lambda: ones(two_d_rows, n),
            "shape_3B": lambda: ones(3, n), "noncontig": lambda: ones(2 * n)[::2], "grad": lambda: ones(n).requires_grad_(True),
            "cpu": lambda: torch.ones(n), "int": lambda: ones(n).int(), "list": lambda: [1.0] * n}[kind]()


def make(dev, mod, fmt, geom, ext, **p):
    """The keyword arguments of one call of module `mod` ("fp4", "tok", "qs") over a cache of format `fmt`, geometry `geom`
    ("padded", "paged", "packed"), for the Python wrapper or (ext) the binding: B 2, H 4, H_kv 2, D 64, 64 rows per page or
    sequence, two pages per sequence, packed rows (1, 4) -- but for the properties p names."""
    g = p.get
    z = lambda *s, dtype=F16, d=dev: torch.zeros(*s, dtype=dtype, device=d)
    paged, packed = geom != "padded", geom == "packed"
    D, hk, rows, n = g("D", 64), g("hk", 2), g("rows", 64), g("n", 4 if paged else B)
    q = z(5, H, D, dtype=g("q_dtype", F16)) if packed else z(B, H, 1, D, dtype=g("q_dtype", F16))
    q = {None: lambda: q, "rank": lambda: q[0], "empty": lambda: q[:0], "cpu": lambda: q.cpu(), "none": lambda: None,
         "grad": lambda: q.requires_grad_(True), "misaligned": lambda: z(*q.shape[:-1], D + 8)[..., 1:D + 1]}[g("q")]()
    # the caches: K and V are one tensor unless a fault sets them apart
    fp4 = fmt == MXFP4
    cD = g("cache_D", D)
    rowb, cdt = (cD // 2, U8) if fp4 else (cD, F8)
    cdt = g("cache_dtype", cdt)

    def lead(rows_, tail, dtype, fill=0.0):
        """[n, hk, rows_, *tail]; a count of 2**31 is an expanded size-1 dimension"""
        real = [1 if s >= 2 ** 31 else s for s in (n, hk, rows_)]
        t = torch.full((*real, *tail), fill, dtype=F32, device=dev).to(dtype)
        return t.expand(n, hk, rows_, *tail) if real != [n, hk, rows_] else t
    kc = vc = lead(rows, (rowb,), cdt)
    ck = g("cache")
    if ck == "rank":
        kc = vc = kc[0]
    elif ck == "misaligned":
        kc = vc = lead(rows, (rowb + 32,), cdt)[..., 1:rowb + 1]
    elif ck == "rowstride":
        kc = lead(rows, (rowb + 16,), cdt)[..., :rowb]
    elif ck == "grad":
        kc = lead(rows, (rowb,), cdt).requires_grad_(True)
    elif ck == "list":
        kc = [0.0]
    elif ck == "v_dtype":
        vc = lead(rows, (rowb,), F16)
    if "v_rows" in p:
        vc = lead(p["v_rows"], (rowb,), cdt)
    # the scales
    ks = vs = None
    if fmt != E4M3 or "scale_dtype" in p:
        sD = g("scale_D", D)
        srows = g("s_rows", rows)
        if fp4:
            ks = vs = lead(srows, (sD // 32,), g("scale_dtype", U8))
        else:
            ks = vs = lead(srows, (), g("scale_dtype", F32), 1.0)
        sk = g("scale")
        if sk == "misaligned":
            ks = vs = lead(srows, (sD // 32 + 2,), U8)[..., 1:sD // 32 + 1]
        elif sk == "rank":
            ks = vs = ks[0]
        elif sk == "grad":
            ks = lead(srows, (), F32, 1.0).requires_grad_(True)
        elif sk == "list":
            ks = [1.0]
        elif sk == "k_only":
            vs = None
        elif sk == "none":
            ks = vs = None
    sl = {None: lambda: z(B, dtype=I32), "int64": lambda: z(B, dtype=torch.int64), "len": lambda: z(3, dtype=I32),
          "2d": lambda: z(1, B, dtype=I32), "noncontig": lambda: z(2 * B, dtype=I32)[::2], "cpu": lambda: z(B, dtype=I32, d="cpu"),
          "list": lambda: [0] * B}[g("sl")]()
    bt0 = torch.arange(4, dtype=I32, device=dev).view(B, 2)
    bt = {None: lambda: bt0, "int64": lambda: bt0.long(), "rank": lambda: bt0[0], "rows": lambda: bt0[:1], "nopages": lambda: bt0[:, :0],
          "stride": lambda: z(B, 4, dtype=I32)[:, ::2], "cpu": lambda: bt0.cpu(), "list": lambda: [[0, 1], [2, 3]],
          "none": lambda: None}[g("bt")]()
    cu0 = torch.tensor([0, 1, 5], dtype=I32, device=dev)
    cu = {None: lambda: cu0, "int64": lambda: cu0.long(), "2d": lambda: cu0[None], "one": lambda: cu0[:1],
          "noncontig": lambda: z(6, dtype=I32)[::2], "cpu": lambda: cu0.cpu(), "none": lambda: None}[g("cu")]()
    kn0 = z(5, hk, D) if packed else z(B, hk, 1, D)
    nk = g("knew")
    kn = vn = {None: lambda: None, "ok": lambda: kn0, "alone": lambda: kn0, "rank": lambda: kn0[0],
               "heads": lambda: z(5, 4, D) if packed else z(B, 4, 1, D), "dtype": lambda: kn0.float(), "cpu": lambda: kn0.cpu(),
               "grad": lambda: kn0.requires_grad_(True)}[nk]()
    if nk == "alone":
        vn = None
    kw = {"q": q, "k_cache": kc, "v_cache": vc, "cache_seqlens": sl, "k_new": kn, "v_new": vn}
    if paged or ext:
        kw["block_table"] = bt if paged else None
    if packed:
        kw["cu_seqlens_q"] = cu
        out = {None: lambda: None, "list": lambda: [0.0], "shape": lambda: z(5, H, 2 * D), "dtype": lambda: z(5, H, D, dtype=BF16),
               "cpu": lambda: z(5, H, D, d="cpu"), "grad": lambda: z(5, H, D).requires_grad_(True),
               "misaligned": lambda: z(5, H, D + 8)[..., 1:D + 1]}[g("out")]()
        kw["out"] = out
    if mod == "qs":
        kw.update(k_scale=ks, v_scale=vs, softcap=g("softcap", 30.0),
                  k_descale=_vec(dev, p["kd"], hk) if "kd" in p else None, v_descale=_vec(dev, p["vd"], hk) if "vd" in p else None)
        if ext:
            kw["format"] = g("format", fmt)
    else:
        kw.update(k_scale=ks, v_scale=vs, sinks=_vec(dev, p["sinks"], H) if "sinks" in p else None)
    if ext:
        kw.update(window_left=g("wl", -1), window_right=g("wr", -1), softmax_scale=g("softmax_scale", 0.0))
    else:
        for name in ("window", "is_causal", "softmax_scale"):
            if name in p:
                kw["window_size" if name == "window" else name] = p[name]
    return kw


def make_mla(dev, ext, **p):
    """The keyword arguments of one MLA call: B 2, H 4, S_q 1, two pages of 64 rows per sequence."""
    g = p.get
    z = lambda *s, dtype=F16, d=dev: torch.zeros(*s, dtype=dtype, device=d)
    D, page, n = g("D", 576), g("rows", 64), g("n", 4)
    q = z(B, H, 1, D, dtype=g("q_dtype", F16))
    q = {None: lambda: q, "rank": lambda: q[0], "empty": lambda: q[:, :0], "cpu": lambda: q.cpu(), "none": lambda: None,
         "grad": lambda: q.requires_grad_(True)}[g("q")]()
    kD = g("cache_D", 576)
    kv = {None: lambda: z(n, page, kD), "rank": lambda: z(n, 1, page, kD), "dtype": lambda: z(n, page, kD, dtype=BF16),
          "rowstride": lambda: z(n, page, kD + 4)[..., :kD], "dim_stride": lambda: z(n, kD, page).transpose(1, 2),
          "grad": lambda: z(n, page, kD).requires_grad_(True), "misaligned": lambda: z(n, page, kD + 8)[..., 4:kD + 4],
          "cpu": lambda: z(n, page, kD, d="cpu"), "many": lambda: z(1, page, kD).expand(2 ** 31, page, kD),
          "list": lambda: [0.0]}[g("kv")]()
    sl = {None: lambda: z(B, dtype=I32), "int64": lambda: z(B, dtype=torch.int64), "len": lambda: z(3, dtype=I32),
          "noncontig": lambda: z(2 * B, dtype=I32)[::2], "cpu": lambda: z(B, dtype=I32, d="cpu")}[g("sl")]()
    bt0 = torch.arange(4, dtype=I32, device=dev).view(B, 2)
    bt = {None: lambda: bt0, "int64": lambda: bt0.long(), "rank": lambda: bt0[0], "rows": lambda: bt0[:1],
          "stride": lambda: z(B, 4, dtype=I32)[:, ::2], "cpu": lambda: bt0.cpu()}[g("bt")]()
    kvn = {None: lambda: None, "shape": lambda: z(B, 2, 576), "dtype": lambda: z(B, 1, 576, dtype=BF16), "list": lambda: [0.0],
           "grad": lambda: z(B, 1, 576).requires_grad_(True)}[g("kvnew")]()
    out = {None: lambda: None, "shape": lambda: z(B, H, 1, 576), "dtype": lambda: z(B, H, 1, 512, dtype=BF16),
           "stride": lambda: z(B, H, 1, 1024)[..., ::2], "grad": lambda: z(B, H, 1, 512).requires_grad_(True),
           "overlap": lambda: z(1, H, 1, 512).expand(B, H, 1, 512), "misaligned": lambda: z(B, H, 1, 520)[..., 4:516]}[g("out")]()
    kw = {"q": q, "kv_cache": kv, "cache_seqlens": sl, "block_table": bt, "kv_new": kvn, "out": out}
    if ext:
        kw.update(is_causal=False, softmax_scale=g("softmax_scale", 0.0))
    elif "softmax_scale" in p:
        kw["softmax_scale"] = p["softmax_scale"]
    return kw


def _table(T, unbuilt, prefix, fn, build, faults, pairs=True):
    """the cases of one function: one per fault of its ordered list, and one per pair of neighbours"""
    def case(name, props):
        T.append(("%s/%s" % (prefix, name), (lambda: fn(**build(**props)))))
    for i, (name, props) in enumerate(faults):
        case(name, props)
        if not pairs or i + 1 == len(faults) or name == "ok":
            continue
        nxt, nprops = faults[i + 1]
        if nxt == "ok":
            continue
        clash = sorted(set(props) & set(nprops))
        why = NO_PAIR.get((prefix, name, nxt)) or NO_PAIR.get(("*", name, nxt))
        if clash or why:
            assert why or all(c in SAME_PROPERTY for c in clash), (prefix, name, nxt, clash)
            unbuilt.append(("%s/%s+%s" % (prefix, name, nxt), why or "; ".join(SAME_PROPERTY[c] for c in clash)))
        else:
            case("%s+%s" % (name, nxt), dict(props, **nprops))


def _modules():
    import fp4_kvcache as F
    import fp4_ragged_kvcache as FR
    import fp8_token_kvcache as T
    import quant_softcap_kvcache as Q
    import mla_kvcache as M
    return F, FR, T, Q, M


def _functions():
    """{(mod, geom, ext): (table prefix, function)}"""
    F, FR, T, Q, M = _modules()
    return {
        ("fp4", "padded", False): ("F.flash_attention_kvcache_fp4", F.flash_attention_kvcache_fp4),
        ("fp4", "paged", False): ("F.flash_attention_kvcache_fp4_paged", F.flash_attention_kvcache_fp4_paged),
        ("fp4", "packed", False): ("FR.flash_attention_kvcache_fp4_ragged", FR.flash_attention_kvcache_fp4_ragged),
        ("tok", "padded", False): ("T.flash_attention_kvcache_fp8_token", T.flash_attention_kvcache_fp8_token),
        ("tok", "paged", False): ("T.flash_attention_kvcache_fp8_token_paged", T.flash_attention_kvcache_fp8_token_paged),
        ("tok", "packed", False): ("T.flash_attention_kvcache_fp8_token_ragged", T.flash_attention_kvcache_fp8_token_ragged),
        ("qs", "padded", False): ("Q.flash_attention_kvcache_quant_softcap", Q.flash_attention_kvcache_quant_softcap),
        ("qs", "paged", False): ("Q.flash_attention_kvcache_quant_softcap_paged", Q.flash_attention_kvcache_quant_softcap_paged),
        ("qs", "packed", False): ("Q.flash_attention_kvcache_quant_softcap_ragged", Q.flash_attention_kvcache_quant_softcap_ragged),
        ("fp4", "padded", True): ("ext.kvcache_fp4_forward[padded]", F._ext.kvcache_fp4_forward),
        ("fp4", "paged", True): ("ext.kvcache_fp4_forward[paged]", F._ext.kvcache_fp4_forward),
        ("fp4", "packed", True): ("ext.kvcache_fp4_ragged_forward", F._ext.kvcache_fp4_ragged_forward),
        ("tok", "padded", True): ("ext.kvcache_fp8_token_forward[padded]", T._ext.kvcache_fp8_token_forward),
        ("tok", "paged", True): ("ext.kvcache_fp8_token_forward[paged]", T._ext.kvcache_fp8_token_forward),
        ("tok", "packed", True): ("ext.kvcache_fp8_token_ragged_forward", T._ext.kvcache_fp8_token_ragged_forward),
        ("qs", "padded", True): ("ext.kvcache_quant_softcap_forward[padded]", Q._ext.kvcache_quant_softcap_forward),
        ("qs", "paged", True): ("ext.kvcache_quant_softcap_forward[paged]", Q._ext.kvcache_quant_softcap_forward),
        ("qs", "packed", True): ("ext.kvcache_quant_softcap_ragged_forward", Q._ext.kvcache_quant_softcap_ragged_forward),
    }


def signatures():
    F, FR, T, Q, M = _modules()
    fns = (F._ext.kvcache_fp4_forward, F._ext.kvcache_fp4_ragged_forward, T._ext.kvcache_fp8_token_forward,
           T._ext.kvcache_fp8_token_ragged_forward, Q._ext.kvcache_quant_softcap_forward,
           Q._ext.kvcache_quant_softcap_ragged_forward, M._ext.kvcache_mla_forward)
    return {f.__name__: f.__doc__.splitlines()[0] for f in fns}


def _formats(mod):
    return {"fp4": (MXFP4,), "tok": (TOKEN,), "qs": (E4M3, TOKEN, MXFP4)}[mod]


# ---- the ordered checks of the bindings (csrc/torch_binding_fp4.cpp, _fp8_token.cpp, _quant_softcap.cpp) ----------------------
def ext_front(mod, fmt, geom):
    """in front of the first is_cuda check: reachable with CPU tensors"""
    packed, fp4, tok, e4m3, qs = geom == "packed", fmt == MXFP4, fmt == TOKEN, fmt == E4M3, mod == "qs"
    f = []
    if qs:
        f += [("format", {"format": 3})]
    f += [("rank_q", {"q": "rank"}), ("rank_k", {"cache": "rank"})]
    if not qs:
        f += [("rank_scale", {"scale": "rank"})]
    if packed:
        f += [("q_empty", {"q": "empty"})]
    if qs:
        f += [("scale_k_only", {"scale": "k_only"})] if not e4m3 else [("scales_given", {"scale_dtype": F32})]
        if not e4m3:
            f += [("descale_given", {"kd": "ok"})]
    f += [("cache_dtype", {"cache_dtype": torch.int8 if fp4 else F16})]
    if qs and fp4:
        f += [("rank_scale", {"scale": "rank"})]
    if tok:
        f += [("scale_dtype", {"scale_dtype": torch.float64})]
        if qs:
            f += [("rank_scale", {"scale": "rank"})]
    f += [("head_dim", {"D": 96}), ("kv_shape", {"v_rows": 32}), ("cache_row", {"cache_D": 128})]
    if not e4m3:
        f += [("scale_shape", {"s_rows": 32})]
    if fp4:
        f += [("scale_row", {"scale_D": 128})]
    f += [("group", {"hk": 3}), ("group_zero", {"hk": 0}), ("knew_alone", {"knew": "alone"}), ("window_left", {"wl": -2}),
          ("window_big", {"wr": 2 ** 31})]
    if qs:
        f += [("softcap_zero", {"softcap": 0.0}), ("softcap_nan", {"softcap": NAN})]
    return f + [("ok", {})]


def ext_behind(mod, fmt, geom):
    """behind it, on device tensors; every one refused before anything is allocated or launched"""
    packed, paged, fp4, tok, e4m3, qs = geom == "packed", geom != "padded", fmt == MXFP4, fmt == TOKEN, fmt == E4M3, mod == "qs"
    f = [("cpu_seqlens", {"sl": "cpu"}), ("q_f32", {"q_dtype": F32})]
    if packed:
        f += [("cu_int64", {"cu": "int64"}), ("cu_2d", {"cu": "2d"}), ("cu_one", {"cu": "one"}), ("cu_noncontig", {"cu": "noncontig"})]
    f += [("seqlens_int64", {"sl": "int64"}), ("seqlens_len", {"sl": "len"}), ("seqlens_2d", {"sl": "2d"}),
          ("seqlens_noncontig", {"sl": "noncontig"})]
    if paged:
        f += [("page_48", {"rows": 48}), ("page_16", {"rows": 16}), ("table_int64", {"bt": "int64"}), ("table_rank", {"bt": "rank"}),
              ("table_rows", {"bt": "rows"}), ("table_no_pages", {"bt": "nopages"}), ("table_stride", {"bt": "stride"}),
              ("too_many_pages", {"n": 2 ** 31})]
    else:
        f += [("batch", {"n": 3}), ("s_cache_big", {"rows": 2 ** 31})]
    f += [("grad_q", {"q": "grad"})]
    if qs and not fp4:
        f += [("grad_k", {"cache": "grad"})]
    if not qs:
        f += [("sinks_f64", {"sinks": "f64"}), ("sinks_shape", {"sinks": "shape"}), ("sinks_2d", {"sinks": "2d"}),
              ("sinks_noncontig", {"sinks": "noncontig"}), ("sinks_grad", {"sinks": "grad"}), ("sinks_cpu", {"sinks": "cpu"})]
    elif e4m3:
        for a in ("kd", "vd"):
            f += [("%s_%s" % (a, k), {a: k}) for k in ("f64", "shape", "shape_3B", "noncontig", "grad", "cpu")]
    f += [("cache_misaligned", {"cache": "misaligned"}), ("cache_rowstride", {"cache": "rowstride"})]
    if fp4:
        f += [("scale_misaligned", {"scale": "misaligned"})]
    if tok:
        f += [("scale_grad", {"scale": "grad"})]
    f += [("knew_rank", {"knew": "rank"}), ("knew_heads", {"knew": "heads"}), ("knew_dtype", {"knew": "dtype"}),
          ("knew_cpu", {"knew": "cpu"}), ("knew_grad", {"knew": "grad"})]
    if packed:
        f += [("out_shape", {"out": "shape"}), ("out_dtype", {"out": "dtype"}), ("out_cpu", {"out": "cpu"}),
              ("out_grad", {"out": "grad"}), ("out_misaligned", {"out": "misaligned"})]
    return f


# ---- the ordered checks of the Python wrappers ---------------------------------------------------------------------------------
def wrapper_checks(mod, fmt, geom):
    """(in front of the wrapper's or the binding's first device check, behind it)"""
    packed, paged, fp4, tok, e4m3, qs = geom == "packed", geom != "padded", fmt == MXFP4, fmt == TOKEN, fmt == E4M3, mod == "qs"
    window = [("window", {"window": (-2, -1)}), ("causal_window", {"is_causal": True, "window": (-1, 3)})]
    scale_new = [("scale_neg", {"softmax_scale": -1.0}), ("scale_inf", {"softmax_scale": INF}), ("scale_nan", {"softmax_scale": NAN}),
                 ("knew_alone", {"knew": "alone"})]
    cap = [("softcap_str", {"softcap": "30"}), ("softcap_bool", {"softcap": True}), ("softcap_zero", {"softcap": 0.0}),
           ("softcap_inf", {"softcap": INF})] if qs else []
    if fp4:      # fp4_kvcache._check_formats, then the head dim
        formats = [("cache_dtype", {"cache_dtype": F16}), ("v_dtype", {"cache": "v_dtype"}), ("scale_dtype", {"scale_dtype": I32}),
                   ("head_dim", {"D": 96})]
    elif tok:    # fp8_token_kvcache._check_formats
        formats = ([("cache_list", {"cache": "list"}), ("scale_list", {"scale": "list"})] if not qs else []) + [
            ("rank_k", {"cache": "rank"}), ("kv_shape", {"v_rows": 32}), ("scale_shape", {"s_rows": 32}), ("head_dim", {"D": 96})]
        if not qs:
            formats[2:2] = [("cache_dtype", {"cache_dtype": F16}), ("scale_dtype", {"scale_dtype": torch.float64})]
    else:
        formats = [("rank_k", {"cache": "rank"}), ("kv_shape", {"v_rows": 32}), ("head_dim", {"D": 96}), ("kd_int", {"kd": "int"}),
                   ("vd_list", {"vd": "list"})]
    if qs:       # quant_softcap_kvcache._format in front of the format's own checks
        formats = [("cache_list", {"cache": "list"}), ("scale_k_only", {"scale": "k_only"} if not e4m3 else {"scale_dtype": F32, "scale": "k_only"}),
                   ("scales_and_descales", {"kd": "ok"} if not e4m3 else {"scale_dtype": F32, "kd": "ok"})] + (
                       [("scale_list", {"scale": "list"})] if not e4m3 else []) + formats + [("no_format", {"cache_dtype": F16})]
    grads = [("grad_q", {"q": "grad"})]
    if qs and not fp4:
        grads += [("grad_k", {"cache": "grad"})]
    if tok:
        grads += [("grad_scale", {"scale": "grad"})]
    grads += [("grad_knew", {"knew": "grad"})]
    if not qs:
        grads += [("grad_sinks", {"sinks": "grad"})]
    through = [("kv_shape", {"v_rows": 32})] if fp4 else []          # the binding's own, through the wrapper
    through += [("group", {"hk": 3})]
    behind = [("cpu_seqlens", {"sl": "cpu"}), ("q_f32", {"q_dtype": F32}), ("seqlens_int64", {"sl": "int64"})]
    behind += [("table_rows", {"bt": "rows"})] if geom == "paged" else []
    behind += ([("sinks_f64", {"sinks": "f64"})] if not qs else [("kd_shape", {"kd": "shape"})] if e4m3 else [])
    behind += [("cache_misaligned", {"cache": "misaligned"}), ("knew_dtype", {"knew": "dtype"})]
    if packed:
        behind += [("out_cpu", {"out": "cpu"}), ("out_misaligned", {"out": "misaligned"})]
        head = window
        if fp4 and not qs:
            head = head + [("scale_list", {"scale": "list"})]
        head = head + [("q_none", {"q": "none"}), ("cu_int64", {"cu": "int64"}), ("cu_2d", {"cu": "2d"}), ("cu_one", {"cu": "one"}),
                       ("table_int64", {"bt": "int64"}), ("table_rows", {"bt": "rows"}), ("seqlens_len", {"sl": "len"}),
                       ("rank_q", {"q": "rank"})]
        front = head + cap + formats + [("page_48", {"rows": 48})] + scale_new + [
            ("out_list", {"out": "list"}), ("out_shape", {"out": "shape"}), ("out_dtype", {"out": "dtype"})] + grads + [
            ("grad_out", {"out": "grad"}), ("ok", {})]
        return front, [("cpu_cu", {"cu": "cpu"}), ("cpu_table", {"bt": "cpu"})] + through + behind
    if fp4 and not qs:
        body = window + [("q_none", {"q": "none"}), ("sl_list", {"sl": "list"})] + formats[:-1] + [
            ("rank_q", {"q": "rank"}), formats[-1]] + scale_new + grads
    else:
        body = window + [("sl_list", {"sl": "list"}), ("q_none", {"q": "none"}), ("rank_q", {"q": "rank"})] + cap + formats + scale_new + grads
    if not paged:
        return body + through + [("ok", {})], behind
    table = [("table_list", {"bt": "list"}), ("table_int64", {"bt": "int64"}), ("table_rank", {"bt": "rank"})]
    if fp4 and not qs:     # block_table, its device, the page size
        return table + [("ok", {})], [("cpu_table", {"bt": "cpu"}), ("page_48", {"rows": 48})] + body + through + behind
    return (table + [("cache_list", {"cache": "list"}), ("rank_k", {"cache": "rank"}), ("page_48", {"rows": 48}), ("page_16", {"rows": 16}),
                     ("ok", {})], [("cpu_table", {"bt": "cpu"})] + body + through + behind)


# ---- MLA (csrc/torch_binding_mla.cpp, mla_kvcache.py): its own geometry and its own order, device checks last --------------------
MLA_EXT_FRONT = [
    ("rank_q", {"q": "rank"}), ("q_dim", {"D": 512}), ("rank_kv", {"kv": "rank"}), ("kv_dim", {"cache_D": 512}),
    ("q_f32", {"q_dtype": F32}), ("kv_dtype", {"kv": "dtype"}), ("q_empty", {"q": "empty"}), ("page_48", {"rows": 48}),
    ("page_16", {"rows": 16}), ("seqlens_int64", {"sl": "int64"}), ("seqlens_len", {"sl": "len"}), ("seqlens_noncontig", {"sl": "noncontig"}),
    ("table_int64", {"bt": "int64"}), ("table_rank", {"bt": "rank"}), ("table_rows", {"bt": "rows"}), ("table_stride", {"bt": "stride"}),
    ("kv_rowstride", {"kv": "rowstride"}), ("kv_dim_stride", {"kv": "dim_stride"}), ("kvnew_shape", {"kvnew": "shape"}),
    ("kvnew_dtype", {"kvnew": "dtype"}), ("kvnew_grad", {"kvnew": "grad"}), ("out_shape", {"out": "shape"}), ("out_dtype", {"out": "dtype"}),
    ("out_stride", {"out": "stride"}), ("out_overlap", {"out": "overlap"}), ("out_grad", {"out": "grad"}), ("grad_q", {"q": "grad"}),
    ("grad_kv", {"kv": "grad"}), ("ok", {})]
MLA_EXT_BEHIND = [("cpu_seqlens", {"sl": "cpu"}), ("cpu_table", {"bt": "cpu"}), ("kv_misaligned", {"kv": "misaligned"}),
                  ("out_misaligned", {"out": "misaligned"}), ("too_many_pages", {"kv": "many"})]
MLA_WRAPPER_FRONT = [("q_none", {"q": "none"}), ("kv_list", {"kv": "list"}), ("kvnew_list", {"kvnew": "list"}),
                     ("table_int64", {"bt": "int64"}), ("seqlens_int64", {"sl": "int64"}), ("ok", {})]
MLA_WRAPPER_BEHIND = [("cpu_seqlens", {"sl": "cpu"}), ("cpu_table", {"bt": "cpu"}), ("scale_neg", {"softmax_scale": -1.0}),
                      ("scale_nan", {"softmax_scale": NAN}), ("grad_q", {"q": "grad"}), ("grad_kv", {"kv": "grad"}),
                      ("grad_kvnew", {"kvnew": "grad"}), ("grad_out", {"out": "grad"})]


def _cases(dev, half):
    """(cases, unbuilt pairs) of one half: 0 the checks in front of the first device check, 1 those behind it"""
    _, _, _, _, M = _modules()
    T, unbuilt = [], []
    for (mod, geom, ext), (prefix, fn) in _functions().items():
        for fmt in _formats(mod):
            name = prefix + ("{%s}" % FMT_NAMES[fmt] if mod == "qs" else "")
            faults = (ext_front, ext_behind)[half](mod, fmt, geom) if ext else wrapper_checks(mod, fmt, geom)[half]
            _table(T, unbuilt, name, fn, (lambda mod=mod, fmt=fmt, geom=geom, ext=ext, **p: make(dev, mod, fmt, geom, ext, **p)), faults)
    mla_ext, mla_wrap = (MLA_EXT_FRONT, MLA_WRAPPER_FRONT) if half == 0 else (
        MLA_EXT_BEHIND, MLA_WRAPPER_BEHIND + [f for f in MLA_EXT_FRONT if f[0] not in ("ok", "grad_q", "grad_kv")] + MLA_EXT_BEHIND[2:])
    _table(T, unbuilt, "ext.kvcache_mla_forward", M._ext.kvcache_mla_forward, (lambda **p: make_mla(dev, True, **p)), mla_ext)
    _table(T, unbuilt, "M.flash_attention_mla_kvcache", M.flash_attention_mla_kvcache, (lambda **p: make_mla(dev, False, **p)), mla_wrap)
    assert len(dict(T)) == len(T), "duplicate case ids"
    return T, unbuilt


def cpu_cases():
    return _cases("cpu", 0)[0]


def gpu_cases(dev="cuda"):
    return _cases(dev, 1)[0]


def unbuilt_pairs():
    """[(case id, reason)]: the neighbouring checks no one call can violate together"""
    return _cases("cpu", 0)[1] + _cases("cpu", 1)[1]


def outcome(thunk):
    """[exception type, message] of a call that must be refused; a call that returns is recorded as such"""
    try:
        thunk()
    except Exception as e:      # the type and the text are the surface
        return [type(e).__name__, str(e)]
    return ["returned", ""]


def errors(cases):
    return {cid: outcome(thunk) for cid, thunk in cases}


def load(path=None):
    """The fixture as {"signatures": {...}, "cpu": {case id: [type, message]}, "gpu": {...}}.  On disk the few hundred distinct
    outcomes stand once, in "outcomes", and a half holds one line per table: {case name: index into "outcomes"}."""
    with open(path or os.path.join(GOLDEN, FIXTURE)) as fh:
        raw = json.load(fh)
    halves = {h: {"%s/%s" % (t, n): raw["outcomes"][i] for t, rows in raw[h].items() for n, i in rows.items()} for h in ("cpu", "gpu")}
    return dict(halves, signatures=raw["signatures"])


def dump(got, path):
    outcomes = sorted({tuple(v) for h in ("cpu", "gpu") for v in got[h].values()})
    index = {o: i for i, o in enumerate(outcomes)}
    lines = lambda items: ",\n".join(" " + x for x in items)
    text = '{\n"signatures": {\n%s\n},\n"outcomes": [\n%s\n]' % (
        lines("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(got["signatures"].items())),
        lines(json.dumps(list(o)) for o in outcomes))
    for h in ("cpu", "gpu"):
        tables = {}
        for cid, v in got[h].items():       # the tables' own order of cases: the order of the checks
            t, n = cid.rsplit("/", 1)
            tables.setdefault(t, {})[n] = index[tuple(v)]
        text += ',\n"%s": {\n%s\n}' % (h, lines("%s: %s" % (json.dumps(t), json.dumps(r)) for t, r in sorted(tables.items())))
    with open(path, "w") as fh:
        fh.write(text + "\n}\n")


def main(argv):
    out = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN     # another directory: leave the fixture alone
    old = load() if os.path.exists(os.path.join(GOLDEN, FIXTURE)) else {}
    # the GPU table is recorded where there is a GPU; elsewhere the committed one is kept
    got = {"signatures": signatures(), "cpu": errors(cpu_cases()),
           "gpu": errors(gpu_cases()) if torch.cuda.is_available() else old.get("gpu", {})}
    if "--check" in argv:
        same = old == got
        print("fixture matches this tree" if same else "differs: %s" % FIXTURE)
        if not same:
            for half in ("signatures", "cpu", "gpu"):
                for cid in sorted(set(got[half]) | set(old.get(half, {}))):
                    if got[half].get(cid) != old.get(half, {}).get(cid):
                        print("  %s %s: %r, recorded %r" % (half, cid, got[half].get(cid), old.get(half, {}).get(cid)))
        return 0 if same else 1
    dump(got, os.path.join(out, FIXTURE))
    print("wrote %s (%d cpu cases, %d gpu cases)" % (os.path.join(os.path.relpath(out, ROOT), FIXTURE), len(got["cpu"]), len(got["gpu"])))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
