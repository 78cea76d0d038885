"""The MLA decode family's host surface, pinned (tests/golden/mla_errors.json), in the manner of tests/quant_surface.py, whose
make_mla, _table, outcome, errors and fixture format it uses:

"c"    the refusals of the ten C entry points fa_fwd_kvcache_mla{,_ragged,_fp8,_sparse,_sparse_fp8}{,_workspace_bytes}, called
       through ctypes with host pointers: per function the ORDERED list of its checks, one fault per check, and for neighbours a
       and b the case "a+b" that commits both, so that the fixture fixes the order.  An outcome is [return code, fa_last_error()].
"cpu"  the refusals of the four binding functions and Python wrappers that tests/golden/quant_errors.json does not hold (packed,
       FP8, sparse, sparse FP8; the dense pair stays there), on CPU tensors: the checks in front of the first device check, and,
       with tests/test_host_mla.py's OnDevice, the wrappers' checks behind theirs.
"gpu"  the checks behind the device checks, on device tensors: every call refused before anything is allocated or launched.
"signatures"  the four pybind signature lines.

No C case can reach a launch: every call is made with fa_debug_kvcache_splits(3) and a 16-byte workspace, so that a call no
other check refuses is refused by the workspace check, the last one ("backstop").  The workspace functions are also recorded
under the two other settings that matter: 0 (the formula) and 1 (no workspace).

    python tests/mla_surface.py            # rewrite (the device half where there is a GPU; elsewhere the committed one is kept)
    python tests/mla_surface.py --check    # compare only (exit 1 on a difference)
    python tests/mla_surface.py --out DIR  # write it somewhere else

tests/test_host_mla_surface.py and tests/test_gpu_mla_errors.py replay the fixture.  It was recorded from the tree of the commit
it names, before the five entry-point files, bindings and wrappers were folded onto their shared helpers."""
import ctypes
import os
import subprocess
import sys

import torch

import quant_surface as qs
from quant_surface import F16, F32, GOLDEN, INF, NAN, ROOT, _table, errors, make_mla, outcome  # noqa: F401  (outcome: the tests')

FIXTURE = "mla_errors.json"
HALVES = ("c", "cpu", "gpu")
KINDS = ("ragged", "fp8", "sparse", "sparse_fp8")     # the four pairs recorded here
C_KINDS = ("dense",) + KINDS

# ---- the C entry points ---------------------------------------------------------------------------------------------------------
qs.SAME_PROPERTY.update({k: "%s is one argument" % k for k in (
    "new", "o", "lse", "ws", "wsb", "B", "H", "Sq", "Tq", "topk", "pages", "page", "mp", "bts", "Snew", "has_new", "dtype", "sc",
    "causal", "qs", "ks", "os", "is_", "cu", "forced")})
_DENSE = ("q", "kv", "new", "sl", "bt", "o", "lse", "ws", "wsb", "B", "H", "Sq", "pages", "page", "mp", "bts", "Snew", "dtype", "sc",
          "causal", "qs", "ks", "os")
_SPARSE = _DENSE[:3] + ("idx",) + _DENSE[3:12] + ("topk",) + _DENSE[12:] + ("is_",)
_RAGGED = ("q", "kv", "new", "cu", "sl", "bt", "o", "lse", "ws", "wsb", "Tq", "B", "H", "pages", "page", "mp", "bts", "has_new", "dtype",
           "sc", "causal", "qs", "ks", "os")
C_ARGS = {"dense": _DENSE, "fp8": _DENSE, "sparse": _SPARSE, "sparse_fp8": _SPARSE, "ragged": _RAGGED}
C_WS_ARGS = {"dense": ("B", "H", "Sq", "mp", "page", "Snew"), "fp8": ("B", "H", "Sq", "mp", "page", "Snew"),
             "sparse": ("B", "H", "Sq", "topk", "mp", "page", "Snew"), "sparse_fp8": ("B", "H", "Sq", "topk", "mp", "page", "Snew"),
             "ragged": ("Tq", "B", "H", "mp", "page")}
C_NAME = {k: "fa_fwd_kvcache_mla" + ("" if k == "dense" else "_" + k) for k in C_KINDS}
_POINTERS = ("q", "kv", "new", "idx", "cu", "sl", "bt", "o", "lse", "ws")
_BUF = (ctypes.c_char * 4096)()
_P = (ctypes.addressof(_BUF) + 15) & ~15        # a 16-byte aligned host address: no case may reach a launch


def _c_defaults():
    return dict(q=0, kv=0, new=None, idx=0, cu=0, sl=0, bt=0, o=0, lse=0, ws=0, wsb=16, B=2, H=16, Sq=1, Tq=5, topk=64, pages=8, page=64,
                mp=4, bts=4, Snew=0, has_new=0, dtype=1, sc=576 ** -0.5, causal=1, qs=None, ks=None, os=None, is_=None)


def _c_call(kind, workspace_fn, forced=3, **faults):
    """[return code, fa_last_error()] of one call; a pointer property is its offset from the aligned address (None: NULL), a
    stride property a tuple"""
    import _mi355fa as fa
    a = dict(_c_defaults(), **faults)
    for k in _POINTERS:
        a[k] = None if a[k] is None else _P + a[k]
    keep = []
    for k in ("qs", "ks", "os", "is_"):
        if a[k] is not None:
            keep.append((ctypes.c_longlong * len(a[k]))(*a[k]))
            a[k] = keep[-1]
    force = fa.lib.fa_debug_kvcache_splits
    force.argtypes, force.restype = [ctypes.c_int], None
    force(forced)
    try:
        if workspace_fn:
            rc = getattr(fa.lib, C_NAME[kind] + "_workspace_bytes")(*(a[k] for k in C_WS_ARGS[kind]))
        else:
            rc = getattr(fa.lib, C_NAME[kind])(*(a[k] for k in C_ARGS[kind]), None)
        text = fa.lib.fa_last_error().decode() if rc < 0 else ""
    finally:
        force(0)
    assert workspace_fn or rc < 0, (kind, faults, rc)     # refused, every one: a call that returned has launched
    return [str(rc), text]


def c_shape_faults(kind):
    """the checks the call and its workspace function share, in their order"""
    sparse, ragged = kind.startswith("sparse"), kind == "ragged"
    if ragged:
        f = [("Tq_zero", {"Tq": 0}), ("B_zero", {"B": 0}), ("H_zero", {"H": 0}), ("rows_big", {"H": 1 << 20, "Tq": 32}),
             ("B_big", {"B": (1 << 24) + 1})]
    else:
        f = [("B_zero", {"B": 0}), ("H_zero", {"H": 0}), ("Sq_zero", {"Sq": 0}), ("Snew_neg", {"Snew": -1})]
        if sparse:
            f += [("topk_zero", {"topk": 0}), ("topk_big", {"topk": (1 << 24) + 1})]
        f += [("rows_big", {"H": 1 << 20, "Sq": 32})]
    f += [("page_48", {"page": 48}), ("page_0", {"page": 0}), ("mp_zero", {"mp": 0, "bts": 0}), ("reach", {"mp": 1 << 26, "bts": 1 << 26})]
    # too many workgroups or rows: a packed step's 2^24 row blocks times 2^10 forced splits; elsewhere B * H * S_q * 512 > 2^40
    f += [("launch_big", {"Tq": 1 << 23, "B": 1 << 24, "H": 2, "forced": 1 << 10} if ragged else {"B": 2 ** 31 - 1})]
    return f


def c_faults(kind):
    """the ordered checks of fa_fwd_kvcache_mla* itself"""
    sparse, ragged, fp8 = kind.startswith("sparse"), kind == "ragged", kind.endswith("fp8")
    f = [("null_q", {"q": None}), ("null_kv", {"kv": None})]
    f += [("null_idx", {"idx": None})] if sparse else [("null_cu", {"cu": None})] if ragged else []
    f += [("null_sl", {"sl": None}), ("null_bt", {"bt": None}), ("null_o", {"o": None})]
    if ragged:
        f += [("has_new_2", {"has_new": 2}), ("has_new_alone", {"has_new": 1}), ("new_alone", {"new": 0})]
    else:
        f += [("Snew_alone", {"Snew": 2}), ("new_alone", {"new": 0})]
    f += [("dtype", {"dtype": 2}), ("causal", {"causal": 2}), ("scale_neg", {"sc": -1.0}), ("scale_zero", {"sc": 0.0}),
          ("scale_inf", {"sc": INF}), ("scale_nan", {"sc": NAN})]
    f += c_shape_faults(kind)
    f += [("pages_zero", {"pages": 0}), ("bts_small", {"bts": 3}), ("bts_big", {"bts": 1 << 31})]
    if ragged:      # {row, head}
        f += [("qs_odd", {"qs": (580, 576)}), ("qs_big", {"qs": (1 << 30, 576)}), ("qs_row", {"qs": (512, 576)}),
              ("os_neg", {"os": (-8, 512)}), ("os_row", {"os": (504, 512)}), ("os_zero", {"os": (8192, 0)})]
    else:           # {batch, head, row}
        f += [("qs_odd", {"qs": (0, 580, 576)}), ("qs_big", {"qs": ((1 << 40) + 8, 576, 576)}), ("qs_row", {"qs": (0, 0, 512)}),
              ("qs_slice", {"qs": (0, 0, 1 << 30), "Sq": 2}), ("os_neg", {"os": (8192, 512, -8)}), ("os_row", {"os": (8192, 512, 504)}),
              ("os_zero_head", {"os": (8192, 0, 512)}), ("os_zero_batch", {"os": (0, 512, 512)})]
    if fp8:         # bytes
        f += [("ks_page", {"ks": (41992, 656)}), ("ks_page_big", {"ks": ((1 << 41) + 16, 656)}), ("ks_row", {"ks": (41984, 664)}),
              ("ks_row_small", {"ks": (41984, 640)}), ("ks_big", {"ks": (0, 1 << 26)})]
    else:           # elements
        f += [("ks_page", {"ks": (36868, 576)}), ("ks_page_big", {"ks": ((1 << 40) + 8, 576)}), ("ks_row", {"ks": (36864, 580)}),
              ("ks_row_small", {"ks": (36864, 568)}), ("ks_big", {"ks": (0, 1 << 25)})]
    if sparse:
        f += [("is_neg", {"is_": (-1, 64)}), ("is_big", {"is_": (64, (1 << 40) + 1)})]
    f += [("align_q", {"q": 8}), ("align_kv", {"kv": 4}), ("align_new", {"new": 2, "has_new": 1} if ragged else {"new": 2, "Snew": 1}),
          ("align_o", {"o": 8}), ("align_ws", {"ws": 8}), ("align_lse", {"lse": 2})]
    f += [("align_idx", {"idx": 2})] if sparse else [("align_cu", {"cu": 2})] if ragged else []
    f += [("align_sl", {"sl": 2}), ("align_bt", {"bt": 1}), ("ws_null", {"ws": None, "wsb": 0}), ("backstop", {})]
    return f


def c_cases():
    T, unbuilt = [], []
    for kind in C_KINDS:
        _table(T, unbuilt, C_NAME[kind], (lambda kind=kind, **p: _c_call(kind, False, **p)), dict, c_faults(kind))
        ws = C_NAME[kind] + "_workspace_bytes"
        _table(T, unbuilt, ws, (lambda kind=kind, **p: _c_call(kind, True, **p)), dict, c_shape_faults(kind))
        for forced in (0, 1, 3):
            T.append(("%s/splits_%d" % (ws, forced), (lambda kind=kind, forced=forced: _c_call(kind, True, forced))))
    assert len(dict(T)) == len(T), "duplicate case ids"
    return T, unbuilt


# ---- the bindings and the wrappers ---------------------------------------------------------------------------------------------
def _kw(kind):
    return dict(pool="fp8" if kind.endswith("fp8") else "16bit", packed=kind == "ragged", sparse=kind.startswith("sparse"))


def _modules():
    import mla_ragged_kvcache as R
    import mla_fp8_kvcache as F
    import mla_sparse_kvcache as S
    import mla_sparse_fp8_kvcache as SF
    return {"ragged": (R, "flash_attention_mla_kvcache_ragged", "kvcache_mla_ragged_forward"),
            "fp8": (F, "flash_attention_mla_kvcache_fp8", "kvcache_mla_fp8_forward"),
            "sparse": (S, "flash_attention_mla_kvcache_sparse", "kvcache_mla_sparse_forward"),
            "sparse_fp8": (SF, "flash_attention_mla_kvcache_sparse_fp8", "kvcache_mla_sparse_fp8_forward")}


def signatures():
    return {ext: getattr(M._ext, ext).__doc__.splitlines()[0] for M, _, ext in _modules().values()}


_SEQLENS = [("seqlens_int64", {"sl": "int64"}), ("seqlens_len", {"sl": "len"}), ("seqlens_noncontig", {"sl": "noncontig"})]
_TABLE = [("table_int64", {"bt": "int64"}), ("table_rank", {"bt": "rank"}), ("table_rows", {"bt": "rows"}), ("table_stride", {"bt": "stride"})]
_CU = [("cu_int64", {"cu": "int64"}), ("cu_2d", {"cu": "2d"}), ("cu_one", {"cu": "one"}), ("cu_noncontig", {"cu": "noncontig"})]
_IDX = [("idx_int64", {"idx": "int64"}), ("idx_rank", {"idx": "rank"}), ("idx_rows", {"idx": "rows"}), ("idx_topk0", {"idx": "topk0"}),
        ("idx_stride", {"idx": "stride"})]


def ext_front(kind):
    """csrc/torch_binding_mla_<kind>.cpp: in front of the is_cuda check, reachable with CPU tensors"""
    fp8, ragged, sparse = kind.endswith("fp8"), kind == "ragged", kind.startswith("sparse")
    f = [("rank_q", {"q": "rank"}), ("q_dim", {"D": 512})]
    kv = [("rank_kv", {"kv": "rank"}), ("kv_dim", {"cache_D": 512})]
    dt = [("q_f32", {"q_dtype": F32}), ("kv_dtype", {"kv": "dtype"})]
    f += dt + kv if fp8 else kv + dt
    f += [("q_empty", {"q": "empty"}), ("page_48", {"rows": 48}), ("page_16", {"rows": 16})]
    f += _IDX if sparse else _CU if ragged else []
    f += _SEQLENS + _TABLE + [("kv_rowstride", {"kv": "rowstride"}), ("kv_dim_stride", {"kv": "dim_stride"}), ("kvnew_shape", {"kvnew": "shape"}),
                              ("kvnew_dtype", {"kvnew": "dtype"}), ("kvnew_grad", {"kvnew": "grad"}), ("out_shape", {"out": "shape"}),
                              ("out_dtype", {"out": "dtype"}), ("out_stride", {"out": "stride"}), ("out_overlap", {"out": "overlap"}),
                              ("out_grad", {"out": "grad"}), ("grad_q", {"q": "grad"})]
    f += [] if fp8 else [("grad_kv", {"kv": "grad"})]       # a uint8 pool cannot require grad
    return f + [("ok", {})]


def ext_behind(kind):
    """behind it, on device tensors; every one refused before anything is allocated or launched"""
    mid = [("cpu_idx", {"idx": "cpu"})] if kind.startswith("sparse") else [("cpu_cu", {"cu": "cpu"})] if kind == "ragged" else []
    return [("cpu_seqlens", {"sl": "cpu"}), ("cpu_table", {"bt": "cpu"})] + mid + [
        ("kv_misaligned", {"kv": "misaligned"}), ("out_misaligned", {"out": "misaligned"}), ("too_many_pages", {"kv": "many"})]


def wrapper_front(kind):
    """mla_<kind>_kvcache.py: in front of its first device check"""
    fp8, ragged, sparse = kind.endswith("fp8"), kind == "ragged", kind.startswith("sparse")
    f = [("q_none", {"q": "none"}), ("kv_list", {"kv": "list"})]
    f += [("idx_list", {"idx": "list"})] if sparse else [("cu_list", {"cu": "list"})] if ragged else []
    f += [("seqlens_list", {"sl": "list"}), ("table_list", {"bt": "list"}), ("kvnew_list", {"kvnew": "list"}), ("out_list", {"out": "list"})]
    f += [("kv_dtype", {"kv": "dtype"})] if fp8 else []
    f += [("idx_int64", {"idx": "int64"})] if sparse else _CU[:3] if ragged else []
    f += [("table_int64", {"bt": "int64"})] + ([("table_rank", {"bt": "rank"}), ("table_rows", {"bt": "rows"})] if ragged else [])
    f += [("seqlens_int64", {"sl": "int64"})] + ([("seqlens_len", {"sl": "len"})] if ragged else [])
    return f + [("ok", {})]


def wrapper_behind(kind):
    """behind it: its device checks (on the GPU), softmax_scale, grad, then the binding's own through the wrapper"""
    fp8 = kind.endswith("fp8")
    mid = [("cpu_idx", {"idx": "cpu"})] if kind.startswith("sparse") else [("cpu_cu", {"cu": "cpu"})] if kind == "ragged" else []
    dev = mid + [("cpu_seqlens", {"sl": "cpu"}), ("cpu_table", {"bt": "cpu"})]
    rest = [("scale_neg", {"softmax_scale": -1.0}), ("scale_zero", {"softmax_scale": 0.0}), ("scale_inf", {"softmax_scale": INF}),
            ("scale_nan", {"softmax_scale": NAN}), ("grad_q", {"q": "grad"})]
    rest += ([] if fp8 else [("grad_kv", {"kv": "grad"})]) + [("grad_kvnew", {"kvnew": "grad"}), ("grad_out", {"out": "grad"})]
    rest += [f for f in ext_front(kind) if f[0] not in ("ok", "grad_q", "grad_kv")]
    return dev, rest


def _cases(dev, half):
    """(cases, unbuilt pairs) of one half: 0 the CPU, 1 the device"""
    from test_host_mla import OnDevice
    T, unbuilt = [], []
    for kind, (M, fn, ext) in _modules().items():
        kw = _kw(kind)
        e, w = getattr(M._ext, ext), getattr(M, fn)
        devchecks, rest = wrapper_behind(kind)
        build = lambda is_ext, wrap=None, kw=kw: (lambda **p: make_mla(dev, is_ext, wrap=wrap, **kw, **p))
        if half == 0:
            _table(T, unbuilt, "ext." + ext, e, build(True), ext_front(kind))
            _table(T, unbuilt, "M." + fn, w, build(False), wrapper_front(kind))
            # the wrapper's checks behind its device checks: reached on the CPU, and ended by the binding's device check ("ok")
            _table(T, unbuilt, "M.%s{OnDevice}" % fn, w, build(False, lambda t: t.as_subclass(OnDevice)), rest + [("ok", {})])
        else:
            _table(T, unbuilt, "ext." + ext, e, build(True), ext_behind(kind))
            _table(T, unbuilt, "M." + fn, w, build(False), devchecks + rest + ext_behind(kind)[len(devchecks):])
    assert len(dict(T)) == len(T), "duplicate case ids"
    return T, unbuilt


def cpu_cases():
    return _cases("cpu", 0)[0]


def gpu_cases(dev="cuda"):
    return _cases(dev, 1)[0]


def unbuilt_pairs():
    return c_cases()[1] + _cases("cpu", 0)[1] + _cases("cpu", 1)[1]


def load():
    return qs.load(os.path.join(GOLDEN, FIXTURE), HALVES, ("signatures", "commit"))


def _commit(old):
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    except Exception:       # no history here (a copied tree): the recorded one stands
        return old.get("commit", "unknown")


def main(argv):
    out = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN
    old = load() if os.path.exists(os.path.join(GOLDEN, FIXTURE)) else {}
    got = {"signatures": signatures(), "c": {cid: thunk() for cid, thunk in c_cases()[0]}, "cpu": errors(cpu_cases()),
           "gpu": errors(gpu_cases()) if torch.cuda.is_available() else old.get("gpu", {})}
    if "--check" in argv:
        same = all(old.get(k) == got[k] for k in got)
        print("fixture matches this tree" if same else "differs: %s" % FIXTURE)
        for half in got:
            for cid in sorted(set(got[half]) | set(old.get(half, {}))):
                if got[half].get(cid) != old.get(half, {}).get(cid):
                    print("  %s %s: %r, recorded %r" % (half, cid, got[half].get(cid), old.get(half, {}).get(cid)))
        return 0 if same else 1
    # the commit is that of the first recording: the device half is added to it from a copy of the same tree
    got["commit"] = old["commit"] if "--keep-commit" in argv and old else _commit(old)
    qs.dump(got, os.path.join(out, FIXTURE), HALVES, ("commit",))
    print("wrote %s (%d c cases, %d cpu cases, %d gpu cases)" % (os.path.join(os.path.relpath(out, ROOT), FIXTURE), len(got["c"]),
                                                                 len(got["cpu"]), len(got["gpu"])))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
