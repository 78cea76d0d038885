#!/usr/bin/env python3
"""Record what the decode entry points of libmi355fa.so answer to bad arguments: (return code, fa_last_error() text) for the
fixed list CASES below, over the ten decode calls and their six workspace functions.  Every case is refused before anything is
launched, so this runs through ctypes on a machine without a GPU.

usage: record_refusals.py [--lib LIB.so] [--commit REV] [--out FILE.json]
Without --out the table is printed.  tests/golden/decode_refusals.json is this tool's output for the library built from
the commit named inside it, the one BEFORE the decode host path was folded; tests/test_host_refusals.py replays CASES against
the in-tree library and compares code and text exactly, so a refactor of the host path cannot change which refusal a call
gets, or -- where a case has two faults -- which of them fires first.  Regenerate the file only from a library built at a
commit whose refusals are the intended ones, never from the code under review.

A case is (id, function, {argument: value}): the named arguments replace the function's defaults (DEFAULTS), which
describe a well-formed call.  Pointers are "P" (a 16-byte aligned host address, never dereferenced), "P+n", or None;
strides a list of three; opts / mods a dict of their members; "splits" forces the split count (1: no workspace needed).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd"))

_HEAD = "q k_cache v_cache k_new v_new cache_seqlens".split()
_OUT = "o lse workspace workspace_bytes".split()
_SHAPE = "B H H_kv S_q S_cache S_new D dtype".split()
_PSHAPE = "B H H_kv S_q num_pages page_size max_pages_per_seq block_table_stride S_new D dtype".split()
_TAIL = "window_left window_right opts stream".split()
_FP4 = "q k_cache v_cache k_scale v_scale k_new v_new cache_seqlens".split()
# the parameters of every function, in the order of its header
PARAMS = {
    "fa_fwd_kvcache": _HEAD + _OUT + _SHAPE + ["scale"] + _TAIL,
    "fa_fwd_kvcache_softcap": _HEAD + _OUT + _SHAPE + ["scale", "softcap"] + _TAIL,
    "fa_fwd_kvcache_alibi": _HEAD + _OUT + _SHAPE + ["scale", "alibi_slopes", "slopes_batch_stride"] + _TAIL,
    "fa_fwd_kvcache_sink": _HEAD + _OUT + _SHAPE + ["scale", "sinks"] + _TAIL,
    "fa_fwd_kvcache_fp8": _HEAD + ["k_descale", "v_descale", "descale_bstride"] + _OUT + _SHAPE + ["kv_dtype", "scale"] + _TAIL,
    "fa_fwd_kvcache_fp8_sink": _HEAD + ["k_descale", "v_descale", "descale_bstride"] + _OUT + _SHAPE +
                               ["kv_dtype", "scale", "sinks"] + _TAIL,
    "fa_fwd_kvcache_paged": _HEAD + ["block_table"] + _OUT + _PSHAPE + ["cache_dtype", "scale"] + _TAIL[:2] + ["mods"] + _TAIL[2:],
    "fa_fwd_kvcache_ragged": _HEAD[:5] + ["cu_seqlens_q", "cache_seqlens", "block_table"] + _OUT +
                             "total_q B H H_kv num_pages page_size max_pages_per_seq block_table_stride D dtype cache_dtype scale".split() +
                             _TAIL[:2] + ["mods"] + _TAIL[2:],
    "fa_fwd_kvcache_fp4": _FP4 + ["k_scale_strides", "v_scale_strides", "sinks"] + _OUT + _SHAPE + ["kv_dtype", "scale"] + _TAIL,
    "fa_fwd_kvcache_fp4_paged": _FP4 + ["block_table", "k_scale_strides", "v_scale_strides", "sinks"] + _OUT + _PSHAPE +
                                ["kv_dtype", "scale"] + _TAIL,
    "fa_fwd_kvcache_workspace_bytes": "B H H_kv S_q S_cache S_new D".split(),
    "fa_fwd_kvcache_fp8_workspace_bytes": "B H H_kv S_q S_cache S_new D".split(),
    "fa_fwd_kvcache_fp4_workspace_bytes": "B H H_kv S_q S_cache S_new D".split(),
    "fa_fwd_kvcache_paged_workspace_bytes": "B H H_kv S_q max_pages_per_seq page_size S_new D cache_dtype".split(),
    "fa_fwd_kvcache_fp4_paged_workspace_bytes": "B H H_kv S_q max_pages_per_seq page_size S_new D".split(),
    "fa_fwd_kvcache_ragged_workspace_bytes": "total_q B H H_kv max_pages_per_seq page_size D cache_dtype".split(),
}
# a well-formed call: bf16, B = 2, H = 8 over H_kv = 2, one query, D = 128, a cache of 1024 rows or 16 pages of 64 out of 40
DEFAULTS = dict(
    q="P", k_cache="P", v_cache="P", k_scale="P", v_scale="P", k_new=None, v_new=None, cache_seqlens="P", cu_seqlens_q="P",
    block_table="P", o="P", lse=None, workspace=None, workspace_bytes=0, k_descale=None, v_descale=None, descale_bstride=0,
    k_scale_strides=None, v_scale_strides=None, sinks="P", alibi_slopes="P", slopes_batch_stride=0, softcap=30.0,
    B=2, H=8, H_kv=2, S_q=1, S_cache=1024, S_new=0, D=128, dtype=1, kv_dtype=None, cache_dtype=0, scale=0.125, total_q=3,
    num_pages=40, page_size=64, max_pages_per_seq=16, block_table_stride=16, window_left=-1, window_right=-1, opts=None,
    mods=None, stream=None)
KV_DTYPE = {"fa_fwd_kvcache_fp8": 0, "fa_fwd_kvcache_fp8_sink": 0, "fa_fwd_kvcache_fp4": 1, "fa_fwd_kvcache_fp4_paged": 1}

PLAIN, CAP, ALIBI, SINK, FP8, FP8S, PAGED, RAGGED, FP4, FP4P = (
    "fa_fwd_kvcache", "fa_fwd_kvcache_softcap", "fa_fwd_kvcache_alibi", "fa_fwd_kvcache_sink", "fa_fwd_kvcache_fp8",
    "fa_fwd_kvcache_fp8_sink", "fa_fwd_kvcache_paged", "fa_fwd_kvcache_ragged", "fa_fwd_kvcache_fp4", "fa_fwd_kvcache_fp4_paged")
CALLS = (PLAIN, CAP, ALIBI, SINK, FP8, FP8S, PAGED, RAGGED, FP4, FP4P)
WS = tuple(n for n in PARAMS if n.endswith("_workspace_bytes"))
INF, NAN = float("inf"), float("nan")
PAD = 1024 * 128          # elements of one head of the default padded cache


def _cases():
    c = []
    add = lambda cid, fn, **kw: c.append((cid, fn, kw))
    # ---- every call: what kvcache_impl and the shape checks refuse
    for fn in CALLS:
        s = fn[len("fa_fwd_kvcache"):].lstrip("_") or "plain"
        add(s + "/null_q", fn, q=None)
        add(s + "/null_seqlens", fn, cache_seqlens=None)
        add(s + "/k_new_alone", fn, k_new="P")
        add(s + "/scale_zero", fn, scale=0.0)
        add(s + "/scale_nan", fn, scale=NAN)
        add(s + "/opts_size", fn, opts={"size": 8})
        add(s + "/opts_dropout", fn, opts={"p_drop": 0.5})
        add(s + "/group", fn, H=6, H_kv=4)
        add(s + "/H_kv_zero", fn, H_kv=0)
        add(s + "/dtype", fn, dtype=2)
        add(s + "/head_dim_96", fn, D=96)
        add(s + "/window", fn, window_left=-2)
        add(s + "/misaligned_q", fn, q="P+8")
        add(s + "/misaligned_lse", fn, lse="P+4")
        add(s + "/misaligned_seqlens", fn, cache_seqlens="P+2")
        add(s + "/workspace_missing", fn, splits=4)
        add(s + "/workspace_small", fn, splits=4, workspace="P", workspace_bytes=64)
        add(s + "/q_stride_odd", fn, opts={"q_strides": [8 * 128 + 4, 128, 128]} if fn != RAGGED else {"q_strides": [0, 132, 8 * 128]})
        add(s + "/two:group+window", fn, H=6, H_kv=4, window_right=-5)
        add(s + "/two:scale+null", fn, scale=-1.0, o=None)
        if fn != RAGGED:
            add(s + "/B_zero", fn, B=0)
            add(s + "/S_new_negative", fn, S_new=-1)
            add(s + "/S_new_without_k_new", fn, S_new=2)
            add(s + "/k_new_without_S_new", fn, k_new="P", v_new="P")
            add(s + "/too_many_rows", fn, H=1 << 12, H_kv=1 << 12, S_q=(1 << 12) + 1)
            add(s + "/o_stride_zero", fn, opts={"o_strides": [0, 128, 128]})
            add(s + "/two:S_new+D", fn, S_new=-1, D=96)
    for fn in (PLAIN, CAP, ALIBI, SINK, FP8, FP8S, FP4):
        s = fn[len("fa_fwd_kvcache"):].lstrip("_") or "plain"
        add(s + "/S_cache_zero", fn, S_cache=0)
        add(s + "/slice_2^31", fn, S_cache=1 << 23, D=128)
    # ---- cache layouts, by format
    for fn in (PLAIN, CAP, ALIBI, SINK, PAGED):
        s = fn[len("fa_fwd_kvcache"):].lstrip("_") or "plain"
        add(s + "/k_stride_negative", fn, opts={"k_strides": [-8, PAD, 128]})
        add(s + "/k_stride_odd", fn, opts={"k_strides": [2 * PAD + 4, PAD, 128]})
        add(s + "/k_row_short", fn, opts={"k_strides": [2 * PAD, PAD, 64]})
        add(s + "/k_slice_2^31", fn, opts={"k_strides": [0, 0, 1 << 26]})
        add(s + "/kv_row_strides_differ", fn, opts={"k_strides": [2 * PAD, PAD, 128], "v_strides": [4 * PAD, 2 * PAD, 256]})
        add(s + "/two:k_stride+misaligned", fn, v_cache="P+8", opts={"k_strides": [2 * PAD, PAD, 100]})
    for fn in (FP8, FP8S, PAGED):
        s = fn[len("fa_fwd_kvcache"):].lstrip("_")
        kw = {"cache_dtype": 1} if fn == PAGED else {}
        add(s + "/fp8_stride_granule", fn, opts={"k_strides": [2 * PAD + 8, PAD, 128]}, **kw)
        add(s + "/fp8_row_short", fn, opts={"v_strides": [2 * PAD, PAD, 64]}, **kw)
        add(s + "/fp8_slice_2^31", fn, opts={"k_strides": [0, 0, 1 << 27]}, **kw)
        add(s + "/fp8_kv_row_strides_differ", fn, opts={"k_strides": [2 * PAD, PAD, 128], "v_strides": [4 * PAD, 2 * PAD, 256]}, **kw)
    for fn in (FP8, FP8S):
        s = fn[len("fa_fwd_kvcache_"):]
        add(s + "/kv_dtype", fn, kv_dtype=1)
        add(s + "/descale_bstride_small", fn, k_descale="P", descale_bstride=1)
        add(s + "/descale_bstride_huge", fn, k_descale="P", descale_bstride=1 << 31)
        add(s + "/descale_misaligned", fn, v_descale="P+2")
        add(s + "/two:kv_dtype+null", fn, kv_dtype=3, k_cache=None)
        add(s + "/two:descale+window", fn, k_descale="P+1", window_left=-3)
    for fn in (FP4, FP4P):
        s = fn[len("fa_fwd_kvcache_"):]
        rows = 1024 if fn == FP4 else 64
        add(s + "/kv_dtype", fn, kv_dtype=0)
        add(s + "/head_dim_256", fn, D=256)
        add(s + "/null_scale", fn, v_scale=None)
        add(s + "/scale_misaligned", fn, k_scale="P+2")
        add(s + "/scale_misaligned_d64", fn, v_scale="P+1", D=64)
        add(s + "/sinks_misaligned", fn, sinks="P+2")
        add(s + "/no_sinks_null_q", fn, sinks=None, q=None)
        add(s + "/scale_row_short", fn, k_scale_strides=[2 * rows * 4, rows * 4, 0])
        add(s + "/scale_stride_granule", fn, v_scale_strides=[2 * rows * 4, rows * 4, 6])
        add(s + "/scale_slice_2^31", fn, k_scale_strides=[0, 0, 1 << 30])
        add(s + "/cache_stride_granule", fn, opts={"k_strides": [2 * rows * 64 + 8, rows * 64, 64]})
        add(s + "/cache_row_short", fn, opts={"k_strides": [2 * rows * 64, rows * 64, 48]})
        add(s + "/cache_slice_2^31", fn, opts={"v_strides": [0, 0, 1 << 30]})
        add(s + "/kv_row_strides_differ", fn, opts={"k_strides": [2 * rows * 64, rows * 64, 64], "v_strides": [4 * rows * 64, 2 * rows * 64, 128]})
        add(s + "/two:kv_dtype+D", fn, kv_dtype=2, D=256)
        add(s + "/two:D+sinks", fn, D=32, sinks="P+1")
        add(s + "/two:scale_misaligned+scale_stride", fn, k_scale="P+2", k_scale_strides=[2 * rows * 4, rows * 4, 6])
        add(s + "/two:scale_misaligned+cache_misaligned", fn, v_scale="P+2", k_cache="P+8")
        add(s + "/two:sinks+null", fn, sinks="P+2", cache_seqlens=None)
    # ---- the transforms of the padded calls
    add("softcap/zero", CAP, softcap=0.0)
    add("softcap/inf", CAP, softcap=INF)
    add("softcap/two:softcap+null", CAP, softcap=-1.0, q=None)
    add("alibi/null", ALIBI, alibi_slopes=None)
    add("alibi/misaligned", ALIBI, alibi_slopes="P+2")
    add("alibi/stride_small", ALIBI, slopes_batch_stride=4)
    add("alibi/stride_negative", ALIBI, slopes_batch_stride=-8)
    add("alibi/stride_huge", ALIBI, slopes_batch_stride=1 << 31)
    add("alibi/two:slopes+window", ALIBI, alibi_slopes="P+2", window_left=-2)
    add("alibi/two:null+scale", ALIBI, alibi_slopes=None, scale=0.0)
    for fn in (SINK, FP8S):
        s = fn[len("fa_fwd_kvcache_"):]
        add(s + "/sinks_null", fn, sinks=None)
        add(s + "/sinks_misaligned", fn, sinks="P+2")
        add(s + "/two:sinks+q", fn, sinks="P+2", q=None)
    add("fp8_sink/two:kv_dtype+sinks", FP8S, kv_dtype=1, sinks=None)
    # ---- the block table and the page geometry
    for fn in (PAGED, RAGGED, FP4P):
        s = fn[len("fa_fwd_kvcache_"):]
        add(s + "/table_null", fn, block_table=None)
        add(s + "/table_misaligned", fn, block_table="P+2")
        add(s + "/table_stride_small", fn, block_table_stride=8)
        add(s + "/table_stride_huge", fn, block_table_stride=1 << 31)
        for page in (16, 0, 48, -32):
            add(s + "/page_size_%d" % page, fn, page_size=page)
        add(s + "/num_pages_zero", fn, num_pages=0)
        add(s + "/max_pages_zero", fn, max_pages_per_seq=0, block_table_stride=0)
        add(s + "/reach_2^31", fn, max_pages_per_seq=1 << 26, page_size=64, block_table_stride=1 << 26)
        add(s + "/two:table_null+page_size", fn, block_table=None, page_size=16)
        add(s + "/two:page_size+D", fn, page_size=16, D=96)
        add(s + "/two:page_size+table_stride", fn, page_size=48, block_table_stride=1)
        add(s + "/two:table_stride+table_misaligned", fn, block_table_stride=8, block_table="P+2")
        add(s + "/two:table_misaligned+null", fn, block_table="P+2", q=None)
    for fn in (PAGED, RAGGED):
        s = fn[len("fa_fwd_kvcache_"):]
        add(s + "/cache_dtype", fn, cache_dtype=2)
        add(s + "/two:cache_dtype+table_null", fn, cache_dtype=7, block_table=None)
        add(s + "/two:cache_dtype+page_size", fn, cache_dtype=-1, page_size=0)
        add(s + "/two:cache_dtype+table_stride", fn, cache_dtype=2, block_table_stride=1)
        add(s + "/two_transforms", fn, mods={"softcap": 30.0, "sinks": "P"})
        add(s + "/fp8_with_softcap", fn, cache_dtype=1, mods={"softcap": 30.0})
        add(s + "/fp8_with_alibi", fn, cache_dtype=1, mods={"alibi_slopes": "P"})
        add(s + "/descale_without_fp8", fn, mods={"k_descale": "P"})
        add(s + "/descale_bstride_without_fp8", fn, mods={"descale_bstride": 2})
        add(s + "/softcap_nan", fn, mods={"softcap": NAN})
        add(s + "/softcap_negative", fn, mods={"softcap": -1.0})
        add(s + "/sinks_misaligned", fn, mods={"sinks": "P+2"})
        add(s + "/alibi_misaligned", fn, mods={"alibi_slopes": "P+2"})
        add(s + "/alibi_stride_small", fn, mods={"alibi_slopes": "P", "slopes_batch_stride": 4})
        add(s + "/fp8_descale_bstride", fn, cache_dtype=1, mods={"k_descale": "P", "descale_bstride": 1})
        add(s + "/fp8_descale_misaligned", fn, cache_dtype=1, mods={"v_descale": "P+2"})
        add(s + "/two:transforms+softcap_nan", fn, mods={"softcap": NAN, "alibi_slopes": "P"})
        add(s + "/two:sinks_misaligned+null", fn, mods={"sinks": "P+2"}, q=None)
        add(s + "/two:fp8_descale+stride", fn, cache_dtype=1, mods={"k_descale": "P+2"}, opts={"k_strides": [64 * 128 + 8, 64 * 128, 128]})
    # ---- packed queries
    add("ragged/cu_null", RAGGED, cu_seqlens_q=None)
    add("ragged/cu_misaligned", RAGGED, cu_seqlens_q="P+2")
    add("ragged/total_q_zero", RAGGED, total_q=0)
    add("ragged/B_zero", RAGGED, B=0)
    add("ragged/too_many_rows", RAGGED, total_q=(1 << 21) + 1)
    add("ragged/too_many_sequences", RAGGED, B=(1 << 24) + 1, total_q=1)
    add("ragged/q_head_stride_odd", RAGGED, opts={"q_strides": [0, 132, 8 * 128]})
    add("ragged/q_row_short", RAGGED, opts={"q_strides": [0, 128, 64]})
    add("ragged/o_head_stride_zero", RAGGED, opts={"o_strides": [0, 0, 8 * 128]})
    add("ragged/v_new_alone", RAGGED, v_new="P")
    add("ragged/two:cu_null+total_q", RAGGED, cu_seqlens_q=None, total_q=0)
    add("ragged/two:total_q+table_null", RAGGED, total_q=0, block_table=None)
    add("ragged/two:cu_misaligned+q_misaligned", RAGGED, cu_seqlens_q="P+2", q="P+8")
    add("ragged/two:o_stride+kv_stride", RAGGED, opts={"o_strides": [0, 0, 8 * 128], "k_strides": [64 * 128 + 4, 64 * 128, 128]})
    # ---- the workspace functions
    for fn in WS:
        s = "ws_" + (fn[len("fa_fwd_kvcache_"):-len("_workspace_bytes")].rstrip("_") or "plain")
        add(s + "/group", fn, H=6, H_kv=4)
        add(s + "/H_zero", fn, H=0)
        add(s + "/head_dim_96", fn, D=96)
        add(s + "/head_dim_32", fn, D=32)
        add(s + "/two:D256+H_zero", fn, D=256, H=0)
        if "ragged" in fn:
            add(s + "/total_q_zero", fn, total_q=0)
            add(s + "/too_many_rows", fn, total_q=(1 << 21) + 1)
            add(s + "/two:group+total_q", fn, H_kv=3, total_q=0)
        else:
            add(s + "/S_new_negative", fn, S_new=-1)
            add(s + "/S_q_zero", fn, S_q=0)
            add(s + "/too_many_rows", fn, H=1 << 12, H_kv=1 << 12, S_q=(1 << 12) + 1)
            add(s + "/too_many_workgroups", fn, splits=64, B=1 << 14, H=1 << 10, H_kv=1 << 10, S_q=1 << 8, D=64)
            add(s + "/two:S_new+S_q", fn, S_new=-1, S_q=0)
        if "paged" in fn or "ragged" in fn:
            add(s + "/page_size", fn, page_size=40)
            add(s + "/max_pages_zero", fn, max_pages_per_seq=0)
            add(s + "/reach_2^31", fn, max_pages_per_seq=1 << 26)
            add(s + "/two:page_size+group", fn, page_size=0, H_kv=3)
            if "fp4" not in fn:
                add(s + "/cache_dtype", fn, cache_dtype=2)
                add(s + "/two:cache_dtype+page_size", fn, cache_dtype=2, page_size=16)
                add(s + "/two:cache_dtype+D", fn, cache_dtype=-1, D=96)
        else:
            add(s + "/S_cache_zero", fn, S_cache=0)
            add(s + "/slice_2^31", fn, S_cache=1 << 23)
        if "fp4" in fn:
            add(s + "/two:D256+group", fn, D=256, H_kv=3)
    ids = [x[0] for x in c]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    return c


CASES = _cases()


class Replay:
    """Calls the cases' functions in `lib_path` (default: the in-tree library)."""

    def __init__(self, lib_path=None):
        import _mi355fa as fa
        self.fa = fa
        self.lib = ctypes.CDLL(lib_path) if lib_path else fa.lib
        for name in list(PARAMS) + ["fa_last_error"]:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = fa.ALL_SIGNATURES[name]
            assert name == "fa_last_error" or len(fn.argtypes) == len(PARAMS[name]), name
        self.lib.fa_debug_kvcache_splits.argtypes = [ctypes.c_int]
        self.lib.fa_debug_kvcache_splits.restype = None
        self._buf = ctypes.create_string_buffer(256)
        self.base = (ctypes.addressof(self._buf) + 63) // 64 * 64
        self._keep = []

    def ptr(self, v):
        if v is None:
            return None
        assert v == "P" or v.startswith("P+"), v
        return self.base + (int(v[2:]) if len(v) > 1 else 0)

    def strides(self, v):
        if v is None:
            return None
        a = (ctypes.c_longlong * 3)(*v)
        self._keep.append(a)
        return ctypes.cast(a, ctypes.POINTER(ctypes.c_longlong))

    def struct(self, cls, d):
        if d is None:
            return None
        o = cls()
        if cls is self.fa.Opts:
            o.size = ctypes.sizeof(cls)
        for k, v in d.items():
            if k.endswith("_strides") and cls is self.fa.Opts:
                v = self.strides(v)
            elif isinstance(v, str):
                v = self.ptr(v)
            setattr(o, k, v)
        self._keep.append(o)
        return ctypes.byref(o)

    def run(self, fn, kw):
        """(return code, fa_last_error() text) of one case"""
        kw = dict(kw)
        args = dict(DEFAULTS, kv_dtype=KV_DTYPE.get(fn))
        if "sink" not in fn:
            args["sinks"] = None            # optional in the MXFP4 calls; the cases that give them say so
        if fn in (FP4, FP4P):
            args["sinks"] = "P"
        splits = kw.pop("splits", 1)
        unknown = set(kw) - set(PARAMS[fn])
        assert not unknown, (fn, unknown)
        args.update(kw)
        vals = []
        for name in PARAMS[fn]:
            v = args[name]
            if name in ("k_scale_strides", "v_scale_strides"):
                v = self.strides(v)
            elif name == "opts":
                v = self.struct(self.fa.Opts, v)
            elif name == "mods":
                v = self.struct(self.fa.PagedMods, v)
            elif v is None or isinstance(v, str):
                v = self.ptr(v)
            vals.append(v)
        self.lib.fa_debug_kvcache_splits(splits)
        try:
            rc = getattr(self.lib, fn)(*vals)
        finally:
            self.lib.fa_debug_kvcache_splits(0)
            self._keep.clear()
        return [int(rc), self.lib.fa_last_error().decode()]

    def table(self):
        return {cid: self.run(fn, kw) for cid, fn, kw in CASES}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", help="the library to question (default: the in-tree build)")
    ap.add_argument("--commit", default="", help="the commit the library was built from, recorded in the file")
    ap.add_argument("--out")
    a = ap.parse_args()
    table = Replay(a.lib).table()
    launched = [cid for cid, (rc, _) in table.items() if rc >= 0]
    assert not launched, "not refused (every case must be): %s" % launched
    doc = {"commit": a.commit, "tool": "tools/record_refusals.py", "cases": table}
    text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
        print("%d cases, %d distinct refusals -> %s" % (len(table), len({tuple(v) for v in table.values()}), a.out))
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
