"""The paged and packed decode calls' surface, pinned: the pybind signature lines of kvcache_paged_forward and
kvcache_ragged_forward, for each malformed call of the tables below the check that fails FIRST with its exception type and
exact message (tests/golden/paged_errors.json), and the split rule as the four workspace functions of the C ABI return it
over a grid of shapes (tests/golden/decode_splits.json).  tests/host_surface.py does the same for the padded calls.

tests/test_host_paged.py, tests/test_host_kvcache.py and tests/test_gpu_paged_errors.py replay the fixtures; this file, run
as a script, rewrites them from the tree it is run in:

    python tests/paged_surface.py            # rewrite both
    python tests/paged_surface.py --check    # compare only (exit 1 on a difference)
    python tests/paged_surface.py --out DIR  # write them somewhere else

cpu_cases() uses CPU tensors only: its calls reach every check in front of the binding's first is_cuda check (a well-formed
call ends at the wrappers' own device check, or at that one, which is a case too).  gpu_cases() holds the checks behind
it; each is refused before anything is allocated or launched.  A case is (id, thunk); "a+b" violates two checks so that
the fixture fixes their order.  Both fixtures were recorded from the tree before the decode path was folded."""
import ctypes
import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "flashattention-from-scratch-with-triton_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

F8 = torch.float8_e4m3fn
INF, NAN = float("inf"), float("nan")


def _modules():
    """(paged_kvcache, ragged_kvcache, kvcache_paged_forward, kvcache_ragged_forward)"""
    import paged_kvcache as P
    import ragged_kvcache as R
    return P, R, P._ext.kvcache_paged_forward, R._ext.kvcache_ragged_forward


def signatures():
    _, _, fp, fr = _modules()
    return {f.__name__: f.__doc__.splitlines()[0] for f in (fp, fr)}


def _rows(table, prefix, fn, base, rows):
    for name, over in rows.items():
        kw = dict(base)
        kw.update(over)
        table.append(("%s/%s" % (prefix, name), (lambda fn=fn, kw=kw: fn(**kw))))


def _inputs(dev, B=2, H=4, Hkv=2, Sq=1, D=64, page=64, pages=3):
    """zeros-maker, q [B, H, S_q, D], packed q [B + 3, H, D], a pool of B * pages pages, its e4m3 form, cache_seqlens,
    block_table [B, pages] and cu_seqlens_q [B + 1] (the last sequence has four rows)"""
    z = lambda *s, **k: torch.zeros(*s, dtype=k.get("dtype", torch.float16), device=dev)
    pool = z(B * pages, Hkv, page, D)
    bt = torch.arange(B * pages, dtype=torch.int32, device=dev).view(B, pages)
    cu = torch.tensor(list(range(B)) + [B + 3], dtype=torch.int32, device=dev)
    return z, z(B, H, Sq, D), z(B + 3, H, D), pool, pool.to(F8), z(B, dtype=torch.int32), bt, cu


_EXT_TAIL = {"k_new": None, "v_new": None, "window_left": -1, "window_right": -1, "softmax_scale": 0.0, "softcap": 0.0,
             "alibi_slopes": None, "sinks": None, "k_descale": None, "v_descale": None}


def _bases(q, qr, pool, sl, bt, cu):
    """the well-formed keyword sets of (paged wrapper, ragged wrapper, paged binding, ragged binding)"""
    pw = {"q": q, "k_cache": pool, "v_cache": pool, "cache_seqlens": sl, "block_table": bt}
    rw = dict(pw, q=qr, cu_seqlens_q=cu)
    return pw, rw, dict(pw, **_EXT_TAIL), dict(rw, out=None, **_EXT_TAIL)


def cpu_cases():
    P, R, ext_p, ext_r = _modules()
    T = []
    z, q, qr, pool, pool8, sl, bt, cu = _inputs("cpu")
    grad = lambda t: t.clone().requires_grad_(True)
    ones = torch.ones
    kn, knr = z(2, 2, 1, 64), z(5, 2, 64)
    p48, p16 = z(6, 2, 48, 64), z(6, 2, 16, 64)
    pool3 = z(6, 3, 64, 64)
    W, CW = {"window_size": (-2, -1)}, {"is_causal": True, "window_size": (-1, 3)}
    F8P = {"k_cache": pool8, "v_cache": pool8}
    pw, rw, pe, re_ = _bases(q, qr, pool, sl, bt, cu)

    # -- the two Python wrappers: every check of theirs, in their order ------------------------------------------------
    def wrapper_rows(q, kn):
        return {
            "ok": {}, "window": W, "causal_window": CW, "q_none": {"q": None}, "pool_list": {"k_cache": [0.0]},
            "seqlens_list": {"cache_seqlens": [0, 0]}, "table_list": {"block_table": [[0, 1, 2], [3, 4, 5]]},
            "table_int64": {"block_table": bt.long()}, "table_rank": {"block_table": bt[0]},
            "rank_q": {"q": q[0]}, "rank_k": {"k_cache": pool[0]}, "rank_v": {"v_cache": pool[0]},
            "page_48": {"k_cache": p48, "v_cache": p48}, "page_16": {"k_cache": p16, "v_cache": p16},
            "softcap_alibi": {"softcap": 30.0, "alibi_slopes": ones(4)}, "softcap_sinks": {"softcap": 30.0, "sinks": ones(4)},
            "alibi_sinks": {"alibi_slopes": ones(4), "sinks": ones(4)},
            "all_three": {"softcap": 30.0, "alibi_slopes": ones(4), "sinks": ones(4)},
            "fp8_softcap": dict(F8P, softcap=30.0), "fp8_alibi": dict(F8P, alibi_slopes=ones(4)),
            "kdescale_16bit": {"k_descale": ones(2)}, "vdescale_16bit": {"v_descale": ones(2, 2)},
            "softcap_zero": {"softcap": 0.0}, "softcap_neg": {"softcap": -3.0}, "softcap_inf": {"softcap": INF},
            "softcap_nan": {"softcap": NAN}, "scale_neg": {"softmax_scale": -1.0}, "scale_zero": {"softmax_scale": 0.0},
            "scale_inf": {"softmax_scale": INF}, "scale_nan": {"softmax_scale": NAN},
            "knew_alone": {"k_new": kn}, "vnew_alone": {"v_new": kn},
            "grad_q": {"q": grad(q)}, "grad_k": {"k_cache": grad(pool)}, "grad_v": {"v_cache": grad(pool)},
            "grad_knew": {"k_new": grad(kn), "v_new": kn}, "grad_vnew": {"k_new": kn, "v_new": grad(kn)},
            "grad_slopes": {"alibi_slopes": grad(ones(4))}, "grad_sinks": {"sinks": grad(ones(4))},
            "grad_kdescale": dict(F8P, k_descale=grad(ones(2))), "grad_vdescale": dict(F8P, v_descale=grad(ones(2))),
            "grad_q+grad_sinks": {"q": grad(q), "sinks": grad(ones(4))},
            "window+table_int64": dict(W, block_table=bt.long()), "q_none+table_int64": {"q": None, "block_table": bt.long()},
            "table_int64+table_rank": {"block_table": bt[0].long()}, "table_rank+rank_q": {"block_table": bt[0], "q": q[0]},
            "rank_q+page_48": {"q": q[0], "k_cache": p48, "v_cache": p48},
            "page_48+softcap_sinks": {"k_cache": p48, "v_cache": p48, "softcap": 30.0, "sinks": ones(4)},
            "softcap_sinks+kdescale_16bit": {"softcap": 30.0, "sinks": ones(4), "k_descale": ones(2)},
            "fp8_softcap+softcap_zero": dict(F8P, softcap=0.0), "kdescale_16bit+softcap_zero": {"k_descale": ones(2), "softcap": 0.0},
            "softcap_zero+scale_neg": {"softcap": 0.0, "softmax_scale": -1.0},
            "scale_neg+knew_alone": {"softmax_scale": -1.0, "k_new": kn}, "knew_alone+grad_q": {"k_new": kn, "q": grad(q)},
        }
    _rows(T, "P.flash_attention_kvcache_paged", P.flash_attention_kvcache_paged, pw, wrapper_rows(q, kn))
    _rows(T, "R.flash_attention_kvcache_ragged", R.flash_attention_kvcache_ragged, rw, dict(wrapper_rows(qr, knr), **{
        "cu_none": {"cu_seqlens_q": None}, "cu_int64": {"cu_seqlens_q": cu.long()}, "cu_2d": {"cu_seqlens_q": cu[None]},
        "cu_one_entry": {"cu_seqlens_q": cu[:1]}, "table_rows": {"block_table": bt[:1]},
        "seqlens_len": {"cache_seqlens": z(3, dtype=torch.int32)}, "seqlens_2d": {"cache_seqlens": sl[None]},
        "out_list": {"out": [0.0]}, "out_shape": {"out": z(5, 4, 128)}, "out_dtype": {"out": qr.bfloat16()},
        "grad_out": {"out": grad(qr)}, "ok_out": {"out": torch.zeros_like(qr)},
        "window+cu_int64": dict(W, cu_seqlens_q=cu.long()), "cu_int64+cu_2d": {"cu_seqlens_q": cu[None].long()},
        "cu_one_entry+table_int64": {"cu_seqlens_q": cu[:1], "block_table": bt.long()},
        "table_int64+table_rows": {"block_table": bt[:1].long()}, "table_rows+seqlens_len": {"block_table": bt[:1], "cache_seqlens": z(3, dtype=torch.int32)},
        "seqlens_len+rank_q": {"cache_seqlens": z(3, dtype=torch.int32), "q": q},
        "knew_alone+out_shape": {"k_new": knr, "out": z(5, 4, 128)}, "out_shape+out_dtype": {"out": z(5, 4, 128).bfloat16()},
        "out_dtype+grad_q": {"out": qr.bfloat16(), "q": grad(qr)}}))

    # -- the two pybind functions: the checks in front of is_cuda ----------------------------------------------------------
    def ext_rows(q, kn, head_dim):
        return {
            "ok": {}, "rank_q": {"q": q[0]}, "rank_k": {"k_cache": pool[0]}, "rank_v": {"v_cache": pool[0]},
            "kv_shape": {"v_cache": z(6, 2, 64, 128)}, "kv_pages": {"v_cache": z(7, 2, 64, 64)},
            "kv_dtype": {"v_cache": pool8}, "kv_dtype_bf16": {"v_cache": pool.bfloat16()},
            "head_dim": {"k_cache": z(6, 2, 64, 128), "v_cache": z(6, 2, 64, 128)}, "head_dim_96": head_dim,
            "group": {"k_cache": pool3, "v_cache": pool3}, "group_zero": {"k_cache": z(6, 0, 64, 64), "v_cache": z(6, 0, 64, 64)},
            "page_48": {"k_cache": p48, "v_cache": p48}, "page_16": {"k_cache": p16, "v_cache": p16},
            "page_zero": {"k_cache": z(6, 2, 0, 64), "v_cache": z(6, 2, 0, 64)},
            "knew_alone": {"k_new": kn}, "vnew_alone": {"v_new": kn},
            "window_left": {"window_left": -2}, "window_right": {"window_right": -2}, "window_big": {"window_right": 2 ** 31},
            "scale_neg": {"softmax_scale": -1.0}, "grad_q": {"q": grad(q)}, "fp8": F8P,
            "rank_q+kv_shape": {"q": q[0], "v_cache": z(6, 2, 64, 128)}, "kv_shape+head_dim": {"k_cache": z(6, 2, 64, 128)},
            "head_dim+group": {"k_cache": z(6, 3, 64, 128), "v_cache": z(6, 3, 64, 128)},
            "group+page_48": {"k_cache": z(6, 3, 48, 64), "v_cache": z(6, 3, 48, 64)},
            "page_48+knew_alone": {"k_cache": p48, "v_cache": p48, "k_new": kn},
            "knew_alone+window_left": {"k_new": kn, "window_left": -2},
            "window_left+window_big": {"window_left": -2, "window_right": 2 ** 31},
        }
    p96 = z(6, 2, 64, 96)
    _rows(T, "ext.kvcache_paged_forward", ext_p, pe, ext_rows(q, kn, {"q": z(2, 4, 1, 96), "k_cache": p96, "v_cache": p96}))
    _rows(T, "ext.kvcache_ragged_forward", ext_r, re_, dict(
        ext_rows(qr, knr, {"q": z(5, 4, 96), "k_cache": p96, "v_cache": p96}),
        **{"q_empty": {"q": qr[:0]}, "kv_shape+q_empty": {"q": qr[:0], "v_cache": z(7, 2, 64, 64)},
           "q_empty+head_dim": {"q": qr[:0], "k_cache": z(6, 2, 64, 128), "v_cache": z(6, 2, 64, 128)}}))
    return T


def gpu_cases(dev="cuda"):
    """The checks behind is_cuda on device tensors, B 2, H 4, H_kv 2, two pages of 64 keys per sequence, D 64 (and 96 for
    the head-dim check): every case is refused before anything is allocated or launched."""
    P, R, ext_p, ext_r = _modules()
    T = []
    z, q, qr, pool, pool8, sl, bt, cu = _inputs(dev, pages=2)
    ones = lambda *s: torch.ones(*s, device=dev)
    grad = lambda t: t.clone().requires_grad_(True)
    bf, f32 = (lambda t: t.to(torch.bfloat16)), (lambda t: t.float())
    F8P = {"k_cache": pool8, "v_cache": pool8}
    p96 = z(4, 2, 64, 96)
    odd = z(4, 2, 64, 68)[..., 2:66]                     # a base pointer off the 16-byte boundary
    wide = z(4, 2, 64, 72)[..., :64]                     # rows of 144 bytes: addressable, but not V's row stride
    odd8 = z(4, 2, 64, 80).to(F8)[..., 4:68]
    bt_wide = torch.zeros(2, 4, dtype=torch.int32, device=dev)
    pw, rw, pe, re_ = _bases(q, qr, pool, sl, bt, cu)

    def vec_rows(name, n, two_d, fp8):
        """every check_vec failure of one fp32 vector argument ((n,), or (B, n) where two_d)"""
        base = dict(F8P) if fp8 else {}
        rows = {"f64": ones(n).double(), "f16": ones(n).half(), "shape": ones(n + 1), "shape_3B": ones(3, n),
                "noncontig": ones(2 * n)[::2], "grad": grad(ones(n)), "cpu": torch.ones(n),
                "f64+shape": ones(n + 1).double(), "shape+noncontig": ones(2 * n + 2)[::2],
                "noncontig+cpu": torch.ones(2 * n)[::2]}
        rows["2d"] = ones(2, n)          # fine for slopes and descales (ends at a later check or returns): sinks refuse it
        if two_d:
            del rows["2d"]
        return {"%s_%s" % (name, k): dict(base, **{name: v}) for k, v in rows.items()}

    def rows(q, kn, kn_bad, head_dim):
        r = {
            "cpu_seqlens": {"cache_seqlens": sl.cpu()}, "cpu_table": {"block_table": bt.cpu()}, "cpu_q": {"q": q.cpu()},
            "q_f32": {"q": f32(q)}, "pool_bf16": {"k_cache": bf(pool), "v_cache": bf(pool)}, "pool_f32": {"k_cache": f32(pool), "v_cache": f32(pool)},
            "head_dim_96": head_dim, "seqlens_int64": {"cache_seqlens": sl.long()},
            "seqlens_len": {"cache_seqlens": z(3, dtype=torch.int32)}, "seqlens_2d": {"cache_seqlens": sl[None]},
            "seqlens_noncontig": {"cache_seqlens": z(4, dtype=torch.int32)[::2]},
            "table_int64": {"block_table": bt.long()}, "table_rank": {"block_table": bt[0]}, "table_rows": {"block_table": bt[:1]},
            "table_no_pages": {"block_table": bt[:, :0]}, "table_stride": {"block_table": bt_wide[:, ::2]},
            "table_transposed": {"block_table": bt.t().contiguous().t()},
            "pool_misaligned": {"k_cache": odd, "v_cache": odd}, "pool_row_strides": {"k_cache": wide},
            "pool_head_dim_stride": {"k_cache": pool.transpose(2, 3).contiguous().transpose(2, 3),
                                     "v_cache": pool.transpose(2, 3).contiguous().transpose(2, 3)},
            "fp8_pool_misaligned": {"k_cache": odd8, "v_cache": odd8},
            "knew_dtype": {"k_new": f32(kn), "v_new": f32(kn)}, "vnew_dtype": {"k_new": kn, "v_new": bf(kn)},
            "knew_cpu": {"k_new": kn.cpu(), "v_new": kn.cpu()},
            "q_f32+pool_bf16": {"q": f32(q), "k_cache": bf(pool), "v_cache": bf(pool)},
            "pool_bf16+head_dim_96": dict(head_dim, k_cache=bf(p96), v_cache=bf(p96)),
            "head_dim_96+seqlens_int64": dict(head_dim, cache_seqlens=sl.long()),
            "seqlens_int64+table_int64": {"cache_seqlens": sl.long(), "block_table": bt.long()},
            "table_int64+sinks_f64": {"block_table": bt.long(), "sinks": ones(4).double()},
            "sinks_f64+pool_misaligned": {"sinks": ones(4).double(), "k_cache": odd, "v_cache": odd},
            "pool_misaligned+knew_dtype": {"k_cache": odd, "v_cache": odd, "k_new": f32(kn), "v_new": f32(kn)},
        }
        for name, over in kn_bad.items():
            r["knew_" + name] = {"k_new": over, "v_new": over}
        r["knew_shapes"] = {"k_new": kn, "v_new": torch.cat([kn, kn], dim=-2 if kn.dim() == 4 else 0)}
        r["knew_shapes+knew_dtype"] = {"k_new": f32(kn), "v_new": f32(r["knew_shapes"]["v_new"])}
        r.update(vec_rows("alibi_slopes", 4, True, False))
        r.update(vec_rows("sinks", 4, False, False))
        r.update(vec_rows("k_descale", 2, True, True))
        r.update(vec_rows("v_descale", 2, True, True))
        return r

    kn, knr = z(2, 2, 1, 64), z(5, 2, 64)
    paged_rows = rows(q, kn, {"rank": kn[0], "batch": z(3, 2, 1, 64), "heads": z(2, 4, 1, 64), "head_dim": z(2, 2, 1, 32),
                              "empty": kn[:, :, :0]}, {"q": z(2, 4, 1, 96), "k_cache": p96, "v_cache": p96})
    ragged_rows = rows(qr, knr, {"rank": kn, "rows": z(4, 2, 64), "heads": z(5, 4, 64), "head_dim": z(5, 2, 32)},
                       {"q": z(5, 4, 96), "k_cache": p96, "v_cache": p96})
    ragged_rows.update({
        "cpu_cu": {"cu_seqlens_q": cu.cpu()}, "cu_noncontig": {"cu_seqlens_q": torch.zeros(6, dtype=torch.int32, device=dev)[::2]},
        "out_cpu": {"out": qr.cpu()}, "out_head_dim_stride": {"out": z(5, 4, 128)[..., ::2]},
        "out_misaligned": {"out": z(5, 4, 68)[..., 2:66]}, "out_row_stride": {"out": z(5, 4 * 64 + 4)[:, :256].view(5, 4, 64)},
        "out_heads_overlap": {"out": z(5, 1, 64).expand(5, 4, 64)},
        "head_dim_96+cu_noncontig": {"q": z(5, 4, 96), "k_cache": p96, "v_cache": p96,
                                     "cu_seqlens_q": torch.zeros(6, dtype=torch.int32, device=dev)[::2]},
        "knew_dtype+out_cpu": {"k_new": f32(knr), "v_new": f32(knr), "out": qr.cpu()},
        "out_cpu+out_misaligned": {"out": z(5, 4, 68)[..., 2:66].cpu()}})
    ext_only = lambda q, kn: {
        "grad_q": {"q": grad(q)}, "grad_k": {"k_cache": grad(pool)}, "grad_v": {"v_cache": grad(pool)},
        "grad_knew": {"k_new": grad(kn), "v_new": kn}, "grad_vnew": {"k_new": kn, "v_new": grad(kn)},
        "table_stride+grad_q": {"block_table": bt_wide[:, ::2], "q": grad(q)}, "grad_q+sinks_f64": {"q": grad(q), "sinks": ones(4).double()}}
    ext_ragged = {"cu_int64": {"cu_seqlens_q": cu.long()}, "cu_2d": {"cu_seqlens_q": cu[None]}, "cu_one_entry": {"cu_seqlens_q": cu[:1]},
                  "out_shape": {"out": z(5, 4, 128)}, "out_dtype": {"out": bf(qr)}, "out_grad": {"out": grad(qr)},
                  "cu_int64+seqlens_len": {"cu_seqlens_q": cu.long(), "cache_seqlens": z(3, dtype=torch.int32)},
                  "out_shape+out_grad": {"out": grad(z(5, 4, 128))}, "out_grad+out_misaligned": {"out": z(5, 4, 68, ).requires_grad_(True)[..., 2:66]}}
    _rows(T, "P.flash_attention_kvcache_paged", P.flash_attention_kvcache_paged, pw, paged_rows)
    _rows(T, "R.flash_attention_kvcache_ragged", R.flash_attention_kvcache_ragged, rw, ragged_rows)
    _rows(T, "ext.kvcache_paged_forward", ext_p, pe, dict(paged_rows, **ext_only(q, kn)))
    _rows(T, "ext.kvcache_ragged_forward", ext_r, re_, dict(ragged_rows, **ext_only(qr, knr), **ext_ragged))
    return T


def outcome(thunk):
    """[exception type, message] of a call that must be refused; a call that returns is recorded as such"""
    try:
        thunk()
    except Exception as e:      # the type and the text are the surface
        return [type(e).__name__, str(e)]
    return ["returned", ""]


def errors(cases):
    return {cid: outcome(thunk) for cid, thunk in cases}


# ---- the split rule, as the workspace functions return it ----------------------------------------------------------------------
GRID = {"B": [1, 2, 8, 64, 300], "H_kv": [1, 8], "group": [1, 4, 8], "S_q": [1, 5, 33, 512],
        "reach": [64, 2048, 4096, 32768, 131072], "D": [64, 128]}
PAGE = 64     # the paged and the ragged functions: reach = max_pages_per_seq * PAGE


def split_grid():
    """{"grid": GRID, "page_size": PAGE, function: [value per grid point, itertools.product order]}: the workspace bytes
    (or the error code) of every function at the formula's split count.  The ragged function takes S_q as total_q."""
    import _mi355fa as fa
    L = fa.lib
    L.fa_debug_kvcache_splits.argtypes, L.fa_debug_kvcache_splits.restype = [ctypes.c_int], None
    L.fa_debug_kvcache_splits(0)
    out = {"grid": GRID, "page_size": PAGE, "padded": [], "padded_fp8": [], "paged_16bit": [], "paged_fp8": [],
           "ragged_16bit": [], "ragged_fp8": []}
    for B, Hkv, g, Sq, reach, D in itertools.product(*GRID.values()):
        H = Hkv * g
        out["padded"].append(L.fa_fwd_kvcache_workspace_bytes(B, H, Hkv, Sq, reach, 0, D))
        out["padded_fp8"].append(L.fa_fwd_kvcache_fp8_workspace_bytes(B, H, Hkv, Sq, reach, 0, D))
        for name, cdt in (("16bit", fa.PAGED_CACHE_16BIT), ("fp8", fa.PAGED_CACHE_FP8_E4M3)):
            out["paged_" + name].append(L.fa_fwd_kvcache_paged_workspace_bytes(B, H, Hkv, Sq, reach // PAGE, PAGE, 0, D, cdt))
            out["ragged_" + name].append(L.fa_fwd_kvcache_ragged_workspace_bytes(Sq, B, H, Hkv, reach // PAGE, PAGE, D, cdt))
    return out


def _load(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)


def main(argv):
    out = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN     # another directory: leave the fixtures alone
    old = _load("paged_errors.json") if os.path.exists(os.path.join(GOLDEN, "paged_errors.json")) else {}
    # the GPU table is recorded where there is a GPU; elsewhere the committed one is kept
    got = {"paged_errors.json": {"signatures": signatures(), "cpu": errors(cpu_cases()),
                                 "gpu": errors(gpu_cases()) if torch.cuda.is_available() else old.get("gpu", {})},
           "decode_splits.json": split_grid()}
    if "--check" in argv:
        bad = [n for n in got if not os.path.exists(os.path.join(GOLDEN, n)) or _load(n) != got[n]]
        print("differs: %s" % ", ".join(bad) if bad else "fixtures match this tree")
        return 1 if bad else 0
    for n, data in got.items():
        with open(os.path.join(out, n), "w") as fh:
            if n == "decode_splits.json":      # long lists of integers: one line per list
                fh.write("{\n" + ",\n".join(' %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in sorted(data.items())) + "\n}\n")
            else:
                json.dump(data, fh, indent=1, sort_keys=True)
                fh.write("\n")
        print("wrote %s" % os.path.join(os.path.relpath(out, ROOT), n))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
