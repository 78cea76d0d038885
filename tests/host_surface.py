"""The host layer's surface, pinned: every public signature of My_FlashAttention_optimized and _mi355fa_torch, and a table
of malformed calls with the exception each raises -- which check fails FIRST, its type and its exact message.

tests/test_host_surface.py replays the tables against tests/golden/host_surface.json and tests/golden/host_errors.json;
this file, run as a script, rewrites the two fixtures from the tree it is run in:

    python tests/host_surface.py            # rewrite both
    python tests/host_surface.py --check    # compare only (exit 1 on a difference)
    python tests/host_surface.py --out DIR  # write them somewhere else

cpu_cases() uses CPU tensors only: its calls reach every check in front of the first is_cuda check (a well-formed call ends at
that check, which is a case too).  gpu_cases() (tests/test_gpu_host_errors.py) holds the checks behind it; each is refused
before anything is allocated or launched.  A case is (id, thunk); the id names the violated checks, "a+b" violates two
so that the fixture fixes their order."""
import inspect
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
    import My_FlashAttention_optimized as M
    import _mi355fa_torch as ext
    return M, ext


# ---- signatures ------------------------------------------------------------------------------------------------------------
def surface():
    """{"python": {name: signature}, "autograd": {Class.method: signature}, "binding": {name: pybind signature line}}"""
    M, ext = _modules()
    py, auto = {}, {}
    for name, obj in sorted(vars(M).items()):
        if name.startswith("_") or getattr(obj, "__module__", None) != M.__name__:
            continue
        if inspect.isclass(obj):
            for meth in ("forward", "backward"):
                auto["%s.%s" % (name, meth)] = str(inspect.signature(getattr(obj, meth)))
        elif callable(obj):
            py[name] = str(inspect.signature(obj))
    binding = {name: obj.__doc__.splitlines()[0] for name, obj in sorted(vars(ext).items())
               if callable(obj) and not name.startswith("_")}
    constants = {"FP8_E4M3_MAX": M.FP8_E4M3_MAX, "_DTYPES": sorted(str(k) for k in M._DTYPES),
                 "private": sorted(n for n in ("_check_qkv", "_in_place", "_gqa_window", "_fa", "_DTYPES") if hasattr(M, n))}
    return {"python": py, "autograd": auto, "binding": binding, "constants": constants}


# ---- malformed calls ---------------------------------------------------------------------------------------------------------
def _rows(table, prefix, fn, base, rows):
    for name, over in rows.items():
        kw = dict(base)
        kw.update(over)
        table.append(("%s/%s" % (prefix, name), (lambda fn=fn, kw=kw: fn(**kw))))


def _apply(cls, names):
    """A Function.apply that takes the forward's arguments by name"""
    return lambda **kw: cls.apply(*[kw[n] for n in names if n in kw])


def _decode_inputs(dev, B=2, H=4, Hkv=2, Sq=1, Sc=16, D=64):
    z = lambda *s, **k: torch.zeros(*s, dtype=k.get("dtype", torch.float16), device=dev)
    q, K = z(B, H, Sq, D), z(B, Hkv, Sc, D)
    return z, q, K, K.to(F8), z(B, dtype=torch.int32)


def cpu_cases():
    M, ext = _modules()
    T = []
    z, q, K, K8, sl = _decode_inputs("cpu")
    grad = lambda t: t.clone().requires_grad_(True)
    ones = torch.ones
    W, CW = {"window_size": (-2, -1)}, {"is_causal": True, "window_size": (-1, 3)}
    GQ = {"q": grad(q)}
    bad_vec = lambda name, H, decode: {       # a (H,) fp32 vector argument: slopes or sinks
        "list": {name: [0.0] * H}, "f64": {name: ones(H).double()}, "f16": {name: ones(H).half()},
        "shape": {name: ones(H + 1)}, "shape_2d": {name: ones(H, 1)}, "noncontig": {name: ones(2 * H)[::2]},
        "meta": {name: ones(H, device="meta")}, "grad": {name: grad(ones(H))},
        "f64+shape": {name: ones(H + 1).double()}, "shape+noncontig": {name: ones(2 * H + 2)[::2]},
        "noncontig+grad": {name: grad(ones(2 * H))[::2]}, "meta+grad": {name: ones(H, device="meta").requires_grad_(True)},
        "grad+scale": {name: grad(ones(H)), "softmax_scale": -1.0},
    }
    SCALE = {"scale_neg": {"softmax_scale": -1.0}, "scale_zero": {"softmax_scale": 0.0}, "scale_inf": {"softmax_scale": INF},
             "scale_nan": {"softmax_scale": NAN}}
    CAP = {"softcap_zero": {"softcap": 0.0}, "softcap_neg": {"softcap": -3.0}, "softcap_inf": {"softcap": INF},
           "softcap_nan": {"softcap": NAN}}

    # -- the six Python decode wrappers ------------------------------------------------------------------------------
    d16 = {"q": q, "k_cache": K, "v_cache": K, "cache_seqlens": sl}
    d8 = {"q": q, "k_cache": K8, "v_cache": K8, "cache_seqlens": sl}
    guards16 = {
        "ok": {}, "window": W, "causal_window": CW, "window+causal_window": {"is_causal": True, "window_size": (-2, 3)},
        "grad_q": GQ, "grad_k": {"k_cache": grad(K)}, "grad_v": {"v_cache": grad(K)}, "window+grad": dict(W, **GQ),
        "causal_window+grad": dict(CW, **GQ), "grad+knew_alone": dict(GQ, k_new=K[:, :, :1]),
        "knew_alone": {"k_new": K[:, :, :1]}, "scale_neg": {"softmax_scale": -1.0}, "scale_inf": {"softmax_scale": INF},
        "return_lse": {"return_lse": True},
    }
    _rows(T, "M.flash_attention_kvcache", M.flash_attention_kvcache, d16, guards16)
    _rows(T, "M.flash_attention_kvcache_softcap", M.flash_attention_kvcache_softcap, dict(d16, softcap=30.0), dict(
        guards16, **CAP, **SCALE, **{"softcap+scale": {"softcap": 0.0, "softmax_scale": -1.0},
                                     "scale+window": dict(W, softmax_scale=-1.0), "softcap+grad": dict(GQ, softcap=-1.0)}))
    _rows(T, "M.flash_attention_kvcache_alibi", M.flash_attention_kvcache_alibi, dict(d16, alibi_slopes=ones(4)), dict(
        guards16, **bad_vec("alibi_slopes", 4, True), **SCALE,
        **{"slopes_BH": {"alibi_slopes": ones(2, 4)}, "slopes_3H": {"alibi_slopes": ones(3, 4)},
           "scale+window": dict(W, softmax_scale=-1.0), "rank_q": {"q": q[0]}}))
    _rows(T, "M.flash_attention_kvcache_sink", M.flash_attention_kvcache_sink, dict(d16, sinks=ones(4)), dict(
        guards16, **bad_vec("sinks", 4, True), **SCALE,
        **{"scale+window": dict(W, softmax_scale=-1.0), "sinks_grad+grad_q": dict(GQ, sinks=grad(ones(4)))}))
    kd_ok = ones(2, 2)
    fp8_rows = {
        "ok": {}, "ok_descales": {"k_descale": kd_ok, "v_descale": ones(2)}, "window": W, "causal_window": CW,
        "cache_f16": {"k_cache": K, "v_cache": K}, "cache_k_f16": {"k_cache": K}, "cache_v_u8": {"v_cache": K8.view(torch.uint8)},
        "cache_fnuz": {"k_cache": K.to(torch.float8_e4m3fnuz), "v_cache": K.to(torch.float8_e4m3fnuz)},
        "rank_q": {"q": q[0]}, "rank_k": {"k_cache": K8[0]}, "kdescale_list": {"k_descale": [1.0, 1.0]},
        "kdescale_f64": {"k_descale": kd_ok.double()}, "kdescale_shape": {"k_descale": ones(3)},
        "kdescale_grad": {"k_descale": grad(kd_ok)}, "vdescale_f64": {"v_descale": kd_ok.double()},
        "vdescale_shape": {"v_descale": ones(2, 3)}, "vdescale_grad": {"v_descale": grad(kd_ok)},
        "knew_alone": {"k_new": K[:, :, :1]}, "vnew_alone": {"v_new": K[:, :, :1]}, "grad_q": GQ,
        "grad_knew": {"k_new": grad(K[:, :, :1]), "v_new": K[:, :, :1]},
        "grad_vnew": {"k_new": K[:, :, :1], "v_new": grad(K[:, :, :1])},
        "scale_neg": {"softmax_scale": -1.0}, "scale_inf": {"softmax_scale": INF},
        "window+cache_f16": dict(W, k_cache=K, v_cache=K), "cache_f16+rank_q": {"k_cache": K, "v_cache": K, "q": q[0]},
        "rank_q+kdescale_f64": {"q": q[0], "k_descale": kd_ok.double()},
        "kdescale_shape+vdescale_f64": {"k_descale": ones(3), "v_descale": kd_ok.double()},
        "kdescale_f64+kdescale_grad": {"k_descale": grad(kd_ok.double())},
        "vdescale_grad+knew_alone": {"v_descale": grad(kd_ok), "k_new": K[:, :, :1]},
        "knew_alone+grad_q": dict(GQ, k_new=K[:, :, :1]),
    }
    _rows(T, "M.flash_attention_kvcache_fp8", M.flash_attention_kvcache_fp8, d8, fp8_rows)
    _rows(T, "M.flash_attention_kvcache_fp8_sink", M.flash_attention_kvcache_fp8_sink, dict(d8, sinks=ones(4)), dict(
        fp8_rows, **bad_vec("sinks", 4, True), **SCALE,
        **{"sinks_f64+cache_f16": {"sinks": ones(4).double(), "k_cache": K, "v_cache": K},
           "scale+window": dict(W, softmax_scale=-1.0), "sinks_grad+window": dict(W, sinks=grad(ones(4)))}))

    # -- their six pybind functions ----------------------------------------------------------------------------------
    K3 = z(2, 3, 16, 64)
    shape_rows = lambda K, cast: {     # the checks kvcache_forward runs in front of is_cuda, caches made by cast(.)
        "ok": {}, "rank_q": {"q": q[0]}, "rank_k": {"k_cache": cast(K[0])}, "rank_v": {"v_cache": cast(K[0])},
        "kv_shape": {"v_cache": cast(z(2, 2, 17, 64))}, "batch": {"k_cache": cast(z(3, 2, 16, 64)), "v_cache": cast(z(3, 2, 16, 64))},
        "head_dim": {"k_cache": cast(z(2, 2, 16, 32)), "v_cache": cast(z(2, 2, 16, 32))},
        "group": {"k_cache": cast(K3), "v_cache": cast(K3)},
        "group_zero": {"k_cache": cast(z(2, 0, 16, 64)), "v_cache": cast(z(2, 0, 16, 64))},
        "knew_alone": {"k_new": K[:, :, :1]}, "vnew_alone": {"v_new": K[:, :, :1]},
        "window_left": {"window_left": -2}, "window_right": {"window_right": -2}, "window_big": {"window_right": 2 ** 31},
        "scale_neg": {"softmax_scale": -1.0}, "grad_q": GQ,
        "rank_q+kv_shape": {"q": q[0], "v_cache": cast(z(2, 2, 17, 64))},
        "kv_shape+batch": {"k_cache": cast(z(3, 2, 16, 64))},
        "batch+group": {"k_cache": cast(z(3, 3, 16, 64)), "v_cache": cast(z(3, 3, 16, 64))},
        "group+knew_alone": {"k_cache": cast(K3), "v_cache": cast(K3), "k_new": K[:, :, :1]},
        "knew_alone+window_left": {"k_new": K[:, :, :1], "window_left": -2},
        "window_left+window_big": {"window_left": -2, "window_right": 2 ** 31},
        "window_big+grad_q": dict(GQ, window_left=2 ** 31),
    }
    same, to8 = (lambda t: t), (lambda t: t.to(F8))
    _rows(T, "ext.kvcache_forward", ext.kvcache_forward, d16, shape_rows(K, same))
    _rows(T, "ext.kvcache_softcap_forward", ext.kvcache_softcap_forward, dict(d16, softcap=30.0), dict(
        shape_rows(K, same), **CAP, **{"softcap+rank_q": {"softcap": 0.0, "q": q[0]}}))
    vec_ext = lambda name: {k: v for k, v in bad_vec(name, 4, True).items() if k not in ("list", "grad+scale")}
    _rows(T, "ext.kvcache_alibi_forward", ext.kvcache_alibi_forward, dict(d16, alibi_slopes=ones(4)), dict(
        shape_rows(K, same), **vec_ext("alibi_slopes"),
        **{"slopes_BH": {"alibi_slopes": ones(2, 4)}, "window_big+f64": {"window_right": 2 ** 31, "alibi_slopes": ones(4).double()},
           "rank_q+shape": {"q": q[0], "alibi_slopes": ones(5)}}))
    _rows(T, "ext.kvcache_sink_forward", ext.kvcache_sink_forward, dict(d16, sinks=ones(4)), dict(
        shape_rows(K, same), **vec_ext("sinks"), **{"f64+rank_q": {"q": q[0], "sinks": ones(4).double()}}))
    fp8_shape = dict(shape_rows(K, to8), **{
        "cache_f16": {"k_cache": K, "v_cache": K}, "cache_v_f16": {"v_cache": K}, "cache_u8": {"k_cache": K8.view(torch.uint8)},
        "rank_k+cache_f16": {"k_cache": K[0], "v_cache": K}, "cache_f16+kv_shape": {"k_cache": K, "v_cache": z(2, 2, 17, 64)},
        "kdescale_f64": {"k_descale": kd_ok.double()}, "kdescale_f64+window_left": {"k_descale": kd_ok.double(), "window_left": -2}})
    _rows(T, "ext.kvcache_fp8_forward", ext.kvcache_fp8_forward, d8, fp8_shape)
    _rows(T, "ext.kvcache_fp8_sink_forward", ext.kvcache_fp8_sink_forward, dict(d8, sinks=ones(4)), dict(
        fp8_shape, **vec_ext("sinks"), **{"f64+cache_f16": {"sinks": ones(4).double(), "k_cache": K, "v_cache": K}}))

    # -- the softcap / alibi / sink training functions and launchers -------------------------------------------------
    Q, Kt = z(2, 4, 16, 64), z(2, 2, 16, 64)
    Qp, Kp = z(16, 4, 64), z(16, 2, 64)
    cu = torch.tensor([0, 5, 9, 16], dtype=torch.int32)
    VL = {"Q": Qp, "K": Kp, "V": Kp, "cu_seqlens_q": cu, "cu_seqlens_k": cu}
    VLM = dict(VL, max_seqlen_q=7, max_seqlen_k=7)
    bwd = {"O": Q, "dO": Q, "LSE": torch.zeros(2, 4, 16)}
    qkv = {"Q": Q, "K": Kt, "V": Kt}
    K3t = z(2, 3, 16, 64)
    check_rows = {     # the binding's grouped() and check(), in front of is_cuda
        "ok": {}, "ok_varlen": VLM, "cu_q_alone": {"cu_seqlens_q": cu, "max_seqlen_q": 7, "max_seqlen_k": 7},
        "cu_k_alone": {"cu_seqlens_k": cu, "max_seqlen_q": 7, "max_seqlen_k": 7}, "cu_q_alone_no_max": {"cu_seqlens_q": cu},
        "varlen_no_max": VL, "varlen_max_q_zero": dict(VL, max_seqlen_q=0, max_seqlen_k=7),
        "varlen_max_k_zero": dict(VL, max_seqlen_q=7, max_seqlen_k=0),
        "rank_q": {"Q": Q[0]}, "rank_k": {"K": Kt[0]}, "rank_varlen": dict(VLM, Q=Q), "kv_shape": {"V": z(2, 2, 17, 64)},
        "batch": {"K": z(3, 2, 16, 64), "V": z(3, 2, 16, 64)}, "head_dim": {"K": z(2, 2, 16, 32), "V": z(2, 2, 16, 32)},
        "head_dim_96": {"Q": z(2, 4, 16, 96), "K": z(2, 2, 16, 96), "V": z(2, 2, 16, 96)},
        "group": {"K": K3t, "V": K3t}, "group_zero": {"K": z(2, 0, 16, 64), "V": z(2, 0, 16, 64)},
        "cu_int64": dict(VLM, cu_seqlens_q=cu.long()), "cu_lengths": dict(VLM, cu_seqlens_k=cu[:3]),
        "cu_2d": dict(VLM, cu_seqlens_q=cu[None]), "cu_one_entry": dict(VLM, cu_seqlens_q=cu[:1], cu_seqlens_k=cu[:1]),
        "cu_q_alone+rank_q": {"cu_seqlens_q": cu, "max_seqlen_q": 7, "max_seqlen_k": 7, "Q": Q[0]},
        "varlen_max_q_zero+rank": dict(VL, max_seqlen_q=0, max_seqlen_k=7, Q=Q),
        "rank_q+kv_shape": {"Q": Q[0], "V": z(2, 2, 17, 64)}, "kv_shape+batch": {"K": z(3, 2, 16, 64)},
        "batch+head_dim": {"K": z(3, 2, 16, 32), "V": z(3, 2, 16, 32)},
        "head_dim+group": {"K": z(2, 3, 16, 32), "V": z(2, 3, 16, 32)},
        "group+cu_int64": dict(VLM, K=z(16, 3, 64), V=z(16, 3, 64), cu_seqlens_q=cu.long()),
    }
    win_launch = {"window_left": {"window_left": -2}, "window_right": {"window_right": -2}, "window_big": {"window_left": 2 ** 31},
                  "group+window_left": {"K": K3t, "V": K3t, "window_left": -2},
                  "window_right+cu_int64": dict(VLM, window_right=-2, cu_seqlens_q=cu.long()),
                  "window_left+window_big": {"window_left": -2, "window_right": 2 ** 31}}
    win_public = {"window": W, "causal_window": CW, "window+causal_window": {"is_causal": True, "window_size": (-2, 3)},
                  "window_big": {"window_size": (2 ** 31, -1)}, "window+cu_q_alone_no_max": dict(W, cu_seqlens_q=cu),
                  "window+rank_q": dict(W, Q=Q[0]), "group+window_big": {"K": K3t, "V": K3t, "window_size": (-1, 2 ** 31)}}
    order = ("Q", "K", "V")
    tail = ("window_left", "window_right", "softmax_scale", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k")
    feats = (
        ("softcap", "softcap", 30.0, dict(CAP, **{"softcap+scale": {"softcap": 0.0, "softmax_scale": -1.0},
                                                    "softcap+rank_q": {"softcap": INF, "Q": Q[0]}}),
         M.FlashAttentionSoftcapFunction),
        ("alibi", "alibi_slopes", ones(4), dict(bad_vec("alibi_slopes", 4, False), **{
            "slopes_BH": {"alibi_slopes": ones(2, 4)}, "slopes_varlen_B": dict(VLM, alibi_slopes=ones(3, 4)),
            "slopes_varlen_wrong_B": dict(VLM, alibi_slopes=ones(2, 4)), "f64+rank_q": {"alibi_slopes": ones(4).double(), "Q": Q[0]},
            "group+f64": {"K": K3t, "V": K3t, "alibi_slopes": ones(4).double()}}), M.FlashAttentionAlibiFunction),
        ("sink", "sinks", ones(4), dict(bad_vec("sinks", 4, False), **{
            "sinks_varlen_shape": dict(VLM, sinks=ones(16)), "f64+rank_q": {"sinks": ones(4).double(), "Q": Q[0]},
            "group+f64": {"K": K3t, "V": K3t, "sinks": ones(4).double()}}), M.FlashAttentionSinkFunction),
    )
    for feat, arg, ok, own, twin in feats:
        base = dict(qkv, **{arg: ok})
        scale_rows = dict(SCALE, **{"scale+rank_q": {"softmax_scale": -1.0, "Q": Q[0]},
                                    "scale+cu_q_alone": {"softmax_scale": INF, "cu_seqlens_q": cu, "max_seqlen_q": 7, "max_seqlen_k": 7}})
        launch_rows = dict(check_rows, **win_launch, **scale_rows, **own)
        if feat != "softcap":     # no list in front of pybind: its TypeError text is pybind's, not the project's
            launch_rows = {k: v for k, v in launch_rows.items() if k != "list"}
        public = getattr(M, "flash_attention_" + feat)
        _rows(T, "M.flash_attention_" + feat, public, base, dict(check_rows, **win_public, **scale_rows, **own,
                                                                  **{"scale+window": dict(W, softmax_scale=-1.0)}))
        _rows(T, "M.flash_attention_%s_forward" % feat, getattr(M, "flash_attention_%s_forward" % feat),
              dict(base, window_left=-1, window_right=0), launch_rows)
        _rows(T, "M.flash_attention_%s_backward" % feat, getattr(M, "flash_attention_%s_backward" % feat),
              dict(base, window_left=-1, window_right=0, **bwd), launch_rows)
        _rows(T, "M.%s.apply" % twin.__name__, _apply(twin, order + (arg,) + tail),
              dict(base, window_left=-1, window_right=0, softmax_scale=None, cu_seqlens_q=None, cu_seqlens_k=None,
                   max_seqlen_q=0, max_seqlen_k=0), dict(launch_rows, **({"list": own["list"]} if "list" in own else {})))
        _rows(T, "ext.flash_attention_" + feat, getattr(ext, "flash_attention_" + feat), base, launch_rows)
        _rows(T, "ext.%s_forward_launch" % feat, getattr(ext, feat + "_forward_launch"), base, launch_rows)
        _rows(T, "ext.%s_backward_launch" % feat, getattr(ext, feat + "_backward_launch"), dict(base, **bwd), launch_rows)
    return T


def gpu_cases(dev="cuda"):
    """The checks behind is_cuda, B=1 H=2 H_kv=1 S_q=1 S_cache=16, D=64 (and 96 for the head-dim check): every case is
    refused before anything is allocated or launched."""
    M, ext = _modules()
    T = []
    z, q, K, K8, sl = _decode_inputs(dev, B=1, H=2, Hkv=1)
    _, q96, K96, K96_8, _ = _decode_inputs(dev, B=1, H=2, Hkv=1, D=96)
    kn = K[:, :, :1]
    ones = lambda *s: torch.ones(*s, device=dev)
    bf = lambda t: t.to(torch.bfloat16)
    f32 = lambda t: t.float()
    Kt = z(1, 16, 1, 72)[..., :64].transpose(1, 2)     # rows of 144 bytes: a multiple of 16 the kernels address in place
    Kodd = z(1, 1, 16, 68)[..., 2:66]                  # a base pointer off the 16-byte boundary: copied, so no append
    K8odd = z(1, 1, 16, 80).to(F8)[..., 4:68]
    Kt8 = z(1, 16, 1, 80).to(F8)[..., :64].transpose(1, 2)
    common = lambda K, cast: {
        "cpu_seqlens": {"cache_seqlens": sl.cpu()}, "q_f32": {"q": f32(q)}, "head_dim_96": {"q": q96, "k_cache": cast(K96), "v_cache": cast(K96)},
        "seqlens_int64": {"cache_seqlens": sl.long()}, "seqlens_shape": {"cache_seqlens": z(2, dtype=torch.int32)},
        "seqlens_2d": {"cache_seqlens": sl[None]},
        "knew_rank": {"k_new": kn[0], "v_new": kn[0]}, "knew_shapes": {"k_new": kn, "v_new": K[:, :, :2]},
        "knew_batch": {"k_new": z(2, 1, 1, 64), "v_new": z(2, 1, 1, 64)}, "knew_heads": {"k_new": z(1, 2, 1, 64), "v_new": z(1, 2, 1, 64)},
        "knew_head_dim": {"k_new": z(1, 1, 1, 32), "v_new": z(1, 1, 1, 32)}, "knew_empty": {"k_new": kn[:, :, :0], "v_new": kn[:, :, :0]},
        "knew_dtype": {"k_new": f32(kn), "v_new": f32(kn)}, "vnew_dtype": {"k_new": kn, "v_new": bf(kn)},
        "knew_cpu": {"k_new": kn.cpu(), "v_new": kn.cpu()},
        "q_f32+head_dim_96": {"q": f32(q96), "k_cache": cast(K96), "v_cache": cast(K96)},
        "head_dim_96+seqlens_int64": {"q": q96, "k_cache": cast(K96), "v_cache": cast(K96), "cache_seqlens": sl.long()},
        "seqlens_int64+knew_rank": {"cache_seqlens": sl.long(), "k_new": kn[0], "v_new": kn[0]},
        "knew_shapes+knew_dtype": {"k_new": f32(kn), "v_new": f32(K[:, :, :2])},
    }
    rows16 = dict(common(K, lambda t: t), **{
        "cache_bf16": {"k_cache": bf(K), "v_cache": bf(K)}, "v_cache_bf16": {"v_cache": bf(K)},
        "q_f32+cache_bf16": {"q": f32(q), "k_cache": bf(K), "v_cache": bf(K)},
        "cache_bf16+head_dim_96": {"q": q96, "k_cache": bf(K96), "v_cache": bf(K96)},
        "knew_cache_not_in_place": {"k_cache": Kodd, "v_cache": Kodd, "k_new": kn, "v_new": kn},
        "knew_cache_row_strides": {"k_cache": Kt, "v_cache": K, "k_new": kn, "v_new": kn},
        "knew_dtype+cache_not_in_place": {"k_cache": Kodd, "v_cache": Kodd, "k_new": f32(kn), "v_new": f32(kn)}})
    rows8 = dict(common(K, lambda t: t.to(F8)), **{
        "kdescale_f64": {"k_descale": ones(1, 1).double()}, "kdescale_shape": {"k_descale": ones(2)},
        "kdescale_grad": {"k_descale": ones(1).requires_grad_(True)},
        "kdescale_cpu": {"k_descale": torch.ones(1)}, "vdescale_f64": {"v_descale": ones(1).double()},
        "vdescale_shape": {"v_descale": ones(2, 1)}, "vdescale_cpu": {"v_descale": torch.ones(1, 1)},
        "seqlens_int64+kdescale_f64": {"cache_seqlens": sl.long(), "k_descale": ones(1).double()},
        "kdescale_cpu+vdescale_f64": {"k_descale": torch.ones(1), "v_descale": ones(1).double()},
        "vdescale_shape+knew_rank": {"v_descale": ones(2, 1), "k_new": kn[0], "v_new": kn[0]},
        "knew_cache_not_in_place": {"k_cache": K8odd, "v_cache": K8odd, "k_new": kn, "v_new": kn},
        "knew_cache_row_strides": {"k_cache": Kt8, "v_cache": K8, "k_new": kn, "v_new": kn}})
    d16 = {"q": q, "k_cache": K, "v_cache": K, "cache_seqlens": sl}
    d8 = {"q": q, "k_cache": K8, "v_cache": K8, "cache_seqlens": sl}
    grad = lambda t: t.clone().requires_grad_(True)
    ext_only = {"grad_q": {"q": grad(q)}, "grad_q+knew_rank": {"q": grad(q), "k_new": kn[0], "v_new": kn[0]},
                "seqlens_shape+grad_q": {"q": grad(q), "cache_seqlens": z(2, dtype=torch.int32)}}
    py_only = {"knew_alone": {"k_new": kn}, "vnew_alone": {"v_new": kn}, "knew_alone+q_f32": {"k_new": kn, "q": f32(q)}}
    py_scale = {"scale_zero": {"softmax_scale": 0.0}, "scale_neg": {"softmax_scale": -1.0},
                "knew_alone+scale_neg": {"k_new": kn, "softmax_scale": -1.0}, "scale_neg+q_f32": {"softmax_scale": -1.0, "q": f32(q)}}
    sink_rows = {"sinks_cpu": {"sinks": torch.ones(2)}, "sinks_grad": {"sinks": ones(2).requires_grad_(True)},
                 "sinks_grad+q_f32": {"sinks": ones(2).requires_grad_(True), "q": f32(q)},
                 "sinks_grad+cpu_seqlens": {"sinks": ones(2).requires_grad_(True), "cache_seqlens": sl.cpu()}}
    slope_rows = {"slopes_cpu": {"alibi_slopes": torch.ones(2)}, "slopes_cpu+cpu_seqlens": {"alibi_slopes": torch.ones(2), "cache_seqlens": sl.cpu()},
                  "slopes_cpu+q_f32": {"alibi_slopes": torch.ones(2), "q": f32(q)}}
    for prefix, mod, names, py in (("M", M, ("flash_attention_kvcache", "flash_attention_kvcache_softcap", "flash_attention_kvcache_alibi",
                                            "flash_attention_kvcache_sink", "flash_attention_kvcache_fp8", "flash_attention_kvcache_fp8_sink"), True),
                                   ("ext", ext, ("kvcache_forward", "kvcache_softcap_forward", "kvcache_alibi_forward",
                                                 "kvcache_sink_forward", "kvcache_fp8_forward", "kvcache_fp8_sink_forward"), False)):
        for name in names:
            fp8 = "fp8" in name
            base, rows = (dict(d8), dict(rows8)) if fp8 else (dict(d16), dict(rows16))
            rows.update(py_only if py else ext_only)
            if py and name in ("flash_attention_kvcache", "flash_attention_kvcache_fp8"):
                rows.update(py_scale)     # the other wrappers check the scale in front of is_cuda (CPU table)
            if py and name == "flash_attention_kvcache_fp8":     # flash_attention_kvcache lets inf through to the C ABI
                rows["scale_inf"] = {"softmax_scale": INF}
            if "softcap" in name:
                base["softcap"] = 30.0
            if "alibi" in name:
                base["alibi_slopes"] = ones(2)
                rows.update(slope_rows)
            if "sink" in name:
                base["sinks"] = ones(2)
                rows.update(sink_rows)
            _rows(T, "%s.%s" % (prefix, name), getattr(mod, name), base, rows)
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


def _load(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)


def main(argv):
    out = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN     # another directory: leave the fixtures alone
    got = {"host_surface.json": surface(), "host_errors.json": {"cpu": errors(cpu_cases())}}
    old = _load("host_errors.json") if os.path.exists(os.path.join(GOLDEN, "host_errors.json")) else {}
    # the GPU table is recorded where there is a GPU; elsewhere the committed one is kept
    got["host_errors.json"]["gpu"] = errors(gpu_cases()) if torch.cuda.is_available() else old.get("gpu", {})
    if "--check" in argv:
        bad = [n for n in got if not os.path.exists(os.path.join(GOLDEN, n)) or _load(n) != got[n]]
        print("differs: %s" % ", ".join(bad) if bad else "fixtures match this tree")
        return 1 if bad else 0
    for n, data in got.items():
        with open(os.path.join(out, n), "w") as fh:
            json.dump(data, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote %s" % os.path.join(os.path.relpath(out, ROOT), n))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
