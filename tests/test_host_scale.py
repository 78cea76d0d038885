"""CPU tests of the softmax-scale check: every C entry point that takes `scale` refuses one that is not finite and > 0
(include/mi355fa.h) with MI355FA_ERR_SHAPE before anything is launched, and fa_last_error names the scale.  The fp16
kernels keep a running maximum of the raw scores, the wrong extreme for a negative scale, and divide by the scale in their
deferred-rescale threshold; none of these values may reach a kernel.  No compute is launched here (no GPU)."""
import ctypes
import math

import pytest

BAD_SCALES = (0.0, -0.0, -0.125, math.nan, math.inf, -math.inf)


def _ptr():
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _calls(p):
    """name -> f(scale): one otherwise well-formed call per entry point (B = 1, H = 2, S = 8, D = 64)."""
    import _mi355fa as fa
    L = fa.lib
    B, H, Hkv, S, D, dt = 1, 2, 1, 8, 64, fa.BF16
    S3 = ctypes.c_longlong * 3
    st = S3(H * S * D, S * D, D)                       # contiguous, spelled out
    cu = (ctypes.c_int * 2)(0, S)
    cu_p = ctypes.addressof(cu)
    sh = (B, H, S, S, D, dt, 0)
    vl = (cu_p, cu_p, 1, H, S, S, S, S, D, dt, 0)
    drop = (0.25, 1, 0)
    opts = fa.Opts.make()
    return {
        "fa_fwd": lambda s: L.fa_fwd(p, p, p, p, p, *sh, s, None),
        "fa_bwd_dq": lambda s: L.fa_bwd_dq(p, p, p, p, p, p, p, p, *sh, s, None),
        "fa_bwd_dkv": lambda s: L.fa_bwd_dkv(p, p, p, p, p, p, p, p, *sh, s, None),
        "fa_fwd_strided": lambda s: L.fa_fwd_strided(p, st, p, st, p, st, p, st, p, *sh, s, None),
        "fa_bwd_dq_strided": lambda s: L.fa_bwd_dq_strided(p, st, p, st, p, st, p, st, p, st, p, p, st, p, *sh, s, None),
        "fa_bwd_dkv_strided": lambda s: L.fa_bwd_dkv_strided(p, st, p, st, p, st, p, st, p, p, p, st, p, st, *sh, s, None),
        "fa_fwd_varlen": lambda s: L.fa_fwd_varlen(p, p, p, p, p, *vl, s, None),
        "fa_bwd_dq_varlen": lambda s: L.fa_bwd_dq_varlen(p, p, p, p, p, p, p, p, *vl, s, None),
        "fa_bwd_dkv_varlen": lambda s: L.fa_bwd_dkv_varlen(p, p, p, p, p, p, p, p, *vl, s, None),
        "fa_fwd_dropout": lambda s: L.fa_fwd_dropout(p, p, p, p, p, *sh, s, *drop, None),
        "fa_bwd_dq_dropout": lambda s: L.fa_bwd_dq_dropout(p, p, p, p, p, p, p, p, *sh, s, *drop, None),
        "fa_bwd_dkv_dropout": lambda s: L.fa_bwd_dkv_dropout(p, p, p, p, p, p, p, p, *sh, s, *drop, None),
        "fa_fwd_ex": lambda s: L.fa_fwd_ex(p, p, p, p, p, *sh, s, ctypes.byref(opts), None),
        "fa_bwd_dq_ex": lambda s: L.fa_bwd_dq_ex(p, p, p, p, p, p, p, p, *sh, s, ctypes.byref(opts), None),
        "fa_bwd_dkv_ex": lambda s: L.fa_bwd_dkv_ex(p, p, p, p, p, p, p, p, *sh, s, ctypes.byref(opts), None),
        "fa_fwd_local": lambda s: L.fa_fwd_local(p, p, p, p, p, B, H, S, S, D, dt, s, 3, 0, None, None),
        "fa_bwd_dq_local": lambda s: L.fa_bwd_dq_local(p, p, p, p, p, p, p, p, B, H, S, S, D, dt, s, 3, 0, None, None),
        "fa_bwd_dkv_local": lambda s: L.fa_bwd_dkv_local(p, p, p, p, p, p, p, p, B, H, S, S, D, dt, s, 3, 0, None, None),
        "fa_fwd_gqa": lambda s: L.fa_fwd_gqa(p, p, p, p, p, B, H, Hkv, S, S, D, dt, s, -1, -1, None, None),
        "fa_bwd_dq_gqa": lambda s: L.fa_bwd_dq_gqa(p, p, p, p, p, p, p, p, B, H, Hkv, S, S, D, dt, s, -1, -1, None, None),
        "fa_bwd_dkv_gqa": lambda s: L.fa_bwd_dkv_gqa(p, p, p, p, p, p, p, p, B, H, Hkv, S, S, D, dt, s, -1, -1, None, None),
        "fa_fwd_kvcache": lambda s: L.fa_fwd_kvcache(p, p, p, None, None, p, p, p, p, 1 << 12, B, H, Hkv, 1, S, 0, D, dt, s,
                                                     -1, -1, None, None),
    }


def test_every_entry_point_with_a_scale_is_covered():
    """The table below names every function of the four public headers whose signature has a `scale` argument."""
    import _mi355fa as fa
    _buf, p = _ptr()
    calls = _calls(p)
    with_scale = set()
    for name, (_, argtypes) in fa.SIGNATURES.items():
        if name.startswith("fa_debug") or name == "fa_dropout_keep_scale":
            continue
        if ctypes.c_float in argtypes and name != "fa_fwd_kvcache_workspace_bytes":
            with_scale.add(name)
    assert with_scale == set(calls), sorted(with_scale ^ set(calls))


@pytest.mark.parametrize("scale", BAD_SCALES, ids=["0", "-0", "-0.125", "nan", "inf", "-inf"])
def test_bad_scale_is_refused_before_launch(scale):
    import _mi355fa as fa
    _buf, p = _ptr()
    calls = _calls(p)
    for name, call in calls.items():
        fa.lib.fa_last_error()
        rc = call(scale)
        assert rc == -2, (name, scale, rc)                               # MI355FA_ERR_SHAPE
        msg = fa.lib.fa_last_error()
        # names the scale and the function (the *_strided forms report under their plain name)
        assert b"scale" in msg and name.encode().startswith(msg.split(b":")[0]), (name, msg)


def test_scale_check_order_and_its_boundaries():
    """A bad scale is reported even when everything else is valid, and a NULL pointer still wins over it (the order of
    the checks is part of what fa_last_error tells a caller)."""
    import _mi355fa as fa
    L = fa.lib
    _buf, p = _ptr()
    assert L.fa_fwd(None, p, p, p, p, 1, 2, 8, 8, 64, 1, 0, math.nan, None) == -1
    assert b"NULL" in L.fa_last_error()
    assert L.fa_fwd(p, p, p, p, p, 1, 2, 8, 8, 64, 1, 0, -1.0, None) == -2
    assert b"scale" in L.fa_last_error()
    # the smallest positive float is finite and > 0: the scale check lets it through (the shape check then refuses B = 0)
    tiny = float.fromhex("0x1p-149")
    assert L.fa_fwd(p, p, p, p, p, 0, 2, 8, 8, 64, 1, 0, tiny, None) == -2
    assert b"scale" not in L.fa_last_error()
    assert L.fa_fwd(p, p, p, p, p, 0, 2, 8, 8, 64, 1, 0, 3.0e38, None) == -2
    assert b"scale" not in L.fa_last_error()
