"""CPU tests of the grouped-query attention (GQA) boundary: include/mi355fa_gqa.h declares exactly three entry points and
MI355FA_ERR_GROUP, libmi355fa.so exports them, bad arguments are refused before anything is launched, and the Python
surface is as documented; the fp64 GQA references the GPU tests trust (fa_oracle.attention_fp64_chunked and
attn_ref.attention_fp64, with their group sums) agree with torch.autograd at head groups that are no power of two.  No compute
is launched here (no GPU)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT


def _gqa_header_functions():
    txt = open(os.path.join(ROOT, "include", "mi355fa_gqa.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fa_[a-z_]+)\s*\(", txt)))


def test_companion_header_declares_the_three_gqa_entry_points():
    assert _gqa_header_functions() == ["fa_bwd_dkv_gqa", "fa_bwd_dq_gqa", "fa_fwd_gqa"]
    txt = open(os.path.join(ROOT, "include", "mi355fa_gqa.h")).read()
    assert '#include "mi355fa_local.h"' in txt
    assert re.search(r"#define\s+MI355FA_ERR_GROUP\s+\(-8\)", txt)
    # H_kv follows H in every signature
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in _gqa_header_functions():
        sig = body[body.index(name + "("):]
        sig = sig[:sig.index(";")]
        assert re.search(r"int H, int H_kv, int S_q", sig), name


def test_library_exports_the_gqa_entry_points():
    import _mi355fa as fa
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in _gqa_header_functions():
        assert hasattr(raw, name), name
        assert name in fa.SIGNATURES, "python binding misses " + name
    assert fa.ERR_GROUP == -8
    assert fa.lib.fa_abi_version() == 7


def _ptr():
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_bad_arguments_are_refused_before_launch():
    import _mi355fa as fa
    L = fa.lib
    _buf, p = _ptr()
    B, Sq, Sk = 1, 8, 8

    def calls(H, Hkv, D, wl, wr, opts=None, q=p):
        return (
            L.fa_fwd_gqa(q, p, p, p, p, B, H, Hkv, Sq, Sk, D, fa.BF16, 0.125, wl, wr, opts, None),
            L.fa_bwd_dq_gqa(q, p, p, p, p, p, p, p, B, H, Hkv, Sq, Sk, D, fa.FP16, 0.125, wl, wr, opts, None),
            L.fa_bwd_dkv_gqa(q, p, p, p, p, p, p, p, B, H, Hkv, Sq, Sk, D, fa.FP16, 0.125, wl, wr, opts, None),
        )

    for rc in calls(4, 0, 64, -1, -1):
        assert rc == fa.ERR_GROUP                                         # H_kv = 0
    assert b"H_kv" in L.fa_last_error()
    for rc in calls(4, -2, 64, -1, 0):
        assert rc == fa.ERR_GROUP
    for rc in calls(6, 4, 64, -1, 0):
        assert rc == fa.ERR_GROUP                                         # H % H_kv != 0
    for rc in calls(4, 2, 64, -2, 0):
        assert rc == fa.ERR_WINDOW                                        # a window below -1
    for rc in calls(4, 2, 64, 3, -5):
        assert rc == fa.ERR_WINDOW
    for rc in calls(4, 2, 96, -1, 0):
        assert rc == -3                                                   # MI355FA_ERR_HEAD_DIM
    for rc in calls(4, 2, 64, -1, 0, q=None):
        assert rc == -1                                                   # MI355FA_ERR_NULL
    drop = fa.Opts.make(p_drop=0.25, seed=1)
    for fn_rc in zip(calls(4, 2, 64, -1, -1, opts=ctypes.byref(drop)), ("fwd", "dq", "dkv")):
        assert fn_rc[0] == -2, fn_rc                                      # dropout: MI355FA_ERR_SHAPE
    assert b"dropout" in L.fa_last_error() and b"grouped-query" in L.fa_last_error()
    bad = fa.Opts.make()
    bad.size = 4
    for rc in calls(4, 2, 64, -1, 0, opts=ctypes.byref(bad)):
        assert rc == -2                                                   # options as for fa_*_ex
    # a stride that is not a multiple of 8 elements, on K (described as [B, H_kv, S_k, D])
    kst = (ctypes.c_longlong * 3)(2 * Sk * 64, Sk * 64, 65)
    st = fa.Opts.make(k_strides=ctypes.cast(kst, ctypes.POINTER(ctypes.c_longlong)))
    assert L.fa_fwd_gqa(p, p, p, p, p, B, 4, 2, Sq, Sk, 64, fa.BF16, 0.125, -1, 0, ctypes.byref(st), None) == -6


def test_existing_entry_points_still_refuse_fewer_kv_heads():
    import My_FlashAttention_optimized as M
    Q = torch.zeros(1, 4, 8, 64, dtype=torch.float16)
    K = torch.zeros(1, 2, 8, 64, dtype=torch.float16)
    with pytest.raises(AssertionError):
        M._check_qkv(Q, K, K)


def test_python_surface():
    import My_FlashAttention_optimized as M
    import _mi355fa_torch as ext
    assert str(inspect.signature(M.flash_attention_gqa)) == (
        "(Q, K, V, is_causal=False, window_size=(-1, -1), cu_seqlens_q=None, cu_seqlens_k=None, "
        "max_seqlen_q=None, max_seqlen_k=None)")
    assert hasattr(M, "FlashAttentionGQAFunction")
    for name in ("flash_attention_gqa", "gqa_forward_launch", "gqa_backward_launch"):
        assert hasattr(ext, name), name


def test_python_refuses_bad_shapes_and_causal_with_a_right_window():
    import My_FlashAttention_optimized as M
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    Q = mk(2, 8, 16, 64)
    cases = [
        (Q, mk(1, 2, 16, 64), mk(1, 2, 16, 64), {}),                        # batch mismatch
        (Q, mk(2, 2, 16, 128), mk(2, 2, 16, 128), {}),                      # head dim mismatch
        (Q, mk(2, 3, 16, 64), mk(2, 3, 16, 64), {}),                        # 8 % 3 != 0
        (Q, mk(2, 2, 16, 64), mk(2, 4, 16, 64), {}),                        # K and V differ
        (Q, mk(2, 2, 16, 64), mk(2, 2, 16, 64), {"is_causal": True, "window_size": (-1, 4)}),
        (Q, mk(2, 2, 16, 64), mk(2, 2, 16, 64), {"window_size": (-3, 0)}),
    ]
    for q, k, v, kw in cases:
        with pytest.raises(AssertionError):
            M.flash_attention_gqa(q, k, v, **kw)
    # is_causal with window_right 0 or -1 is the causal window
    assert M._gqa_window(True, (-1, -1)) == (-1, 0)
    assert M._gqa_window(True, (100, 0)) == (100, 0)
    assert M._gqa_window(False, (7, 3)) == (7, 3)


def test_cpp_binding_accepts_grouped_shapes_and_refuses_others():
    """The C++ function's own checks (no device needed): grouped shapes pass them and stop only at the device check."""
    import _mi355fa_torch as ext
    mk = lambda *s: torch.zeros(*s, dtype=torch.float16)
    cu = {"cu_seqlens_q": torch.zeros(3, dtype=torch.int32), "cu_seqlens_k": torch.zeros(3, dtype=torch.int32),
          "max_seqlen_q": 4, "max_seqlen_k": 4}
    cases = [((mk(2, 8, 16, 64), mk(2, 2, 16, 64), mk(2, 2, 16, 64)), {}, "device tensors"),
             ((mk(2, 8, 16, 64), mk(2, 1, 16, 64), mk(2, 1, 16, 64)), {}, "device tensors"),
             ((mk(10, 8, 64), mk(12, 2, 64), mk(12, 2, 64)), cu, "device tensors"),
             ((mk(2, 8, 16, 64), mk(2, 3, 16, 64), mk(2, 3, 16, 64)), {}, "multiple"),
             ((mk(10, 8, 64), mk(12, 3, 64), mk(12, 3, 64)), cu, "multiple"),
             ((mk(2, 8, 16, 64), mk(1, 2, 16, 64), mk(1, 2, 16, 64)), {}, "batch"),
             ((mk(2, 8, 16, 64), mk(2, 2, 16, 64), mk(2, 2, 16, 64)), {"cu_seqlens_q": cu["cu_seqlens_q"]}, "together")]
    for args, kw, msg in cases:
        with pytest.raises(AssertionError, match=msg):
            ext.flash_attention_gqa(*args, -1, 0, **kw)


@pytest.mark.parametrize("H,Hkv", [(6, 2), (7, 1), (12, 2)], ids=["g3", "g7-mqa", "g6"])
def test_fp64_references_agree_with_autograd_at_odd_groups(H, Hkv):
    """The closed-form fa_oracle.attention_fp64_chunked and attn_ref.attention_fp64 against autograd through plain fp64
    attention on repeat_interleave'd K / V, whose backward sums dK / dV over each group (fp64, CPU)."""
    import attn_ref
    import fa_oracle as fo
    B, Sq, Sk, D = 2, 11, 17, 8
    g = H // Hkv
    gen = torch.Generator().manual_seed(H + Hkv)
    Q, dO = (torch.randn(B, H, Sq, D, generator=gen, dtype=torch.float64) for _ in range(2))
    K, V = (torch.randn(B, Hkv, Sk, D, generator=gen, dtype=torch.float64) for _ in range(2))
    for wl, wr in ((-1, -1), (-1, 0), (3, 0), (2, 2)):
        q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
        s = (q @ k.repeat_interleave(g, 1).transpose(-1, -2)) * D ** -0.5
        s = s.masked_fill(~fo.visible_mask(Sq, Sk, (wl, wr)), -torch.inf)
        o = torch.softmax(s, -1) @ v.repeat_interleave(g, 1)
        o.backward(dO)
        want = dict(O=o.detach(), LSE=torch.logsumexp(s.detach(), -1), dQ=q.grad, dK=k.grad, dV=v.grad)
        assert k.grad.shape == K.shape
        for name, ref in (("chunked", fo.attention_fp64_chunked(Q, K, V, dO, window=(wl, wr))),
                          ("attn_ref", attn_ref.attention_fp64(Q, K, V, dO, D ** -0.5, attn_ref.visible(Sq, Sk, wl, wr, "cpu")))):
            for n, t in want.items():
                assert torch.allclose(ref[n], t, rtol=1e-10, atol=1e-10), (name, n, wl, wr, (ref[n] - t).abs().max().item())
