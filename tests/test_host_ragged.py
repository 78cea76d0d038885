"""CPU tests of the packed-variable-length decoding boundary: include/mi355fa_ragged.h declares exactly two entry points and
MI355FA_ERR_RAGGED (-13); libmi355fa.so and the ctypes tables export them (a table of their own, RAGGED_SIGNATURES, as
every companion header has); the ABI version and the older headers are untouched; every refusal is reported before
anything is launched; the workspace is the header's formula; the bound NB_max the grid is sized by holds for every split of
total_q into B lengths; the Python function refuses what it must; and the tests' own pack / unpack helpers
(tests/raggedcheck.py) agree with a hand-written loop.  No compute is launched here (no GPU)."""
import ctypes
import os
import random
import re

import pytest
import torch

from conftest import ROOT
import raggedcheck as rc
import variantcheck as vck

HDR = os.path.join(ROOT, "include", "mi355fa_ragged.h")
NAMES = ["fa_fwd_kvcache_ragged", "fa_fwd_kvcache_ragged_workspace_bytes"]


def _lib():
    import _mi355fa as fa
    return fa


def test_header_declares_the_ragged_entry_points():
    txt, body, functions = vck.header_functions(HDR)
    assert functions == NAMES
    assert re.search(r"#define\s+MI355FA_ERR_RAGGED\s+\(-13\)", body)
    assert re.search(r'#include\s+"mi355fa_paged.h"', body) and "mi355fa_paged_mods" in body
    assert "typedef" not in body and "fa_debug" not in txt                 # the mods struct is the paged header's
    # the older headers are as they were: ABI 7, the paged header still declares exactly its two functions and -12
    paged = vck.header_functions(os.path.join(ROOT, "include", "mi355fa_paged.h"))
    assert paged[2] == ["fa_fwd_kvcache_paged", "fa_fwd_kvcache_paged_workspace_bytes"]
    assert re.search(r"#define\s+MI355FA_ERR_PAGED\s+\(-12\)", paged[1])
    assert re.search(r"#define\s+MI355FA_ABI_VERSION\s+7\b", open(os.path.join(ROOT, "include", "mi355fa.h")).read())
    for older in ("mi355fa.h", "mi355fa_kvcache.h", "mi355fa_kvcache_fp8.h", "mi355fa_sink.h", "mi355fa_paged.h"):
        assert "ragged" not in open(os.path.join(ROOT, "include", older)).read().lower(), older


def test_library_and_ctypes_export_the_ragged_entry_points():
    fa = _lib()
    raw = ctypes.CDLL(fa.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in fa.RAGGED_SIGNATURES and name in fa.ALL_SIGNATURES, name
        assert name not in fa.SIGNATURES and name not in fa.PAGED_SIGNATURES, name
    assert len(fa.RAGGED_SIGNATURES["fa_fwd_kvcache_ragged"][1]) == 29
    assert len(fa.RAGGED_SIGNATURES["fa_fwd_kvcache_ragged_workspace_bytes"][1]) == 8
    assert fa.ERR_RAGGED == -13 and fa.ERR_PAGED == -12
    assert fa.lib.fa_abi_version() == 7 and fa.ABI_VERSION == 7


def _call(fa, p, **over):
    """One otherwise well-formed packed call (11 rows over B 3, H 8, H_kv 2, 6 pages of 64 keys per sequence, D 64, bf16,
    every pointer p) with the arguments of `over` replaced; mods: a dict of mi355fa_paged_mods members."""
    a = dict(q=p, kp=p, vp=p, kn=None, vn=None, cu=p, sl=p, bt=p, o=p, ws=p, wsb=1 << 20, T=11, B=3, H=8, Hkv=2, NP=100,
             page=64, MP=6, bts=6, D=64, dt=fa.BF16, cdt=fa.PAGED_CACHE_16BIT, scale=0.125, wl=-1, wr=-1, mods=None, opts=None)
    a.update(over)
    mods = None
    if a["mods"] is not None:
        mods = ctypes.byref(fa.PagedMods(**a["mods"]))
    return fa.lib.fa_fwd_kvcache_ragged(a["q"], a["kp"], a["vp"], a["kn"], a["vn"], a["cu"], a["sl"], a["bt"], a["o"], None,
                                        a["ws"], a["wsb"], a["T"], a["B"], a["H"], a["Hkv"], a["NP"], a["page"], a["MP"],
                                        a["bts"], a["D"], a["dt"], a["cdt"], a["scale"], a["wl"], a["wr"], mods, a["opts"],
                                        None)


def test_refusals_come_before_launch():
    fa = _lib()
    L = fa.lib
    _buf, p = vck.aligned_ptr()
    S3 = lambda *s: ctypes.cast((ctypes.c_longlong * 3)(*s), ctypes.POINTER(ctypes.c_longlong))
    for n in (1, 4):   # without and with partials in the workspace: the plan needs one either way
        vck.splits(n)
        try:
            assert _call(fa, p, cu=None) == -1 and b"cu_seqlens_q" in L.fa_last_error()       # MI355FA_ERR_NULL
            for T in (0, -1, -11):
                assert _call(fa, p, T=T) == fa.ERR_RAGGED and b"total_q" in L.fa_last_error(), T
            for B in (0, -3):
                assert _call(fa, p, B=B) == fa.ERR_RAGGED and b"B must be" in L.fa_last_error(), B
            assert _call(fa, p, T=(1 << 24) // 8 + 1) == fa.ERR_RAGGED                         # H * total_q beyond 2^24
            # a row or head stride of q / o off 16 bytes, a row stride below D, an output whose heads share memory
            keep = []
            for which in ("q_strides", "o_strides"):
                for st in ((0, 64, 8 * 64 + 4), (0, 64 + 2, 8 * 64), (0, 64, 56), (0, -64, 8 * 64), (0, 64, 1 << 30)):
                    keep.append(S3(*st))
                    assert _call(fa, p, opts=ctypes.byref(fa.Opts.make(**{which: keep[-1]}))) == fa.ERR_RAGGED, (which, st)
                    assert b"strides of packed q / o" in L.fa_last_error()
            keep.append(S3(0, 0, 8 * 64))
            assert _call(fa, p, opts=ctypes.byref(fa.Opts.make(o_strides=keep[-1]))) == fa.ERR_RAGGED
            for off in (1, 2, 3):
                assert _call(fa, p, cu=p + off) == -5 and b"cu_seqlens_q" in L.fa_last_error()   # MI355FA_ERR_ALIGN
            assert _call(fa, p, kn=p) == -1 and _call(fa, p, vn=p) == -1                         # k_new without v_new
            assert b"k_new and v_new" in L.fa_last_error()
            # the refusals of the paged header, with its codes
            assert _call(fa, p, bt=None) == -1 and b"block_table" in L.fa_last_error()
            for page in (16, 48, 0, -32, 33):
                assert _call(fa, p, page=page) == fa.ERR_PAGED, page
            for kw in ({"NP": 0}, {"MP": 0}, {"bts": 5}, {"bts": 0}):
                assert _call(fa, p, **kw) == fa.ERR_PAGED, kw
            assert _call(fa, p, bt=p + 2) == -5
            for mods in ({"k_descale": p}, {"v_descale": p}, {"descale_bstride": 2}):
                assert _call(fa, p, mods=mods) == fa.ERR_PAGED, mods
            assert _call(fa, p, cdt=2) == -4
            for mods in ({"softcap": 30.0, "sinks": p}, {"softcap": 30.0, "alibi_slopes": p}, {"alibi_slopes": p, "sinks": p}):
                assert _call(fa, p, mods=mods) == fa.ERR_PAGED, mods
            for mods in ({"softcap": 30.0}, {"alibi_slopes": p}):
                assert _call(fa, p, cdt=fa.PAGED_CACHE_FP8_E4M3, mods=mods) == fa.ERR_PAGED, mods
            for cap in (-1.0, float("nan"), float("inf"), -0.0):
                assert _call(fa, p, mods={"softcap": cap}) == fa.ERR_SOFTCAP, cap
            assert _call(fa, p, mods={"sinks": p + 2}) == -5
            assert _call(fa, p, mods={"alibi_slopes": p, "slopes_batch_stride": 3}) == fa.ERR_ALIBI
            assert _call(fa, p, cdt=fa.PAGED_CACHE_FP8_E4M3, mods={"k_descale": p, "descale_bstride": 1}) == -2
            # and kvcache_impl's
            for kw in ({"q": None}, {"kp": None}, {"vp": None}, {"sl": None}, {"o": None}):
                assert _call(fa, p, **kw) == -1, kw
            for kw in ({"scale": 0.0}, {"scale": float("nan")}, {"H": 0, "Hkv": 1}):
                assert _call(fa, p, **kw) == -2, kw
            assert _call(fa, p, D=96) == -3 and _call(fa, p, dt=2) == -4
            assert _call(fa, p, Hkv=3) == fa.ERR_GROUP and _call(fa, p, wl=-2) == fa.ERR_WINDOW
            assert _call(fa, p, q=p + 8) == -5 and _call(fa, p, o=p + 8) == -5 and _call(fa, p, ws=p + 8) == -5
            # the workspace: never 0 (the plan), refused one byte short and when absent
            need = L.fa_fwd_kvcache_ragged_workspace_bytes(11, 3, 8, 2, 6, 64, 64, fa.PAGED_CACHE_16BIT)
            assert need == rc.workspace_bytes(n, 11, 3, 8, 2, 64) and need >= 32
            assert _call(fa, p, wsb=need - 1) == fa.ERR_WORKSPACE and _call(fa, p, ws=None) == fa.ERR_WORKSPACE
            # the workspace function refuses the same shapes
            W = L.fa_fwd_kvcache_ragged_workspace_bytes
            assert W(0, 3, 8, 2, 6, 64, 64, 0) == fa.ERR_RAGGED and W(11, 0, 8, 2, 6, 64, 64, 0) == fa.ERR_RAGGED
            assert W(11, 3, 8, 2, 6, 48, 64, 0) == fa.ERR_PAGED and W(11, 3, 8, 2, 0, 64, 64, 0) == fa.ERR_PAGED
            assert W(11, 3, 8, 3, 6, 64, 64, 0) == fa.ERR_GROUP and W(11, 3, 8, 2, 6, 64, 96, 0) == -3
            assert W(11, 3, 8, 2, 6, 64, 64, 2) == -4
        finally:
            vck.splits(0)


def _rule(wgs, S_cache, target, keys):
    """the split rules of mi355fa_kvcache.h / mi355fa_kvcache_fp8.h on a count of workgroups per split"""
    n = -(-target // wgs)
    by_len = 1
    while (by_len + 1) ** 2 * keys <= S_cache:
        by_len += 1
    return max(1, min(n, by_len, 64))


def test_workspace_is_the_headers_formula():
    fa = _lib()
    W = fa.lib.fa_fwd_kvcache_ragged_workspace_bytes
    shapes = ((8, 8, 32, 8, 128, 128, 128), (145, 32, 32, 8, 128, 128, 128), (575, 64, 32, 8, 32, 128, 128), (1, 1, 4, 4, 1, 32, 64),
              (17, 300, 8, 1, 3, 32, 64), (2176, 129, 32, 8, 64, 256, 64), (33, 5, 16, 16, 7, 96, 128))
    differ = False
    try:
        for n in (0, 1, 2, 7, 64):
            vck.splits(n)
            for (T, B, H, Hkv, MP, page, D) in shapes:
                got = [W(T, B, H, Hkv, MP, page, D, cdt) for cdt in (fa.PAGED_CACHE_16BIT, fa.PAGED_CACHE_FP8_E4M3)]
                wgs = Hkv * rc.nb_max(H // Hkv, T, B)
                want = [n or _rule(wgs, MP * page, 256, 128), n or _rule(wgs, MP * page, 512 if D == 64 else 256, 64)]
                for g, w in zip(got, want):
                    assert g == rc.workspace_bytes(w, T, B, H, Hkv, D), (n, T, B, H, Hkv, MP, page, D, g, w)
                    assert g % 16 == 0 or w > 1
                differ |= got[0] != got[1]
        assert differ, "the two cache formats follow different split rules somewhere in the table above"
    finally:
        vck.splits(0)


def test_row_block_bound_holds_for_every_partition():
    """NB_max = (g * total_q + 31 * B) // 32 >= sum_b ceil(g * S_b / 32) for lengths summing to at most total_q, zeros
    included: ceil(x / 32) <= (x + 31) / 32 per sequence, summed, and the total is an integer.  Brute force over random
    partitions, and the bound is attained."""
    rnd = random.Random(5)
    tight = 0
    for _ in range(4000):
        B = rnd.choice((1, 2, 3, 8, 31, 64, 257))
        total = rnd.choice((1, 2, 7, 32, 33, 100, 1000, 4097))
        cuts = sorted(rnd.randint(0, total) for _ in range(B))           # B lengths, zeros included, summing to <= total
        if rnd.random() < 0.5:
            cuts[-1] = total
        S = [b - a for a, b in zip([0] + cuts[:-1], cuts)]
        assert len(S) == B and sum(S) <= total and min(S) >= 0
        for g in (1, 2, 4, 8, 16):
            nb, bound = rc.blocks(S, g), rc.nb_max(g, total, B)
            assert nb <= bound, (S, g, total, nb, bound)
            tight += nb == bound
    assert tight > 0
    assert rc.blocks([1] * 8, 4) == 8 and rc.nb_max(4, 8, 8) == 8           # pure decode, g = 4: every workgroup has rows
    assert rc.blocks([2048] + [1] * 128, 4) == 384 and rc.nb_max(4, 2176, 129) == 396


def _args(page=64, dtype=torch.bfloat16, cache_dtype=None):
    B, H, Hkv, D, NP, MP, T = 2, 4, 2, 64, 8, 3, 5
    kc = torch.zeros(NP, Hkv, page, D, dtype=cache_dtype or dtype)
    return dict(q=torch.zeros(T, H, D, dtype=dtype), k_cache=kc, v_cache=kc.clone(),
                cu_seqlens_q=torch.tensor([0, 2, 5], dtype=torch.int32), cache_seqlens=torch.zeros(B, dtype=torch.int32),
                block_table=torch.zeros(B, MP, dtype=torch.int32))


def test_python_wrapper_refuses_what_it_must():
    """Every refusal below is reached on the CPU: the wrapper checks cu_seqlens_q, the table, out, the combinations and the
    gradients before the first device check, which is cu_seqlens_q's own."""
    import ragged_kvcache as R
    f = R.flash_attention_kvcache_ragged
    one = torch.ones(4)

    def refused(what, **over):
        kw = _args(**{k: over.pop(k) for k in ("page", "cache_dtype") if k in over})
        kw.update(over)
        with pytest.raises(AssertionError, match=what):
            f(**kw)

    a = _args()
    refused("cu_seqlens_q must be a device tensor")               # everything else in order: the host tensor is what is left
    refused("cu_seqlens_q must be int32", cu_seqlens_q=a["cu_seqlens_q"].to(torch.int64))
    refused("cu_seqlens_q must be a vector of B \\+ 1 entries", cu_seqlens_q=a["cu_seqlens_q"].view(1, 3))
    refused("cu_seqlens_q must be a vector of B \\+ 1 entries", cu_seqlens_q=a["cu_seqlens_q"][:1])
    refused("cu_seqlens_q must be a tensor", cu_seqlens_q=[0, 2, 5])
    refused("block_table must be int32", block_table=a["block_table"].to(torch.int64))
    refused("block_table must be \\[B, max_pages_per_seq\\] with B = 2", block_table=torch.zeros(3, 3, dtype=torch.int32))
    refused("cache_seqlens must have B = 2 entries", cache_seqlens=torch.zeros(3, dtype=torch.int32))
    refused("q must be \\[total_q, H, D\\]", q=a["q"][None])
    refused("multiple of 32", page=48)
    refused("out must have q's shape", out=torch.zeros(6, 4, 64, dtype=torch.bfloat16))
    refused("out must have q's shape", out=torch.zeros(5, 4, 128, dtype=torch.bfloat16))
    refused("out must have q's dtype", out=torch.zeros(5, 4, 64, dtype=torch.float16))
    refused("out must be a tensor", out=[1])
    refused("at most one of softcap, alibi_slopes and sinks", softcap=30.0, sinks=one)
    refused("at most one of softcap, alibi_slopes and sinks", alibi_slopes=one, sinks=one)
    refused("an fp8 cache takes sinks only: softcap", cache_dtype=torch.float8_e4m3fn, softcap=30.0)
    refused("an fp8 cache takes sinks only: alibi_slopes", cache_dtype=torch.float8_e4m3fn, alibi_slopes=one)
    refused("k_descale / v_descale belong to a torch.float8_e4m3fn cache", k_descale=torch.ones(2))
    refused("softcap must be finite and > 0", softcap=0.0)
    refused("softmax_scale must be finite and > 0", softmax_scale=-1.0)
    refused("is_causal=True with window_right > 0", is_causal=True, window_size=(-1, 3))
    refused("k_new and v_new must be given together", k_new=torch.zeros(5, 2, 64, dtype=torch.bfloat16))
    refused("has no backward: q must not require grad", q=a["q"].clone().requires_grad_(True))
    refused("has no backward: k_cache must not require grad", k_cache=a["k_cache"].clone().requires_grad_(True))
    kn = torch.zeros(5, 2, 64, dtype=torch.bfloat16)
    refused("has no backward: k_new must not require grad", k_new=kn.clone().requires_grad_(True), v_new=kn)
    refused("has no backward: sinks must not require grad", sinks=one.clone().requires_grad_(True))
    refused("has no backward: out must not require grad", out=a["q"].clone().requires_grad_(True))
    # the public surface of the module is the one function, and the older surfaces are as they were
    assert R.__all__ == ["flash_attention_kvcache_ragged"]
    import paged_kvcache as P
    assert P.__all__ == ["flash_attention_kvcache_paged"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_pack_and_unpack_agree_with_a_hand_written_loop(dtype):
    H, D, S, pad = 3, 8, [0, 1, 3, 0, 5], 4
    g = torch.Generator().manual_seed(2)
    per = [torch.randn(1, H, s, D, generator=g).to(dtype) for s in S]
    total = sum(S) + pad
    cu = rc.cu_of(S)
    assert cu.dtype == torch.int32 and cu.tolist() == [0, 0, 1, 4, 4, 9]
    q = rc.pack(per, total)
    assert q.shape == (total, H, D) and q.dtype == dtype and q.is_contiguous()
    for b, s in enumerate(S):
        for i in range(s):
            for h in range(H):
                assert torch.equal(q[int(cu[b]) + i, h], per[b][0, h, i]), (b, i, h)
    assert torch.isnan(q[int(cu[-1]):].float()).all() and not torch.isnan(q[:int(cu[-1])].float()).any()
    assert (rc.pack(per, total, fill=7.0)[int(cu[-1]):] == 7).all()
    back = rc.unpack(q, S)
    assert [t.shape for t in back] == [(1, H, s, D) for s in S]
    assert all(torch.equal(x, y) for x, y in zip(back, per))
    lse = torch.arange(H * total, dtype=torch.float32).view(H, total)
    for b, t in enumerate(rc.unpack_lse(lse, S)):
        assert t.shape == (1, H, S[b])
        for i in range(S[b]):
            for h in range(H):
                assert float(t[0, h, i]) == h * total + int(cu[b]) + i
