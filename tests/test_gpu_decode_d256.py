"""GPU tests of head dim 256 on the decode path (run with -m gpu on an MI355X): the padded, paged and packed calls over 16-bit
and e4m3 caches, every score variant.  At D = 256 a workgroup's four waves are two key groups x two halves of the head
dim and the two waves of a pair add their halves of the scores through LDS (csrc/fa_decode_body.inc, "D = 256"), so beside
the checks the other head dims get -- fp64 parity under the project's tolerances, bit identity across the three layouts and
across repeats, the appends byte for byte, graph replay -- there are inputs whose energy sits in one half of the head dim
only, which a swapped, dropped or doubly counted half cannot pass, and fill levels that give a split 0, 1, 2, 3, an odd and
an even number of 32-key tiles, so that both pairs meet a step with a tile and a step without one.

Tolerances (the project's own): fp16 relFro < 1e-3 against attn_ref's fp64 attention; bf16 < max(2 x PyTorch's bf16 SDPA on
the same problem, 4e-3); LSE rtol 1e-3 / atol 2e-3 with -inf exactly on the keyless rows (test_gpu_kvcache.tol / check_lse);
e4m3 caches test_gpu_kvcache_fp8's; the score variants variantcheck.decode_case's with their files' REL and LSE_BOUND."""
import pytest
import torch

import attn_ref as ar
import blockcheck as bc
import pagedcheck as pc
import test_gpu_alibi as tal
import test_gpu_kvcache as tk
import test_gpu_kvcache_fp8 as tk8
import test_gpu_paged as tpg
import test_gpu_ragged as trg
import test_gpu_sink as tsk
import test_gpu_softcap as tsc
import variantcheck as vck

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
D = 256
SC = 704
FILLS = [0, 1, 31, 32, 33, 64, 65, 96, 129, 300, 687]   # 0, 1, 2, 3, 5, 10 and 22 tiles: odd and even shares at every split count
SPLITS = (0, 1, 2, 3, 7)                                 # 7: more splits than tiles for most of the fill levels
GROUPS = [(4, 4), (8, 2), (8, 1), (6, 2)]                # (6, 2): an odd group


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def nan_padded(q, kc, vc, lens):
    for b, L in enumerate(lens):
        kc[b, :, L:] = float("nan")
        vc[b, :, L:] = float("nan")
    return q, kc, vc


def check_padded(q, kc, vc, lens, masks=tk.MASKS, splits=SPLITS, what=()):
    """flash_attention_kvcache on a NaN-padded cache at every mask and forced split count against fp64 under tk.tol and
    tk.check_lse; keyless rows are O = 0; every count repeats its own bits."""
    M = vck.M()
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for is_causal, window in masks:
        wl, wr = tk.window_of(is_causal, window)
        O_ref, LSE_ref = tk.ref_fp64(q, kc, vc, lens, wl, wr)
        bound = tk.tol(q.dtype, q, kc, vc, lens, wl, wr, O_ref)
        for n in splits:
            vck.splits(n)
            o, lse = M.flash_attention_kvcache(q, kc, vc, sl, is_causal=is_causal, window_size=window, return_lse=True)
            o2, lse2 = M.flash_attention_kvcache(q, kc, vc, sl, is_causal=is_causal, window_size=window, return_lse=True)
            torch.cuda.synchronize()
            tag = (*what, is_causal, window, n)
            assert torch.isfinite(o).all(), tag                       # NaN past the fill level is never read
            err = tk.rel(o, O_ref)
            assert err < bound, (tag, err, bound)
            tk.check_lse(lse, LSE_ref)
            assert (o[torch.isinf(LSE_ref)] == 0).all(), tag
            assert bc.same_bits(o, o2) and bc.same_bits(lse, lse2), tag
    return bound


# ---- 1. fp64 parity ----------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("Sq", [1, 3, 9, 40])          # with g = 4, S_q = 9 is one full row block and a partial one
@pytest.mark.parametrize("H,Hkv", GROUPS)
def test_padded_call_matches_fp64(H, Hkv, Sq, dtype):
    q, kc, vc = nan_padded(*tk.make(len(FILLS), H, Hkv, Sq, SC, D, dtype, seed=H + Sq), FILLS)
    check_padded(q, kc, vc, FILLS, what=(H, Hkv, Sq))


# ---- 2. one half of the head dim at a time ----------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("trap", ["qk_high", "qk_low", "v_high_zero", "v_low_zero"])
def test_energy_in_one_half_of_the_head_dim(trap, dtype):
    """q and K non-zero in dims [128, 256) only, then in [0, 128) only: the scores come from one wave of each pair alone, and
    a half that is swapped, dropped or counted twice changes every score.  V zero in one half: that half of O is exactly 0
    and the other one is accurate."""
    H, Hkv, lens = 8, 2, [33, 65, 300, 687]
    for Sq in (1, 9):
        q, kc, vc = tk.make(len(lens), H, Hkv, Sq, SC, D, dtype, seed=Sq)
        half = slice(0, 128) if trap in ("qk_high", "v_low_zero") else slice(128, 256)
        if trap.startswith("qk"):
            q[..., half] = 0
            kc[..., half] = 0
            q *= 2 ** 0.5                                   # (the score variance of a full-width problem)
        else:
            vc[..., half] = 0
        nan_padded(q, kc, vc, lens)
        check_padded(q, kc, vc, lens, splits=(1, 2, 3), what=(trap, Sq))
        if trap.startswith("v_"):
            sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
            o = vck.M().flash_attention_kvcache(q, kc, vc, sl)
            assert (o[..., half] == 0).all() and (o[..., slice(128, 256) if half.start == 0 else slice(0, 128)] != 0).any()


# ---- 3. every variant at one small shape ---------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("Sq", [1, 9])
@pytest.mark.parametrize("variant", ["softcap", "alibi"])
def test_score_variants_match_fp64(variant, Sq, dtype):
    M = vck.M()
    if variant == "softcap":
        cap = 30.0
        call = lambda q, kc, vc, sl, **kw: M.flash_attention_kvcache_softcap(q, kc, vc, sl, cap, **kw)
        res = vck.decode_case(call, lambda Ls: dict(cap=cap), dtype, D, Sq, (-1, 0), tsc.REL[dtype], tsc.CAP_MATTERS,
                              tsc.BOUNDS["LSE_BOUND"][dtype], amp=tsc._amp(cap, D ** -0.5, D))
    else:
        slopes = M.alibi_slopes(8, device="cuda") / 8
        call = lambda q, kc, vc, sl, **kw: M.flash_attention_kvcache_alibi(q, kc, vc, sl, slopes, **kw)
        dist = lambda Ls: torch.stack([ar.distance(Sq, vck.DECODE_CACHE, "cuda", L=L) for L in Ls])[:, None]
        res = vck.decode_case(call, lambda Ls: dict(slopes=slopes, dist=dist(Ls)), dtype, D, Sq, (-1, 0), tal.REL[dtype],
                              tal.BIAS_MATTERS, tal.BOUNDS["LSE_BOUND"][dtype])
    for n, err, lerr in res:
        print("decode", variant, dtype, Sq, "splits", n, "O relFro %.2e LSE max %.2e" % (err, lerr))


@DTYPES
@pytest.mark.parametrize("Sq", [1, 9])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_sinks_match_fp64(fp8, Sq, dtype):
    tsk._decode_case(fp8, dtype, D, Sq, (-1, 0), lens=[0, 300, 650], Sc=704, Snew=2, B=3, H=8, Hkv=2, sinks=tsk._sinks(8),
                     splits=(0, 1, 3, 7), seed=D + Sq)


@DTYPES
@pytest.mark.parametrize("Sq", [1, 9])
def test_fp8_cache_matches_fp64(Sq, dtype):
    for n in (0, 1, 3, 7):
        vck.splits(n)
        tk8.run_case(3, 8, 2, Sq, 704, D, dtype, [0, 300, 650], True, (-1, -1), seed=Sq)


@DTYPES
def test_neutral_transforms_give_the_bits_of_the_plain_call(dtype):
    """sinks = -inf and zero slopes, on 16-bit and e4m3 caches"""
    M = vck.M()
    lens, H, Hkv = [0, 300, 650], 8, 2
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ninf, zero = torch.full((H,), float("-inf"), device="cuda"), torch.zeros(H, device="cuda")
    for Sq in (1, 9):
        q, kc, vc = tk.make(3, H, Hkv, Sq, SC, D, dtype, seed=Sq)
        q8, k8, v8, kd, vd = tk8.make8(3, H, Hkv, Sq, SC, D, dtype, lens, seed=Sq)
        for n in (1, 3):
            vck.splits(n)
            kw = dict(is_causal=True, return_lse=True)
            plain = M.flash_attention_kvcache(q, kc, vc, sl, **kw)
            tpg.assert_same(M.flash_attention_kvcache_sink(q, kc, vc, sl, ninf, **kw), plain, ("sink", Sq, n))
            tpg.assert_same(M.flash_attention_kvcache_alibi(q, kc, vc, sl, zero, **kw), plain, ("alibi", Sq, n))
            plain8 = M.flash_attention_kvcache_fp8(q8, k8, v8, sl, kd, vd, **kw)
            tpg.assert_same(M.flash_attention_kvcache_fp8_sink(q8, k8, v8, sl, ninf, kd, vd, **kw), plain8, ("fp8_sink", Sq, n))


# ---- 4. the appends ---------------------------------------------------------------------------------------------------------
@DTYPES
def test_padded_appends_land_byte_for_byte(dtype):
    M = vck.M()
    B, H, Hkv, Sq, Snew, lens = 3, 8, 2, 3, 3, [0, 300, 650]
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    kn, vn = (torch.randn(B, Hkv, Snew, D, generator=g, device="cuda").to(dtype) for _ in range(2))
    q, kc, vc = tk.make(B, H, Hkv, Sq, SC, D, dtype, seed=1)
    kx, vx = kc.clone(), vc.clone()
    for b, L in enumerate(lens):
        kx[b, :, L:L + Snew], vx[b, :, L:L + Snew] = kn[b], vn[b]
    M.flash_attention_kvcache(q, kc, vc, sl, k_new=kn, v_new=vn, is_causal=True)
    torch.cuda.synchronize()
    assert pc.same_bytes(kc, kx) and pc.same_bytes(vc, vx)
    # the quantising append: the bytes of (x.float() / d).clamp(-448, 448).to(float8_e4m3fn)
    q8, k8, v8, kd, vd = tk8.make8(B, H, Hkv, Sq, SC, D, dtype, lens, seed=2)
    kx, vx = k8.clone(), v8.clone()
    quant = lambda x, d: (x.float() / d[:, :, None, None]).clamp(-448, 448).to(tk8.F8)
    for b, L in enumerate(lens):
        tk8.u8(kx)[b, :, L:L + Snew] = tk8.u8(quant(kn, kd))[b]
        tk8.u8(vx)[b, :, L:L + Snew] = tk8.u8(quant(vn, vd))[b]
    M.flash_attention_kvcache_fp8(q8, k8, v8, sl, kd, vd, k_new=kn, v_new=vn, is_causal=True)
    torch.cuda.synchronize()
    assert pc.same_bytes(k8, kx) and pc.same_bytes(v8, vx)


@pytest.mark.parametrize("variant,dtype", [("plain", F16), ("plain", BF16), ("fp8", BF16), ("fp8_sink", F16)])
def test_append_through_the_table_crosses_a_page_boundary(variant, dtype):
    page, H, Hkv, Sq, Snew = 64, 8, 2, 3, 3
    lens = [0, page - 1, page, 2 * page - 2]
    full = [L + Snew for L in lens]
    c = tpg.Case(variant, dtype, D, H, Hkv, Sq, page, lens, seed=17, alloc=full)
    g = torch.Generator(device="cuda").manual_seed(18)
    kn, vn = (torch.randn(len(lens), Hkv, Snew, D, generator=g, device="cuda").to(dtype) for _ in range(2))
    for n in (0, 3):
        vck.splits(n)
        kc, vc, kp, vp = c.kc.clone(), c.vc.clone(), c.kp.clone(), c.vp.clone()
        ref = c.padded(kc, vc, k_new=kn, v_new=vn, is_causal=True)
        got = c.paged(kp, vp, k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        assert not pc.same_bytes(kc, c.kc)
        (kx, vx), _ = pc.scatter([kc, vc], full, page, kp.shape[0], tpg.MAX_PAGES, 0, table=c.table.cpu())
        assert pc.same_bytes(kp, kx) and pc.same_bytes(vp, vx), n
        tpg.assert_same(got, ref, n)
        assert torch.isfinite(got[0]).all()


# ---- 5. the bits across layouts ------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("page", [32, 64, 96])
@pytest.mark.parametrize("variant", tpg.VARIANTS)
def test_paged_call_has_the_bits_of_the_padded_call(variant, page, dtype):
    """a permuted table whose entries past each sequence's last used page are outside the pool"""
    H, Hkv = 8, 2
    for Sq in (1, 9):
        c = tpg.Case(variant, dtype, D, H, Hkv, Sq, page, tpg.lengths(page), seed=Sq + page)
        for b, L in enumerate(c.lens):
            c.table[b, pc.pages_of(L, page):] = (-1, c.kp.shape[0] + 7)[b % 2]
        for is_causal, window in tk.MASKS:
            for n in (0, 1, 3, 7):
                vck.splits(n)
                kw = dict(is_causal=is_causal, window_size=window)
                what = (Sq, is_causal, window, n)
                got = c.paged(**kw)
                assert torch.isfinite(got[0]).all() and not torch.isnan(got[1]).any(), what
                tpg.assert_same(got, c.padded(**kw), what)
                tpg.assert_same(c.paged(**kw), got, what)                 # split determinism


@DTYPES
@pytest.mark.parametrize("page", [32, 64, 96])
@pytest.mark.parametrize("variant", tpg.VARIANTS)
def test_packed_rows_have_the_bits_of_the_paged_call_on_each_sequence(variant, page, dtype):
    S, lens = [0, 1, 9, 3], [300, 0, 2 * page + 5, 40]
    st = trg.Step(variant, dtype, D, 8, 2, S, page, lens, seed=page, max_pages=-(-max(lens) // page))
    tail = sum(S)
    for is_causal, window in tk.MASKS:
        kw = dict(is_causal=is_causal, window_size=window)
        for n in (0, 1, 3, 7):
            vck.splits(n)
            what = (is_causal, window, n)
            got = st.ragged(**kw)
            assert torch.isfinite(got[0][:tail]).all(), what
            trg.assert_rows(st, got, st.per_sequence(**kw), what)       # and the padding rows past cu[B] keep their fill
            again = st.ragged(**kw)
            assert bc.same_bits(again[0], got[0]) and bc.same_bits(again[1][:, :tail], got[1][:, :tail]), what


@DTYPES
def test_transposed_cache_and_fused_qkv_slice_are_read_in_place(dtype):
    M = vck.M()
    B, H, Hkv, Sq, lens = 3, 8, 2, 3, [33, 300, 650]
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    q, kc, vc = tk.make(B, H, Hkv, Sq, SC, D, dtype, seed=3)
    kt, vt = (x.transpose(1, 2).contiguous().transpose(1, 2) for x in (kc, vc))       # [B, S, H_kv, D] storage
    qkv = torch.randn(B, Sq, (H + 2 * Hkv) * D, device="cuda").to(dtype)              # a fused row: q heads, then k, then v
    qv = qkv[:, :, :H * D].view(B, Sq, H, D).transpose(1, 2)
    qv.copy_(q)
    assert not kt.is_contiguous() and not qv.is_contiguous()
    for n in (1, 3):
        vck.splits(n)
        ref = M.flash_attention_kvcache(q, kc, vc, sl, is_causal=True, return_lse=True)
        tpg.assert_same(M.flash_attention_kvcache(qv, kt, vt, sl, is_causal=True, return_lse=True), ref, n)


# ---- 6. graph capture ----------------------------------------------------------------------------------------------------------
def test_graph_captured_step_replays_after_seqlens_advance():
    M = vck.M()
    B, H, Hkv, Sq, Sc = 2, 8, 2, 1, 1024
    q, kc, vc = tk.make(B, H, Hkv, Sq, Sc, D, BF16, seed=5)
    sl = torch.tensor([500, 900], dtype=torch.int32, device="cuda")
    vck.graph_replay(lambda _: M.flash_attention_kvcache(q, kc, vc, sl), sl, [([700, 1000], None), ([1, 1024], None)])


# ---- 7. the training calls keep to 64 and 128 ------------------------------------------------------------------------------------
def test_training_calls_still_refuse_d256():
    M = vck.M()
    q = torch.randn(1, 4, 64, D, device="cuda", dtype=BF16)
    k = torch.randn(1, 2, 64, D, device="cuda", dtype=BF16)
    for call in (lambda: M.flash_attention(q, q, q), lambda: M.flash_attention(q, q, q, is_causal=True),
                 lambda: M.flash_attention_gqa(q, k, k), lambda: M.flash_attention_local(q, q, q, 8, 0),
                 lambda: M.flash_attention_softcap(q, k, k, 30.0), lambda: M.flash_attention_sink(q, k, k, torch.zeros(4, device="cuda"))):
        with pytest.raises((AssertionError, RuntimeError), match="head dim must be 64 or 128"):
            call()
