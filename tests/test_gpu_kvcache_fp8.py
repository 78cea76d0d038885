"""GPU tests of decoding attention over an FP8 (OCP e4m3) KV cache (include/mi355fa_kvcache_fp8.h,
flash_attention_kvcache_fp8), mirroring tests/test_gpu_kvcache.py test for test.  The reference is that file's fp64
attention on the dequantised cache, k_cache.double() * k_descale and v_cache.double() * v_descale, so quantisation error
is not in the comparison: the kernel's operands are exact and it makes the 16-bit kernel's rounding errors only, which is
why the tolerances are that file's, unchanged (fp16 relFro < 1e-3; bf16 < max(2x PyTorch's bf16 SDPA on the dequantised
cache, 4e-3); LSE rtol 1e-3 / atol 2e-3).

The cache data span the format: random data quantised with quantize_kv_fp8 (descales that are no powers of two and differ
per (b, hk) and between K and V), then every subnormal code, +-448 and +-0 planted at fixed places in visible rows of every
head (plant(); asserted to be there)."""
import ctypes

import pytest
import torch

from test_gpu_kvcache import GROUPS, MASKS, check_lse, ref_fp64, rel, sdpa_level, window_of
import variantcheck as vck

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
F8 = torch.float8_e4m3fn
# subnormals 0x01-0x07 / 0x81-0x87, +-448, +-0
SPECIAL = list(range(0x01, 0x08)) + list(range(0x81, 0x88)) + [0x7E, 0xFE, 0x00, 0x80]


def _M():
    import My_FlashAttention_optimized as M
    return M


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def u8(t):
    return t.view(torch.uint8)


def plant(k8, v8, lens):
    """SPECIAL at K[b, hk, r, 0:18] and V[b, hk, r, 20:38] for the rows r = L_b - 1 (visible to the last query under every
    mask) and L_b // 2 of every sequence with L_b >= 1, every head; asserted to be there."""
    codes = torch.tensor(SPECIAL, dtype=torch.uint8, device=k8.device)
    n = len(SPECIAL)
    for b, L in enumerate(lens):
        for r in {L - 1, L // 2} if L >= 1 else ():
            u8(k8)[b, :, r, 0:n] = codes
            u8(v8)[b, :, r, 20:20 + n] = codes
    for b, L in enumerate(lens):
        if L >= 1:
            assert (u8(k8)[b, :, L - 1, 0:n] == codes).all() and (u8(v8)[b, :, L - 1, 20:20 + n] == codes).all()
            sub = (u8(k8)[b, :, :L] & 0x7F).clamp(max=8)
            assert ((sub >= 1) & (sub <= 7)).any(dim=-1).any(dim=-1).all()      # subnormals in every head


def make8(B, H, Hkv, Sq, Sc, D, dtype, lens, seed=0, per_batch=True):
    """q, the quantised caches with SPECIAL planted, and their descales: (B, H_kv), or (H_kv,) with per_batch=False"""
    M = _M()
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32)
    q, k, v = r(B, H, Sq, D).to(dtype), r(B, Hkv, Sc, D), r(B, Hkv, Sc, D) * 1.7
    if per_batch:
        k8, kd = M.quantize_kv_fp8(k)
        v8, vd = M.quantize_kv_fp8(v)
        assert kd.shape == (B, Hkv) and (kd.flatten().unique().numel() == B * Hkv)
    else:
        k8, kd = M.quantize_kv_fp8(k, k.abs().amax(dim=(0, 2, 3)) / 448)
        v8, vd = M.quantize_kv_fp8(v, v.abs().amax(dim=(0, 2, 3)) / 448)
        assert kd.shape == (Hkv,)
    assert not torch.equal(kd, vd)
    frac = torch.frexp(kd)[0]
    assert (frac != 0.5).all()                                                   # no power of two
    plant(k8, v8, lens)
    return q, k8, v8, kd, vd


def deq(x8, d):
    """the dequantised cache in fp64"""
    return x8.double() * d.double().reshape(-1, x8.shape[1], 1, 1)


def tol(dtype, q, K, V, lens, wl, wr, O_ref):
    """test_gpu_kvcache.tol with PyTorch's SDPA run on the dequantised cache in q's dtype"""
    return 1e-3 if dtype == F16 else max(2 * sdpa_level(q, K.to(dtype), V.to(dtype), lens, wl, wr, O_ref), 4e-3)


def check(q, k8, v8, kd, vd, lens, is_causal, window, o, lse, scale=None):
    B, H, Sq, D = q.shape
    wl, wr = window_of(is_causal, window)
    K, V = deq(k8, kd), deq(v8, vd)
    O_ref, LSE_ref = ref_fp64(q, K, V, lens, wl, wr, scale)
    assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == (B, H, Sq) and lse.dtype == torch.float32
    assert torch.isfinite(o).all()
    err, t = rel(o, O_ref), tol(q.dtype, q, K, V, lens, wl, wr, O_ref)
    print("relFro %.3e tol %.3e" % (err, t))
    assert err < t, (err, t)
    check_lse(lse, LSE_ref)
    return O_ref, LSE_ref


def run_case(B, H, Hkv, Sq, Sc, D, dtype, lens, is_causal, window, seed=0, per_batch=True, **kw):
    M = _M()
    q, k8, v8, kd, vd = make8(B, H, Hkv, Sq, Sc, D, dtype, lens, seed, per_batch)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    o, lse = M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd, is_causal=is_causal, window_size=window, return_lse=True, **kw)
    torch.cuda.synchronize()
    O_ref, LSE_ref = check(q, k8, v8, kd, vd, lens, is_causal, window, o, lse, kw.get("softmax_scale"))
    return q, k8, v8, kd, vd, sl, o, lse, O_ref, LSE_ref


@pytest.mark.parametrize("per_batch", [True, False], ids=["descale_BH", "descale_H"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq", [1, 3, 16, 130])
@pytest.mark.parametrize("H,Hkv", GROUPS)
def test_matches_fp64(H, Hkv, Sq, D, dtype, per_batch):
    Sc = 320 if Sq < 130 else 450
    lens = [Sc - 17, 200, 131] if Sq < 130 else [Sc, 300, 200]
    for is_causal, window in MASKS:
        run_case(3, H, Hkv, Sq, Sc, D, dtype, lens, is_causal, window, seed=Sq + D, per_batch=per_batch)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_softmax_scale_is_honoured(dtype):
    run_case(2, 8, 2, 3, 300, 128, dtype, [300, 77], True, (-1, -1), seed=2, softmax_scale=0.2)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_no_descale_is_ones_and_agrees_with_the_16_bit_kernel(D, dtype):
    M = _M()
    B, H, Hkv, Sq, Sc = 3, 16, 4, 3, 700
    lens = [700, 33, 412]
    q, k8, v8, _, _ = make8(B, H, Hkv, Sq, Sc, D, dtype, lens, seed=3)
    # codes as values (descale 1): keep the scores moderate
    u8(k8).bitwise_and_(0xBF)                                                   # |k| < 2
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ones2, ones1 = torch.ones(B, Hkv, device="cuda"), torch.ones(Hkv, device="cuda")
    for is_causal, window in MASKS:
        kw = dict(is_causal=is_causal, window_size=window, return_lse=True)
        a = M.flash_attention_kvcache_fp8(q, k8, v8, sl, **kw)
        for kd, vd in ((ones2, ones2), (ones1, ones1), (None, ones1), (ones2, None), (ones1, ones2)):
            b = M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd, **kw)
            assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])
        check(q, k8, v8, ones2, ones2, lens, is_causal, window, *a)
        c = M.flash_attention_kvcache(q, k8.to(dtype), v8.to(dtype), sl, **kw)
        wl, wr = window_of(is_causal, window)
        O_ref, _ = ref_fp64(q, k8.double(), v8.double(), lens, wl, wr)
        assert rel(a[0], c[0]) < tol(dtype, q, k8.double(), v8.double(), lens, wl, wr, O_ref)
        check_lse(a[1], c[1].double())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_ragged_lengths_and_rows_without_keys(D, dtype):
    lens = [0, 1, 63, 64, 65, 127, 129, 3000]
    for Sq in (1, 5):                                     # S_q = 5 > L_b for L_b in {0, 1}: rows with no visible key
        for is_causal, window in MASKS:
            q, k8, v8, kd, vd, sl, o, lse, O_ref, LSE_ref = run_case(8, 8, 2, Sq, 3072, D, dtype, lens, is_causal, window)
            empty = torch.isinf(LSE_ref)
            assert empty[0].all()                         # L = 0: every row
            if Sq == 5 and is_causal:
                assert empty[1, :, :4].all()              # L = 1: queries 0..3 sit at negative positions
            assert (o[empty] == 0).all()
            assert torch.isneginf(lse[empty]).all()


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_nan_padding_past_the_fill_level_is_never_read(dtype):
    M = _M()
    B, H, Hkv, Sq, Sc, D = 4, 8, 2, 3, 600, 128
    lens = [0, 70, 333, 600]                              # the last one: L_b = S_cache
    q, k8, v8, kd, vd = make8(B, H, Hkv, Sq, Sc, D, dtype, lens, seed=5)
    for b, L in enumerate(lens):
        u8(k8)[b, :, L:] = 0x7F                           # e4m3 NaN
        u8(v8)[b, :, L:] = 0x7F
    assert torch.isnan(k8[1, :, 70:].float()).all()
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for n in (0, 1, 3, 7):
        vck.splits(n)
        for is_causal, window in MASKS:
            o, lse = M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd, is_causal=is_causal, window_size=window, return_lse=True)
            assert torch.isfinite(o).all() and not torch.isnan(lse).any()
            check(q, k8, v8, kd, vd, lens, is_causal, window, o, lse)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_append_quantises_exactly_the_new_rows(D, dtype):
    M = _M()
    B, H, Hkv, Sq, Sc = 4, 8, 2, 4, 520
    lens = [0, 100, 257, 516]                                   # the last one fills the cache to the end
    Snew = 4
    q, k8, v8, kd, vd = make8(B, H, Hkv, Sq, Sc, D, dtype, lens, seed=7)
    g = torch.Generator(device="cuda").manual_seed(8)
    # magnitudes from far below the smallest e4m3 subnormal x descale to far beyond 448 x descale, signed zeros, exact ties
    mag = torch.logspace(-5, 3, D, device="cuda")[torch.randperm(D, generator=g, device="cuda")]
    kn = (torch.randn(B, Hkv, Snew, D, generator=g, device="cuda") * mag).to(dtype)
    vn = (torch.randn(B, Hkv, Snew, D, generator=g, device="cuda") * mag.flip(0)).to(dtype)
    kn[:, :, 0, 0], kn[:, :, 0, 1], vn[:, :, 1, 2], vn[:, :, 1, 3] = 0.0, -0.0, -0.0, 0.0
    k0, v0 = k8.clone(), v8.clone()
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    o, lse = M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd, k_new=kn, v_new=vn, is_causal=True, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(sl.cpu(), torch.tensor(lens, dtype=torch.int32))      # cache_seqlens is not modified
    # the expected bytes, computed on the CPU
    cast = lambda x, d: (x.cpu().float() / d.cpu()[:, :, None, None]).clamp(-448, 448).to(F8)
    kq, vq = cast(kn, kd), cast(vn, vd)
    for x8 in (kq, vq):
        c = u8(x8) & 0x7F
        assert (c == 0x7E).any() and ((c >= 1) & (c <= 7)).any() and (u8(x8) == 0x80).any() and (c != 0x7F).all()
    kx, vx = k0.clone(), v0.clone()
    for b, L in enumerate(lens):
        u8(kx)[b, :, L:L + Snew] = u8(kq)[b].cuda()
        u8(vx)[b, :, L:L + Snew] = u8(vq)[b].cuda()
    assert torch.equal(u8(k8), u8(kx)), int((u8(k8) != u8(kx)).sum())
    assert torch.equal(u8(v8), u8(vx)), int((u8(v8) != u8(vx)).sum())
    # and the helper builds the same bytes on the device
    assert torch.equal(u8(M.quantize_kv_fp8(kn, kd)[0]).cpu(), u8(kq))
    full = [L + Snew for L in lens]
    o2, lse2 = M.flash_attention_kvcache_fp8(q, kx, vx, torch.tensor(full, dtype=torch.int32, device="cuda"), kd, vd,
                                             is_causal=True, return_lse=True)
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16)) and torch.equal(lse, lse2)
    check(q, kx, vx, kd, vd, full, True, (-1, -1), o, lse)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_transposed_cache_is_read_in_place_bit_for_bit(dtype):
    M = _M()
    B, H, Hkv, Sq, Sc, D = 3, 16, 4, 2, 777, 128
    lens = [777, 5, 400]
    q, k8, v8, kd, vd = make8(B, H, Hkv, Sq, Sc, D, dtype, lens, seed=9)
    kt = k8.transpose(1, 2).contiguous().transpose(1, 2)        # [B, S_cache, H_kv, D] storage seen as [B, H_kv, S_cache, D]
    vt = v8.transpose(1, 2).contiguous().transpose(1, 2)
    assert not kt.is_contiguous() and kt.stride(2) == Hkv * D
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for is_causal, window in MASKS:
        a = M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd, is_causal=is_causal, window_size=window, return_lse=True)
        b = M.flash_attention_kvcache_fp8(q, kt, vt, sl, kd, vd, is_causal=is_causal, window_size=window, return_lse=True)
        assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
        assert torch.equal(a[1], b[1])
    # the append writes the transposed storage in place
    kn = torch.randn(B, Hkv, 3, D, device="cuda").to(dtype)
    vn = torch.randn(B, Hkv, 3, D, device="cuda").to(dtype)
    sl2 = torch.tensor([700, 5, 400], dtype=torch.int32, device="cuda")
    a = M.flash_attention_kvcache_fp8(q, k8, v8, sl2, kd, vd, k_new=kn, v_new=vn, return_lse=True)
    b = M.flash_attention_kvcache_fp8(q, kt, vt, sl2, kd, vd, k_new=kn, v_new=vn, return_lse=True)
    assert torch.equal(u8(k8), u8(kt.contiguous())) and torch.equal(u8(v8), u8(vt.contiguous()))
    assert not torch.equal(u8(k8)[0, :, 700:703], torch.zeros_like(u8(k8)[0, :, 700:703]))
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n", [1, 2, 7, 0])
def test_forced_split_counts_are_accurate_and_repeatable(n, dtype):
    M = _M()
    vck.splits(n)
    B, H, Hkv, Sq, Sc, D = 4, 32, 8, 3, 4100, 128
    lens = [4100, 1, 2222, 777]
    for is_causal, window in MASKS:
        q, k8, v8, kd, vd, sl, o, lse, _, _ = run_case(B, H, Hkv, Sq, Sc, D, dtype, lens, is_causal, window, seed=11)
        for _ in range(3):
            o2, lse2 = M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd, is_causal=is_causal, window_size=window,
                                                     return_lse=True)
            assert torch.equal(o.view(torch.int16), o2.view(torch.int16)) and torch.equal(lse, lse2)


def test_large_point():
    """B8 H32 H_kv 8 S_q 1 L16384 D128 bf16, the benchmark's headline point"""
    B, H, Hkv, L, D = 8, 32, 8, 16384, 128
    run_case(B, H, Hkv, 1, L, D, BF16, [L] * B, False, (-1, -1), seed=17)


def test_graph_captured_step_replays_after_seqlens_advance():
    M = _M()
    B, H, Hkv, Sq, Sc, D, Snew = 4, 32, 8, 1, 4096, 128, 1
    lens = [100, 2000, 3000, 4000]
    q, k8, v8, kd, vd = make8(B, H, Hkv, Sq, Sc, D, BF16, lens, seed=19)
    g = torch.Generator(device="cuda").manual_seed(20)
    kn = torch.randn(B, Hkv, Snew, D, generator=g, device="cuda").to(BF16)
    vn = torch.randn(B, Hkv, Snew, D, generator=g, device="cuda").to(BF16)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")

    def eager():
        kx, vx = k8.clone(), v8.clone()
        o = M.flash_attention_kvcache_fp8(q, kx, vx, sl.clone(), kd, vd, k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        return o, kx, vx

    eager()                                                       # warm-up (LDS opt-in, allocator)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd, k_new=kn, v_new=vn, is_causal=True)
    for step in range(3):
        o_e, k_e, v_e = eager()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), o_e.view(torch.int16)), step
        assert torch.equal(u8(k8), u8(k_e)) and torch.equal(u8(v8), u8(v_e))
        sl += Snew                                                # advance in place; new token's q / k / v
        q.copy_(torch.randn(q.shape, generator=g, device="cuda").to(BF16))
        kn.copy_(torch.randn(kn.shape, generator=g, device="cuda").to(BF16))
        vn.copy_(torch.randn(vn.shape, generator=g, device="cuda").to(BF16))


def raw_kvcache_fp8(q, k8, v8, kd, vd, sl, splits, window=(-1, -1), o=None, q_strides=None, o_strides=None):
    """fa_fwd_kvcache_fp8 through ctypes with `splits` forced: o (NaN-filled unless given), lse and the workspace
    NaN-filled before the launch.  Returns o, lse and the workspace."""
    import _mi355fa as fa
    vck.splits(splits)
    B, H, Sq, D = q.shape
    Hkv, Sc = k8.shape[1], k8.shape[2]
    need = fa.lib.fa_fwd_kvcache_fp8_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D)
    assert need == (0 if splits == 1 else splits * B * H * Sq * (D + 2) * 4), need
    ws = torch.full((max(need, 16) // 4,), float("nan"), device="cuda")
    if o is None:
        o = torch.full_like(q, float("nan"))
    lse = torch.full((B, H, Sq), float("nan"), device="cuda")
    S3 = lambda s: None if s is None else ctypes.cast((ctypes.c_longlong * 3)(*s), ctypes.POINTER(ctypes.c_longlong))
    keep = [S3(q_strides), S3(o_strides)]
    opts = fa.Opts.make(q_strides=keep[0], o_strides=keep[1])
    P = lambda t: t.data_ptr()
    fa.check(fa.lib.fa_fwd_kvcache_fp8(P(q), P(k8), P(v8), None, None, P(sl), P(kd), P(vd), Hkv if kd.dim() == 2 else 0,
                                       P(o), P(lse), P(ws), need, B, H, Hkv, Sq, Sc, 0, D, int(q.dtype == BF16),
                                       fa.KV_FP8_E4M3, D ** -0.5, window[0], window[1], ctypes.byref(opts),
                                       torch.cuda.current_stream().cuda_stream), "fa_fwd_kvcache_fp8")
    torch.cuda.synchronize()
    return o, lse, ws


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_raw_entry_point_writes_every_element_at_forced_splits(dtype):
    B, H, Hkv, Sq, Sc, D = 5, 8, 2, 4, 1400, 128
    lens = [0, 1, 3, 700, 1400]
    for per_batch in (True, False):
        q, k8, v8, kd, vd = make8(B, H, Hkv, Sq, Sc, D, dtype, lens, seed=21, per_batch=per_batch)
        sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        for is_causal, window in MASKS:
            wl, wr = window_of(is_causal, window)
            for n in (1, 2, 7):
                o, lse, _ = raw_kvcache_fp8(q, k8, v8, kd, vd, sl, n, (wl, wr))
                assert not torch.isnan(o).any() and not torch.isnan(lse).any(), (n, is_causal, window)
                _, LSE_ref = check(q, k8, v8, kd, vd, lens, is_causal, window, o, lse)
                assert (o[torch.isinf(LSE_ref)] == 0).all()


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_bshd_query_and_output_views_are_read_and_written_in_place(dtype):
    B, H, Hkv, Sq, Sc, D = 3, 16, 4, 5, 900, 64
    lens = [900, 2, 517]
    q, k8, v8, kd, vd = make8(B, H, Hkv, Sq, Sc, D, dtype, lens, seed=23)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    q_bshd = q.transpose(1, 2).contiguous()
    st = (Sq * H * D, D, H * D)                               # {batch, head, seq} element strides of the view
    for n in (1, 3):
        o_c, lse_c, _ = raw_kvcache_fp8(q, k8, v8, kd, vd, sl, n, (-1, 0))
        o_bshd = torch.full((B, Sq, H, D), float("nan"), dtype=dtype, device="cuda")
        _, lse_v, _ = raw_kvcache_fp8(q_bshd.transpose(1, 2), k8, v8, kd, vd, sl, n, (-1, 0), o=o_bshd.transpose(1, 2),
                                      q_strides=st, o_strides=st)
        assert not torch.isnan(o_bshd).any()
        assert torch.equal(o_bshd.transpose(1, 2).contiguous().view(torch.int16), o_c.view(torch.int16)), n
        assert torch.equal(lse_v, lse_c), n


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_per_head_against_fp64_at_long_ragged_fill_levels(dtype):
    """B16 H32 H_kv 8 S_q 4 with fill levels from 0 to 32768: every (batch, head) of O against fp64 on its own (a
    whole-tensor norm would hide one wrong head), and LSE row by row; full and causal.  Bounds per (batch, head) are those
    of test_gpu_kvcache.test_per_head_against_fp64_at_long_ragged_fill_levels (1e-3 fp16, 8e-3 bf16)."""
    import fa_oracle as fo
    M = _M()
    B, H, Hkv, Sq, Sc, D = 16, 32, 8, 4, 32768, 128
    lens = [32768, 0, 1, 3, 4, 5, 127, 128, 129, 1000, 4097, 8191, 16384, 20000, 32767, 31000]
    q, k8, v8, kd, vd = make8(B, H, Hkv, Sq, Sc, D, dtype, lens, seed=25)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    bound = 1e-3 if dtype == F16 else 8e-3
    for is_causal in (False, True):
        o, lse = M.flash_attention_kvcache_fp8(q, k8, v8, sl, kd, vd, is_causal=is_causal, return_lse=True)
        torch.cuda.synchronize()
        O = torch.zeros(B, H, Sq, D, dtype=torch.float64, device="cuda")
        LSE = torch.empty(B, H, Sq, dtype=torch.float64, device="cuda")
        for b in range(B):                                                     # one sequence at a time: fp64 K/V are large
            O[b:b + 1], LSE[b:b + 1] = ref_fp64(q[b:b + 1], deq(k8[b:b + 1], kd[b:b + 1]), deq(v8[b:b + 1], vd[b:b + 1]),
                                                lens[b:b + 1], -1, 0 if is_causal else -1)
        err = fo.block_errors(O, o, block=Sq)[..., 0]                          # [B, H]
        at = tuple(int(x) for x in torch.unravel_index(err.argmax(), err.shape))
        print("worst (b, h)", at, err[at].item())
        assert (err < bound).all(), ("(b, h)", at, err[at].item(), lens[at[0]], is_causal)
        assert (o[1] == 0).all()                                                # L = 0
        check_lse(lse, LSE)
