"""GPU tests of decoding attention over a padded KV cache (include/mi355fa_kvcache.h, flash_attention_kvcache): O and LSE
against the fp64 attention of tests/attn_ref.py under the bottom-right aligned mask, on K/V sliced to each L_b;
ragged fill levels (0 included), rows with no visible key, NaN padding past L_b, the append, transposed caches read in
place, forced split counts and their determinism, agreement with flash_attention_gqa, one large point against device SDPA,
and a graph-captured decode step replayed after cache_seqlens advances.

Tolerances as in test_gpu_gqa.py: fp16 relFro < 1e-3 against fp64; bf16 < max(2x PyTorch's own bf16 SDPA, 4e-3)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from attn_ref import attention_fp64, visible
import variantcheck as vck

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
GROUPS = [(4, 4), (8, 2), (8, 1), (32, 8)]
MASKS = [(False, (-1, -1)), (True, (-1, -1)), (False, (40, 8))]   # full, causal, window


def _M():
    import My_FlashAttention_optimized as M
    return M


@pytest.fixture(autouse=True)
def _formula_splits():
    yield
    vck.splits(0)


def window_of(is_causal, window):
    wl, wr = window
    return (wl, 0) if is_causal else (wl, wr)


def ref_fp64(q, kc, vc, lens, wl, wr, scale=None):
    """O [B, H, S_q, D] (fp64) and LSE [B, H, S_q]: per sequence, on K/V sliced to L_b (the caches may carry NaN past it)."""
    B, H, Sq, D = q.shape
    scale = D ** -0.5 if scale is None else scale
    O = torch.zeros(B, H, Sq, D, dtype=torch.float64, device=q.device)
    LSE = torch.full((B, H, Sq), float("-inf"), dtype=torch.float64, device=q.device)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        r = attention_fp64(q[b:b + 1], kc[b:b + 1, :, :L], vc[b:b + 1, :, :L], None, scale, visible(Sq, L, wl, wr, q.device, L=L))
        O[b], LSE[b] = r["O"][0], r["LSE"][0]
    return O, LSE


def sdpa_level(q, kc, vc, lens, wl, wr, O_ref, scale=None):
    """relFro of PyTorch's own bf16 SDPA on the same problem, at the same softmax scale (None: 1/sqrt(D)); rows with no
    visible key set to 0."""
    B, H, Sq, D = q.shape
    g = H // kc.shape[1]
    out = torch.zeros(B, H, Sq, D, dtype=torch.float64, device=q.device)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        K = kc[b, :, :L].repeat_interleave(g, 0)[None]
        V = vc[b, :, :L].repeat_interleave(g, 0)[None]
        o = F.scaled_dot_product_attention(q[b][None], K, V, attn_mask=visible(Sq, L, wl, wr, q.device, L=L), scale=scale)
        out[b] = o[0].double().nan_to_num(0.0)
    return rel(out, O_ref)


def rel(a, b):
    n = b.double().norm()
    return float((a.double() - b.double()).norm() / (n if n > 0 else 1.0))


def tol(dtype, q, kc, vc, lens, wl, wr, O_ref, scale=None):
    return 1e-3 if dtype == F16 else max(2 * sdpa_level(q, kc, vc, lens, wl, wr, O_ref, scale), 4e-3)


def check_lse(lse, LSE_ref):
    inf = torch.isinf(LSE_ref)
    assert torch.equal(torch.isneginf(lse), inf), "LSE = -inf exactly on the rows with no visible key"
    assert torch.allclose(lse[~inf].double(), LSE_ref[~inf], rtol=1e-3, atol=2e-3), \
        float((lse[~inf].double() - LSE_ref[~inf]).abs().max())


def make(B, H, Hkv, Sq, Sc, D, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(dtype)
    return r(B, H, Sq, D), r(B, Hkv, Sc, D), r(B, Hkv, Sc, D)


def run_case(B, H, Hkv, Sq, Sc, D, dtype, lens, is_causal, window, seed=0, **kw):
    M = _M()
    q, kc, vc = make(B, H, Hkv, Sq, Sc, D, dtype, seed)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    o, lse = M.flash_attention_kvcache(q, kc, vc, sl, is_causal=is_causal, window_size=window, return_lse=True, **kw)
    torch.cuda.synchronize()
    wl, wr = window_of(is_causal, window)
    O_ref, LSE_ref = ref_fp64(q, kc, vc, lens, wl, wr, kw.get("softmax_scale"))
    assert o.shape == q.shape and o.dtype == dtype and lse.shape == (B, H, Sq) and lse.dtype == torch.float32
    assert torch.isfinite(o).all()
    err = rel(o, O_ref)
    t = tol(dtype, q, kc, vc, lens, wl, wr, O_ref)
    assert err < t, (err, t)
    check_lse(lse, LSE_ref)
    return q, kc, vc, sl, o, lse, O_ref, LSE_ref


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq", [1, 3, 16, 130])
@pytest.mark.parametrize("H,Hkv", GROUPS)
def test_matches_fp64(H, Hkv, Sq, D, dtype):
    Sc = 320 if Sq < 130 else 450
    lens = [Sc - 17, 200, 131] if Sq < 130 else [Sc, 300, 200]
    for is_causal, window in MASKS:
        run_case(3, H, Hkv, Sq, Sc, D, dtype, lens, is_causal, window, seed=Sq + D)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_ragged_lengths_and_rows_without_keys(D, dtype):
    lens = [0, 1, 63, 64, 65, 127, 129, 3000]
    for Sq in (1, 5):                                     # S_q = 5 > L_b for L_b in {0, 1}: rows with no visible key
        for is_causal, window in MASKS:
            q, kc, vc, sl, o, lse, O_ref, LSE_ref = run_case(8, 8, 2, Sq, 3072, D, dtype, lens, is_causal, window)
            empty = torch.isinf(LSE_ref)
            assert empty[0].all()                         # L = 0: every row
            if Sq == 5 and is_causal:
                assert empty[1, :, :4].all()              # L = 1: queries 0..3 sit at negative positions
            assert (o[empty] == 0).all()


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_nan_padding_past_the_fill_level_is_never_read(dtype):
    M = _M()
    B, H, Hkv, Sq, Sc, D = 4, 8, 2, 3, 600, 128
    lens = [0, 70, 333, 600]
    q, kc, vc = make(B, H, Hkv, Sq, Sc, D, dtype, seed=5)
    for b, L in enumerate(lens):
        kc[b, :, L:] = float("nan")
        vc[b, :, L:] = float("nan")
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for n in (0, 1, 3):
        vck.splits(n)
        for is_causal, window in MASKS:
            o, lse = M.flash_attention_kvcache(q, kc, vc, sl, is_causal=is_causal, window_size=window, return_lse=True)
            wl, wr = window_of(is_causal, window)
            O_ref, LSE_ref = ref_fp64(q, kc, vc, lens, wl, wr)
            assert torch.isfinite(o).all() and not torch.isnan(lse).any()
            assert rel(o, O_ref) < tol(dtype, q, kc, vc, lens, wl, wr, O_ref)
            check_lse(lse, LSE_ref)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_append_writes_exactly_the_new_rows(D, dtype):
    M = _M()
    B, H, Hkv, Sq, Sc = 4, 8, 2, 4, 520
    lens = [0, 100, 257, 516]                                   # the last one fills the cache to the end
    Snew = 4
    q, kc, vc = make(B, H, Hkv, Sq, Sc, D, dtype, seed=7)
    g = torch.Generator(device="cuda").manual_seed(8)
    kn = torch.randn(B, Hkv, Snew, D, generator=g, device="cuda").to(dtype)
    vn = torch.randn(B, Hkv, Snew, D, generator=g, device="cuda").to(dtype)
    k0, v0 = kc.clone(), vc.clone()
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    o, lse = M.flash_attention_kvcache(q, kc, vc, sl, k_new=kn, v_new=vn, is_causal=True, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(sl.cpu(), torch.tensor(lens, dtype=torch.int32))      # cache_seqlens is not modified
    kx, vx = k0.clone(), v0.clone()
    for b, L in enumerate(lens):
        kx[b, :, L:L + Snew] = kn[b]
        vx[b, :, L:L + Snew] = vn[b]
    assert torch.equal(kc.view(torch.int16), kx.view(torch.int16))
    assert torch.equal(vc.view(torch.int16), vx.view(torch.int16))
    full = [L + Snew for L in lens]
    O_ref, LSE_ref = ref_fp64(q, kx, vx, full, -1, 0)
    assert rel(o, O_ref) < tol(dtype, q, kx, vx, full, -1, 0, O_ref)
    check_lse(lse, LSE_ref)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_transposed_cache_is_read_in_place_bit_for_bit(dtype):
    M = _M()
    B, H, Hkv, Sq, Sc, D = 3, 16, 4, 2, 777, 128
    q, kc, vc = make(B, H, Hkv, Sq, Sc, D, dtype, seed=9)
    kt = kc.transpose(1, 2).contiguous().transpose(1, 2)        # [B, S_cache, H_kv, D] storage seen as [B, H_kv, S_cache, D]
    vt = vc.transpose(1, 2).contiguous().transpose(1, 2)
    assert not kt.is_contiguous() and kt.stride(2) == Hkv * D
    sl = torch.tensor([777, 5, 400], dtype=torch.int32, device="cuda")
    for is_causal, window in MASKS:
        a = M.flash_attention_kvcache(q, kc, vc, sl, is_causal=is_causal, window_size=window, return_lse=True)
        b = M.flash_attention_kvcache(q, kt, vt, sl, is_causal=is_causal, window_size=window, return_lse=True)
        assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
        assert torch.equal(a[1], b[1])
    # the append writes the transposed storage in place
    kn = torch.randn(B, Hkv, 3, D, device="cuda").to(dtype)
    vn = torch.randn(B, Hkv, 3, D, device="cuda").to(dtype)
    sl2 = torch.tensor([700, 5, 400], dtype=torch.int32, device="cuda")
    a = M.flash_attention_kvcache(q, kc, vc, sl2, k_new=kn, v_new=vn, return_lse=True)
    b = M.flash_attention_kvcache(q, kt, vt, sl2, k_new=kn, v_new=vn, return_lse=True)
    assert torch.equal(kc.view(torch.int16), kt.contiguous().view(torch.int16))
    assert torch.equal(vc.view(torch.int16), vt.contiguous().view(torch.int16))
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n", [1, 2, 7, 0])
def test_forced_split_counts_are_accurate_and_repeatable(n, dtype):
    M = _M()
    vck.splits(n)
    B, H, Hkv, Sq, Sc, D = 4, 32, 8, 3, 4100, 128
    lens = [4100, 1, 2222, 777]
    for is_causal, window in MASKS:
        q, kc, vc, sl, o, lse, _, _ = run_case(B, H, Hkv, Sq, Sc, D, dtype, lens, is_causal, window, seed=11)
        for _ in range(3):
            o2, lse2 = M.flash_attention_kvcache(q, kc, vc, sl, is_causal=is_causal, window_size=window, return_lse=True)
            assert torch.equal(o.view(torch.int16), o2.view(torch.int16)) and torch.equal(lse, lse2)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_single_query_matches_flash_attention_gqa(D, dtype):
    M = _M()
    B, H, Hkv, Sc, L = 2, 32, 8, 5000, 4321
    q, kc, vc = make(B, H, Hkv, 1, Sc, D, dtype, seed=13)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    o = M.flash_attention_kvcache(q, kc, vc, sl)
    ref = M.flash_attention_gqa(q, kc[:, :, :L], vc[:, :, :L])
    O_ref, _ = ref_fp64(q, kc, vc, [L] * B, -1, -1)
    t = tol(dtype, q, kc, vc, [L] * B, -1, -1, O_ref)
    assert rel(o, ref) < t and rel(o, O_ref) < t


def test_large_point_against_sdpa():
    M = _M()
    B, H, Hkv, L, D = 8, 32, 8, 32768, 128
    q, kc, vc = make(B, H, Hkv, 1, L, D, BF16, seed=17)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    o, lse = M.flash_attention_kvcache(q, kc, vc, sl, return_lse=True)
    O_ref, LSE_ref = ref_fp64(q, kc, vc, [L] * B, -1, -1)
    sd = F.scaled_dot_product_attention(q, kc.repeat_interleave(H // Hkv, 1), vc.repeat_interleave(H // Hkv, 1))
    level = rel(sd, O_ref)
    assert rel(o, O_ref) < max(2 * level, 4e-3), (rel(o, O_ref), level)
    check_lse(lse, LSE_ref)


def test_graph_captured_step_replays_after_seqlens_advance():
    M = _M()
    B, H, Hkv, Sq, Sc, D, Snew = 4, 32, 8, 1, 4096, 128, 1
    q, kc, vc = make(B, H, Hkv, Sq, Sc, D, BF16, seed=19)
    g = torch.Generator(device="cuda").manual_seed(20)
    kn = torch.randn(B, Hkv, Snew, D, generator=g, device="cuda").to(BF16)
    vn = torch.randn(B, Hkv, Snew, D, generator=g, device="cuda").to(BF16)
    sl = torch.tensor([100, 2000, 3000, 4000], dtype=torch.int32, device="cuda")

    def eager():
        kx, vx = kc.clone(), vc.clone()
        o = M.flash_attention_kvcache(q, kx, vx, sl.clone(), k_new=kn, v_new=vn, is_causal=True)
        torch.cuda.synchronize()
        return o, kx, vx

    eager()                                                       # warm-up (LDS opt-in, allocator)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = M.flash_attention_kvcache(q, kc, vc, sl, k_new=kn, v_new=vn, is_causal=True)
    for step in range(3):
        o_e, k_e, v_e = eager()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), o_e.view(torch.int16)), step
        assert torch.equal(kc.view(torch.int16), k_e.view(torch.int16)) and torch.equal(vc.view(torch.int16), v_e.view(torch.int16))
        sl += Snew                                                # advance in place; new token's q / k / v
        q.copy_(torch.randn(q.shape, generator=g, device="cuda").to(BF16))
        kn.copy_(torch.randn(kn.shape, generator=g, device="cuda").to(BF16))
        vn.copy_(torch.randn(vn.shape, generator=g, device="cuda").to(BF16))


def raw_kvcache(q, kc, vc, sl, splits, window=(-1, -1), o=None, q_strides=None, o_strides=None):
    """fa_fwd_kvcache through ctypes with `splits` forced: o (NaN-filled unless given), lse and the workspace NaN-filled
    before the launch.  Returns o, lse and the workspace."""
    import _mi355fa as fa
    vck.splits(splits)
    B, H, Sq, D = q.shape
    Hkv, Sc = kc.shape[1], kc.shape[2]
    need = fa.lib.fa_fwd_kvcache_workspace_bytes(B, H, Hkv, Sq, Sc, 0, D)
    assert need == (0 if splits == 1 else splits * B * H * Sq * (D + 2) * 4), need
    ws = torch.full((max(need, 16) // 4,), float("nan"), device="cuda")
    if o is None:
        o = torch.full_like(q, float("nan"))
    lse = torch.full((B, H, Sq), float("nan"), device="cuda")
    S3 = lambda s: None if s is None else ctypes.cast((ctypes.c_longlong * 3)(*s), ctypes.POINTER(ctypes.c_longlong))
    keep = [S3(q_strides), S3(o_strides)]
    opts = fa.Opts.make(q_strides=keep[0], o_strides=keep[1])
    P = lambda t: t.data_ptr()
    fa.check(fa.lib.fa_fwd_kvcache(P(q), P(kc), P(vc), None, None, P(sl), P(o), P(lse), P(ws), need, B, H, Hkv, Sq, Sc, 0,
                                   D, int(q.dtype == BF16), D ** -0.5, window[0], window[1], ctypes.byref(opts),
                                   torch.cuda.current_stream().cuda_stream), "fa_fwd_kvcache")
    torch.cuda.synchronize()
    return o, lse, ws


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_raw_entry_point_writes_every_element_at_forced_splits(dtype):
    """fa_fwd_kvcache with o, lse and the workspace filled with NaN first, at 1, 2 and 7 forced splits: no element of o
    or lse stays NaN -- rows with no visible key (L = 0, and S_q > L under the causal mask) and splits whose key range
    lies past L_b included -- rows without a key come out exactly 0, and the results hold the fp64 tolerance."""
    B, H, Hkv, Sq, Sc, D = 5, 8, 2, 4, 1400, 128
    lens = [0, 1, 3, 700, 1400]
    q, kc, vc = make(B, H, Hkv, Sq, Sc, D, dtype, seed=21)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for is_causal, window in MASKS:
        wl, wr = window_of(is_causal, window)
        O_ref, LSE_ref = ref_fp64(q, kc, vc, lens, wl, wr)
        for n in (1, 2, 7):
            o, lse, _ = raw_kvcache(q, kc, vc, sl, n, (wl, wr))
            assert not torch.isnan(o).any() and not torch.isnan(lse).any(), (n, is_causal, window)
            assert (o[torch.isinf(LSE_ref)] == 0).all()
            assert rel(o, O_ref) < tol(dtype, q, kc, vc, lens, wl, wr, O_ref), n
            check_lse(lse, LSE_ref)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_bshd_query_and_output_views_are_read_and_written_in_place(dtype):
    """Q and O as [B, S_q, H, D] buffers seen as [B, H, S_q, D] (FlashAttention-2's layout), through the q and o strides
    of fa_fwd_kvcache: the view is read in place, O lands in the [B, S_q, H, D] buffer (NaN-filled first), and the bits
    equal the contiguous call's at 1 and 3 splits."""
    B, H, Hkv, Sq, Sc, D = 3, 16, 4, 5, 900, 64
    q, kc, vc = make(B, H, Hkv, Sq, Sc, D, dtype, seed=23)
    sl = torch.tensor([900, 2, 517], dtype=torch.int32, device="cuda")
    q_bshd = q.transpose(1, 2).contiguous()
    st = (Sq * H * D, D, H * D)                               # {batch, head, seq} element strides of the view
    for n in (1, 3):
        o_c, lse_c, _ = raw_kvcache(q, kc, vc, sl, n, (-1, 0))
        o_bshd = torch.full((B, Sq, H, D), float("nan"), dtype=dtype, device="cuda")
        _, lse_v, _ = raw_kvcache(q_bshd.transpose(1, 2), kc, vc, sl, n, (-1, 0), o=o_bshd.transpose(1, 2),
                                  q_strides=st, o_strides=st)
        assert not torch.isnan(o_bshd).any()
        assert torch.equal(o_bshd.transpose(1, 2).contiguous().view(torch.int16), o_c.view(torch.int16)), n
        assert torch.equal(lse_v, lse_c), n


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_per_head_against_fp64_at_long_ragged_fill_levels(dtype):
    """B16 H32 H_kv 8 S_q 4 with fill levels from 0 to 32768: every (batch, head) of O against fp64 on its own (a
    whole-tensor norm would hide one wrong head), and LSE row by row; full and causal.  Bounds per (batch, head) are the
    per-block bounds of tests/test_gpu_persistent.py (1e-3 fp16, 8e-3 bf16)."""
    import fa_oracle as fo
    M = _M()
    B, H, Hkv, Sq, Sc, D = 16, 32, 8, 4, 32768, 128
    lens = [32768, 0, 1, 3, 4, 5, 127, 128, 129, 1000, 4097, 8191, 16384, 20000, 32767, 31000]
    q, kc, vc = make(B, H, Hkv, Sq, Sc, D, dtype, seed=25)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    bound = 1e-3 if dtype == F16 else 8e-3
    for is_causal in (False, True):
        o, lse = M.flash_attention_kvcache(q, kc, vc, sl, is_causal=is_causal, return_lse=True)
        torch.cuda.synchronize()
        O_ref, LSE_ref = ref_fp64(q, kc, vc, lens, -1, 0 if is_causal else -1)
        err = fo.block_errors(O_ref, o, block=Sq)[..., 0]                      # [B, H]
        at = tuple(int(x) for x in torch.unravel_index(err.argmax(), err.shape))
        assert (err < bound).all(), ("(b, h)", at, err[at].item(), lens[at[0]], is_causal)
        assert (o[1] == 0).all()                                                # L = 0
        check_lse(lse, LSE_ref)
