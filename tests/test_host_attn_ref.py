"""CPU tests of tests/attn_ref.py, the fp64 reference the GPU tests trust: its masks against fa_oracle.visible_mask and the
decode definition, the plain closed form against fa_oracle.attention_fp64_chunked, and the composed order of the three
score transforms (cap, then bias, then sink) against torch.autograd through the eager implementation.  The per-feature
agreement with autograd is in test_host_softcap.py, test_host_alibi.py, test_host_sink.py and test_host_gqa.py."""
import pytest
import torch

import attn_ref as ar
import fa_oracle as fo

WINDOWS = [(-1, -1), (-1, 0), (3, 0), (2, 2), (0, 5)]


@pytest.mark.parametrize("Sq,Sk", [(17, 10), (9, 13)])
def test_training_masks_equal_the_oracle_masks(Sq, Sk):
    for w in WINDOWS:
        assert torch.equal(ar.visible(Sq, Sk, w[0], w[1], "cpu"), fo.visible_mask(Sq, Sk, w)), w


@pytest.mark.parametrize("L", [0, 2, 14, 20])
def test_decode_masks_are_bottom_right_aligned_over_the_keys_below_L(L):
    Sq, Sk = 3, 20
    for wl, wr in WINDOWS:
        want = torch.zeros(Sq, Sk, dtype=torch.bool)
        for i in range(Sq):
            pos = L - Sq + i
            for j in range(L):
                want[i, j] = (wl < 0 or j >= pos - wl) and (wr < 0 or j <= pos + wr)
        assert torch.equal(ar.visible(Sq, Sk, wl, wr, "cpu", L=L), want), (wl, wr)


@pytest.mark.parametrize("window", [(-1, -1), (-1, 0), (2, 2)], ids=["full", "causal", "w2x2"])
def test_plain_reference_agrees_with_the_chunked_oracle(window):
    B, H, Hkv, Sq, Sk, D = 2, 6, 2, 17, 10, 8
    g = torch.Generator().manual_seed(Sq + Sk)
    Q, dO = (torch.randn(B, H, Sq, D, generator=g, dtype=torch.float64) for _ in range(2))
    K, V = (torch.randn(B, Hkv, Sk, D, generator=g, dtype=torch.float64) for _ in range(2))
    got = ar.attention_fp64(Q, K, V, dO, D ** -0.5, ar.visible(Sq, Sk, window[0], window[1], "cpu"))
    want = fo.attention_fp64_chunked(Q, K, V, dO, window=window)
    keyless = torch.isneginf(want["LSE"])
    assert torch.equal(torch.isneginf(got["LSE"]), keyless)
    assert bool(keyless.any()) == (window == (2, 2)) and (window != (2, 2) or keyless[:, :, 13:].all())
    fin = ~keyless
    assert torch.allclose(got["LSE"][fin], want["LSE"][fin], rtol=1e-10, atol=1e-10)
    for n in ("O", "dQ", "dK", "dV"):
        assert torch.allclose(got[n], want[n], rtol=1e-10, atol=1e-10), (n, (got[n] - want[n]).abs().max().item())


def test_composed_transforms_agree_with_autograd():
    """Cap, bias and sinks in one call (no kernel composes them; the signature permits it): cap, then bias, then sink."""
    B, H, Hkv, Sq, Sk, D, cap, scale, L, (wl, wr) = 2, 7, 1, 5, 20, 8, 7.0, 0.5, 14, (6, 2)
    g = torch.Generator().manual_seed(L)
    Q = torch.randn(B, H, Sq, D, generator=g, dtype=torch.float64) * (0.7 * cap / (scale * D ** 0.5))
    K, V = (torch.randn(B, Hkv, Sk, D, generator=g, dtype=torch.float64) for _ in range(2))
    dO = torch.randn(B, H, Sq, D, generator=g, dtype=torch.float64)
    slopes = torch.linspace(0.1, 1.0, B * H, dtype=torch.float64).view(B, H)
    sinks = torch.linspace(0.5, 4.0, H, dtype=torch.float64)
    vis, dist = ar.visible(Sq, Sk, wl, wr, "cpu", L=L), ar.distance(Sq, Sk, "cpu", L=L)
    kw = dict(cap=cap, slopes=slopes, dist=dist)
    gt = ar.attention_fp64(Q, K, V, dO, scale, vis, sinks=sinks, **kw)
    q, k, v, z = (x.clone().requires_grad_(True) for x in (Q, K, V, sinks))
    o = ar.attention_eager(q, k, v, scale, vis, sinks=z, **kw)
    o.backward(dO)
    for n, t in (("O", o.detach()), ("dQ", q.grad), ("dK", k.grad), ("dV", v.grad), ("dz", z.grad)):
        assert torch.allclose(gt[n], t, rtol=1e-10, atol=1e-10), (n, (gt[n] - t).abs().max().item())
    # LSE written out in that order (the bias outside the tanh, the sink one more column); every transform matters here
    s = scale * (Q @ K.repeat_interleave(H, 1).transpose(-1, -2))
    lse = torch.logsumexp(torch.cat([(cap * torch.tanh(s / cap) + ar.bias(slopes, dist, B, H)).masked_fill(~vis, -torch.inf),
                                     sinks.view(1, H, 1, 1).expand(B, H, Sq, 1)], -1), -1)
    assert torch.allclose(lse, gt["LSE"], rtol=0, atol=1e-12)
    for one in (dict(cap=cap), dict(slopes=slopes, dist=dist), dict(sinks=sinks)):
        other = ar.attention_fp64(Q, K, V, None, scale, vis, **one)["O"]
        assert (other - gt["O"]).norm() / gt["O"].norm() > 0.02, list(one)
