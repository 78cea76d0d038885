"""What v_cvt_scalef32_pk_{f16,bf16}_fp8 does with a scale operand other than 1.0, element for element through the kernels
(include/mi355fa_kvcache_fp8_token.h, "Exactness"), in the style of tests/test_gpu_fp4_scales.py: one key per sequence and
one-hot queries (head h asks for element h), so that O is the V row as the kernel forms it and LSE is one score.  All 256 e4m3
codes -- the two NaN bytes are left out, the header leaves them unspecified -- against the V scales 2^k, k = -40 .. 24, and
scales that are no powers of two.

The kernel hands a row's fp32 V scale s = 2^e * m (1 <= m < 2) to the conversion AS IT IS and multiplies the key's probability
(here exactly 1) by m before rounding it to T.  So every element must come back as round_T(round_T(m) * (byte * 2^e)): that holds
only if the instruction reads the exponent field of its scale operand alone -- 2^e, the scale rounded DOWN to a power of two,
not one rounding of byte * scale -- and delivers byte * 2^e without rounding wherever T represents it, T's subnormals included.
Measured on an MI355X: it does, for every code, in both dtypes (a stand-alone probe of the instruction, one byte pair and one
scale operand per thread, gave the same over these scales before the kernel was written; the probe is not part of the library).
Elements whose byte * 2^e T does not represent (fp16: below 2^-24 or above 65504) are not compared: the header leaves them to
the instruction."""
import pytest
import torch

import fp8tokencheck as tk
import variantcheck as vck
from fp8tokencheck import DT, F8, IDS

pytestmark = pytest.mark.gpu

CODES = [c for c in range(256) if c & 0x7F != 0x7F]
POW2 = [2.0 ** k for k in range(-40, 25)]
ODD = [1.5, 1.25, 1.9999999, 1.0000001, 0.142857, 3.3e-5, 448.0 / 3.0, 1.75 * 2.0 ** -15, 1.1 * 2.0 ** -20, 1.999 * 2.0 ** 6]
SCALE = 2.0 ** -3


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_every_code_under_powers_of_two_and_other_scales(D, dtype):
    scales = POW2 + ODD
    codes = torch.tensor(CODES, dtype=torch.uint8)
    B = len(scales)
    v8 = torch.full((B, 1, 32, D), 0xFF, dtype=torch.uint8)
    v8[:, 0, 0] = torch.stack([codes.roll(-(D * b) % len(CODES))[:D] for b in range(B)])
    k8 = torch.full((B, 1, 32, D), 0xFF, dtype=torch.uint8)
    k8[:, 0, 0] = 0x38                                                          # 1.0
    vs = torch.full((B, 1, 32), float("nan"))
    vs[:, 0, 0] = torch.tensor(scales)
    ks = torch.full((B, 1, 32), float("nan"))
    ks[:, 0, 0] = torch.tensor(scales).flip(0).clamp(2.0 ** -20, 2.0 ** 10)     # scores that stay moderate
    q = torch.eye(D, dtype=dtype).view(1, D, 1, D).expand(B, D, 1, D).contiguous().cuda()
    sl = torch.ones(B, dtype=torch.int32, device="cuda")
    s64 = vs[:, 0, 0].double()
    e = torch.floor(torch.log2(s64))
    m = (s64 / torch.exp2(e)).to(dtype).double()                                 # round_T of the mantissa
    assert ((s64 / torch.exp2(e)) >= 1).all() and ((s64 / torch.exp2(e)) < 2).all()
    pow2 = v8[:, 0, 0].view(F8).double() * torch.exp2(e)[:, None]                # byte * 2^e
    held = pow2.to(dtype).double() == pow2                                       # T represents it (its subnormals included)
    want = (m[:, None] * pow2).to(dtype)
    held &= torch.isfinite(want.double())
    assert held.float().mean() > 0.5 and held[len(POW2):].float().mean() > 0.8
    assert (pow2[held].abs() < torch.finfo(dtype).tiny).any() and (pow2[held] != 0).any()   # subnormal in T
    seen = {int(c) for c in v8[:, 0, 0][held].tolist()}
    assert seen == set(CODES)
    for n in (1, 2):
        vck.splits(n)
        try:
            o, lse = tk.padded(q, k8.view(F8).cuda(), v8.view(F8).cuda(), ks.cuda(), vs.cuda(), sl, softmax_scale=SCALE)
        finally:
            vck.splits(0)
        torch.cuda.synchronize()
        got = torch.stack([o.cpu()[b, torch.arange(D), 0, torch.arange(D)] for b in range(B)])   # head h holds element h
        bad = held & (got.double() != want.double())
        assert not bad.any(), (n, [(scales[int(i)], hex(int(v8[i, 0, 0, j])), float(got[i, j]), float(want[i, j]))
                                   for i, j in bad.nonzero()[:20]])
        # one rounding of byte * scale would differ somewhere
        once = (v8[:, 0, 0].view(F8).double() * vs[:, 0, 0].double()[:, None]).to(dtype)
        assert (held & (once.double() != want.double())).any()
        # the score of head h is q_h . K = 1.0 * k_scale, times softmax_scale: the LSE of a single key
        want_lse = (ks[:, 0, 0].double() * SCALE).view(B, 1, 1).expand(B, D, 1)
        assert torch.allclose(lse.cpu().double(), want_lse, rtol=1e-6, atol=1e-30)
