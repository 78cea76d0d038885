"""CPU tests of tests/variantcheck.py, the check the soft-cap, ALiBi and sink GPU tests share: it must not go soft.  The
fp64 truth rounded to the dtype (LSE to fp32) -- the best a kernel can store -- passes check_training under each file's
real bounds, and a wrong block, a non-zero keyless row, a moved or wrongly finite LSE row and an output that ignores the
transform are each refused.  The shape (B 1, H 6, H_kv 2, S_q 101, S_k 75, D 64, window (20, 10)) has 6 keyless and 7
few-key rows; the rounded truth's largest block error is 2.2e-4 in fp16 and 1.7e-3 in bf16, under the tightest bounds of
the three files, and the transforms move O by 0.59 (cap 5), 0.49 (slopes 2^-(h+1)) and 1.31 (sinks 0 .. 8) relFro.  The
scaled dQ block is refused by relFro in fp16 (3e-3 to 5e-3 against 1e-3) and by the block check in bf16 (8.3e-3 to
8.9e-3, five times the median block); the other three by the zero-row and LSE-row checks of blockcheck.check_outputs.  A
second test runs the shared host-side calls against the built library."""
import pytest
import torch

import attn_ref as ar
import blockcheck as bc
import test_gpu_alibi as ta
import test_gpu_sink as ts
import test_gpu_softcap as tc
import variantcheck as vck

F16, BF16 = torch.float16, torch.bfloat16
B, H, HKV, SQ, SK, D, WINDOW = 1, 6, 2, 101, 75, 64, (20, 10)
SCALE = D ** -0.5
# the file whose bounds apply, attention_fp64's keywords, the "matters" threshold, the Q amplitude
FEATURES = {
    "softcap": (tc, dict(cap=5.0), tc.CAP_MATTERS, tc._amp(5.0, SCALE, D)),
    "alibi": (ta, dict(slopes=2.0 ** -(torch.arange(H, dtype=torch.float64) + 1), dist=ar.distance(SQ, SK, "cpu")),
              ta.BIAS_MATTERS, 1.0),
    "sink": (ts, dict(sinks=torch.linspace(0, 8, H)), ts.BIAS_MATTERS, 1.0),
}


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("feature", list(FEATURES))
def test_check_training_passes_the_rounded_truth_and_refuses_each_mutation(feature, dtype):
    mod, kw, matters, amp = FEATURES[feature]
    g = torch.Generator().manual_seed(SQ + SK + D)
    Q = (torch.randn(B, H, SQ, D, generator=g) * amp).to(dtype)
    K, V = (torch.randn(B, HKV, SK, D, generator=g).to(dtype) for _ in range(2))
    dO = torch.randn(B, H, SQ, D, generator=g).to(dtype)
    vis = ar.visible(SQ, SK, WINDOW[0], WINDOW[1], "cpu")
    gt = ar.attention_fp64(Q, K, V, dO, SCALE, vis, **kw)
    plain = ar.attention_fp64(Q, K, V, None, SCALE, vis)["O"]
    few = bc.few_rows(vis)
    keyless = ~vis.any(-1)
    assert int(keyless.sum()) == 6 and int(few[0].sum()) == 7

    def check(got):
        return vck.check_training(feature, gt, got, dO, dtype, "ws", mod.REL, mod.RAW_BF16_DKV, mod.BOUNDS, plain, matters, few)

    def good():
        got = {n: gt[n].to(dtype) for n in ("O", "dQ", "dK", "dV")}
        got["LSE"] = gt["LSE"].float()
        return got
    errs = check(good())
    assert set(errs) == {"O", "dQ", "dK", "dV"} and max(errs.values()) <= mod.REL[dtype]

    row = int(keyless.nonzero()[0])
    mutations = {}
    mutations["a 32 x 32 block of dQ scaled by 1.02"] = got = good()
    got["dQ"][0, 1, 32:64, :32] *= 1.02
    mutations["a non-zero element in a keyless row of O"] = got = good()
    got["O"][0, 2, row, 5] = 1e-3
    mutations["an LSE row moved by 0.05"] = got = good()
    got["LSE"][0, 3, 40] += 0.05
    # without sinks a keyless row's LSE is -inf and a finite value is wrong; with them it is z and -inf is wrong
    mutations["a keyless row's LSE finite, or -inf under a sink"] = got = good()
    got["LSE"][0, 4, row] = float("-inf") if feature == "sink" else 0.0
    mutations["the untransformed O"] = got = good()
    got["O"] = plain.to(dtype)
    for what, got in mutations.items():
        try:
            check(got)
        except AssertionError:
            continue
        pytest.fail("check_training accepted " + what)
    # the "matters" assertion on its own: a truth that ignores the transform too passes every other check
    with pytest.raises(AssertionError, match="untransformed"):
        vck.check_training(feature, dict(gt, O=plain), got, dO, dtype, "ws", mod.REL, mod.RAW_BF16_DKV, mod.BOUNDS, plain,
                           matters, few)


def test_entry_calls_and_common_refusals_against_the_library():
    import _mi355fa as fa
    names = ["fa_fwd_alibi", "fa_bwd_dq_alibi", "fa_bwd_dkv_alibi", "fa_fwd_kvcache_alibi"]
    _buf, p = vck.aligned_ptr()
    assert p % 16 == 0
    calls = vck.entry_calls(fa.lib, names, p, B=2)
    assert list(calls) == names
    for name, f in calls.items():   # well-formed up to the last check before a launch: a window below -1
        assert f(0.125, (p, 0), 4, 2, -2, None) == fa.ERR_WINDOW, name
        assert f(0.125, (p, -1), 4, 2, -1, None) == fa.ERR_ALIBI, name   # the spliced arguments reach the library
    texts = vck.check_common_refusals(calls, (p, 0))
    assert list(texts) == names and all(b"H_kv" in t["group"] and b"dropout" in t["dropout"] for t in texts.values())
    with pytest.raises(AssertionError):   # a bad spliced argument is no common refusal: the helper notices
        vck.check_common_refusals(calls, (p, -1))
