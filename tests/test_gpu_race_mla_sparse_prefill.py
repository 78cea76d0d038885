"""The poisoned and decoyed repeat-launch check (tests/racecheck.py, as tests/test_gpu_race_mla_indexer_prefill.py applies it) on
the sparse prefill kernel: 19 tokens (ids past M in the last group of 8) x 40 heads (two head blocks, the second partial) over
lists of 160 entries, five steps through the two-barrier softmax exchange.  Its own control."""
import pytest
import torch

import mlacheck as mc
import mlasparsecheck as msc
import racecheck as rc

pytestmark = pytest.mark.gpu


def test_poisoned_and_decoyed_launches_repeat_bit_for_bit():
    import mla_sparse_prefill as P
    M, H, N, topk = 19, 40, 300, 160

    def problem(dtype, seed):
        q4, kv3 = mc.make(1, H, M, N, dtype, seed=seed)
        return q4, kv3, msc.draw([N], M, topk, seed=seed + 1).cuda()

    def launch(q4, kv3, idx):
        q = q4[0].transpose(0, 1)
        return lambda xs: xs[1].copy_(P.flash_attention_mla_sparse_prefill(q, kv3[0], idx[0], return_lse=True, out=xs[0])[1])
    p, d = problem(mc.BF16, 61), problem(mc.F16, 71)                  # (the decoy: other data through the other instance)
    outs = [rc.Out("o", torch.empty(M, H, mc.DV, dtype=mc.BF16, device="cuda")), rc.Out("lse", torch.empty(M, H, device="cuda"))]
    douts = lambda: [torch.empty(M, H, mc.DV, dtype=mc.F16, device="cuda"), torch.empty(M, H, device="cuda")]
    case = dict(id="mla-sparse-prefill", stems=["fa_decode_paged_kernel"])
    for mode in rc.MODES:
        res = rc.check(case, launch(*p), outs, mode, decoy=lambda: launch(*d)(douts()), runs=40)
    o, lse = res["plain"]
    msc.held(case["id"], msc.reference(*p, [N], False), (o.transpose(0, 1)[None], lse.t()[None]))
