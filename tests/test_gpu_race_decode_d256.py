"""Race tests of the D = 256 decode kernels (run with -m gpu on an MI355X) under the poisoned and the decoy repeat of
tests/racecheck.py, as tests/test_gpu_race_decode.py runs the other head dims: the cases have the shape of
racecases.DECODE_CASES entries and go through racecases.run_decode_case, which also holds the unpoisoned result to fp64.

At D = 256 the two waves of a pair hand each other their halves of the scores through LDS slots behind one workgroup barrier
per step, and two key groups merge where the other head dims merge four waves (csrc/fa_decode_body.inc, "D = 256"): both
are hand-offs through shared LDS that the NaN poison left there by the previous launch, or the decoy's other data, would
show if a barrier were missing.  Padded: all six variants; paged: plain and fp8_sink at page 32 and 64; ragged: plain and
fp8_sink at page 32; both dtypes, every (forced splits, S_q) pair of racecases.DECODE_CONFIGS (ragged: every split count)."""
import itertools

import pytest
import torch

import racecases as rc

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
D = 256


def _case(layout, variant, dtype, page=0):
    configs = [(n, None) for n in rc.DECODE_SPLITS] if layout == "ragged" else rc.DECODE_CONFIGS
    cid = "%s-%s-d%d-%s" % (layout, variant, D, rc.DT[dtype]) + ("-page%d" % page if page else "")
    return dict(id=cid, layout=layout, variant=variant, D=D, dtype=dtype, configs=configs, window=(-1, -1), page=page,
                transposed=False, stems=rc._decode_stems(layout, variant, [n for n, _ in configs]))


CASES = [_case("padded", v, dt) for v, dt in itertools.product(rc.DECODE_VARIANTS, (F16, BF16))] + \
        [_case("paged", v, dt, page) for v, page, dt in itertools.product(("plain", "fp8_sink"), (32, 64), (F16, BF16))] + \
        [_case("ragged", v, dt, 32) for v, dt in itertools.product(("plain", "fp8_sink"), (F16, BF16))]


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in CASES])
def test_d256_decode_call_repeats_its_bits_under_poison_and_decoy(case):
    rc.run_decode_case(case)
