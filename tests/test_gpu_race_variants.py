"""Race tests of the family-1 kernels behind the score variants, dropout and packed batches (run with -m gpu on an MI355X),
under the poisoned and the decoy repeat of tests/racecheck.py, one kernel at a time: the forward, dQ and dK/dV instances
of fa_*_mod_kernel through variantcheck.raw_run -- sliding window (fa_*_local), GQA with g = 4 and g = 3, soft-cap, ALiBi,
sinks (and fa_bwd_dsink) -- at B2, H6 (H8 at g = 4), H_kv 2 (6 for the window alone), S_q 200, S_k 333, D 64 and 128,
both dtypes, the windows (-1, -1), (-1, 0), (70, 0) and (40, 25), bf16 with and without the q_scaled workspace (the dQ
kernel writes it: an output there; the dK/dV kernel reads it); fa_*_dropout (p = 0.25, fixed seed and offset); the causal
packed batch [(0, 5), (37, 37), (200, 333), (64, 1)] through fa_*_varlen, and once more through the GQA g = 3 instance.
What the later kernels read (O, LSE, delta, q_scaled) comes from one undisturbed run.  The undisturbed result of each
case is held to the bounds of the variant's own test file.  On one MI355X this file takes about 14 s.
"""
import pytest

import racecases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in rc.VARIANT_CASES])
def test_variant_kernel_repeats_its_bits_under_poison_and_decoy(case):
    rc.run_variant_case(case)
