"""Race tests of every schedule family at edge shapes (run with -m gpu on an MI355X): the plain entry points fa_fwd,
fa_bwd_dq and fa_bwd_dkv with the family forced through fa_debug_force_impl, under the poisoned and the decoy repeat of
tests/racecheck.py (120 launches per mode, every result the bits of the first and of an undisturbed launch, the
undisturbed result against attn_ref.attention_fp64 under tests/test_gpu_families.py's bounds).  fa_debug_pick and
fa_debug_pick_ex must answer the forced family for every case: an assertion, checked on the CPU too
(tests/test_host_racecheck.py).

Edge shapes are where a counted wait miscounts: its count depends on the pieces in flight, and that changes with one or
two tiles, with fewer tiles than the ring is deep, with a ragged last tile and on a pass's first and last tile.  For each
kernel instance (family, D, dtype, mask), with T the streamed tile and R the ring depth of its *Cfg (racecases.GEOMETRY; the
streamed side is the keys for the forward and dQ, the queries for dK/dV) and BM its workgroup tile on the resident side,
all at B2.H3 unless said:
  ladder      1, 2, R and R + 1 streamed tiles, each in whole tiles (n T) and with a ragged tail (n T - 11); the resident
              side BM + 37 rows, or under the causal mask S_q = S_k (workgroups then stream 1 .. n tiles);
  resident    one partial block (37 rows) and two workgroup tiles plus a remainder (2 BM + 37);
  causal      S_q < S_k and S_q > S_k;
  busy        B 4 or more, H 32, S about 1000: more than 512 workgroups, at least R + 1 tiles;
  family 4    only what fa_kernels.h pick_*_impl admits -- its smallest admissible multiples (causal: S_k a multiple of 256 at
              or above S_q; dQ: whole 128-key tiles; dK/dV: whole 128-row and 256-key tiles, causal S_q >= S_k, bf16; there
              S_q = 384, 640 and 768 over S_k = 256 stream 1, R and R + 1 query tiles behind a key tile's two diagonal ones,
              which S_q in multiples of 256 never does) -- and three persistent grids at the smallest S: fewer
              work items than the 256 workgroups (every B2.H3 case), 384 items (one or two passes per workgroup) and 800 items (three or four).
On one MI355X this file takes about 24 s (0.02-0.2 s per case, the fp64 check included).
"""
import pytest

import racecases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in rc.FAMILY_CASES])
def test_forced_family_repeats_its_bits_under_poison_and_decoy(case):
    rc.run_family_case(case)
