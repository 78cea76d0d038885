"""Race tests of the decode path (run with -m gpu on an MI355X) under the poisoned and the decoy repeat of
tests/racecheck.py.  The poison (or the decoy call) runs once before each WHOLE call; the call's own kernels -- the
append, the ragged plan, the decode kernel, the combine -- then run back to back on one stream, as in production.  The raw
C entry points are used throughout, so that o, lse and the split workspace (with the ragged plan in it) are the caller's
and are filled with 0xFF bytes before every call; the caches are fresh clones of NaN-padded caches (NaN pages and NaN
tails of last pages for a pool) and must equal the reference cache byte for byte after every call.

Geometry: variantcheck.decode_case's -- B3, H8, H_kv 2, 700 cache rows, fill levels 0 / 300 / 650, 2 appended keys; forced
splits 0 / 1 / 3 / 7 and S_q 1 / 4 / 9 (two row blocks at g = 4), all twelve pairs in every case; D 64 and 128, both dtypes.
Padded 16-bit caches: plain, soft-cap, ALiBi, sink; padded e4m3: plain, sink; paged: all six at page 32 and 64, each page
size at both head dims and dtypes, through a permuted table (pagedcheck.scatter); ragged: plain and fp8_sink in the same
eight instances, every split count, with the query counts [0, 1, 9, 3] over fill levels 300 / 0 / 650 / 40 and 5 rows past
cu[B], which must keep their fill; the window (200, 0); a transposed [B, S, H_kv, D] cache.  The control is the same call
at one forced split.  On one MI355X this file takes about 46 s (at most 0.7 s per case).
"""
import pytest

import racecases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in rc.DECODE_CASES])
def test_decode_call_repeats_its_bits_under_poison_and_decoy(case):
    rc.run_decode_case(case)
