"""CPU tests that pin the reach of tests/test_gpu_fp8_token_deep.py: the model of csrc/fa_decode_body.inc's tile and split
arithmetic (tests/test_host_paged.py's _work_items / deep_reach / packed_reach) over that module's own constants, at four tiles
per loop step (D <= 128) and at two (D = 256).  These are conditions on shapes, not measurements: the body looks a table entry
up three steps ahead, builds the page's descriptors -- with a per-token-scaled cache, the two descriptors of the fp32 scale pools
and the two scale offsets too -- two steps ahead and loads one ahead, so an entry looked up inside the loop feeds a load only in
a wave that runs at least 4 loop steps, and the pipeline is in steady state from about 8.  Whoever shrinks the shapes below that
reach fails here, without a GPU.  The same model over the shapes of tests/test_gpu_kvcache_fp8_token.py and
tests/test_gpu_ragged_fp8_token.py shows what those modules cannot reach."""
import test_gpu_fp8_token_deep as td
import test_gpu_kvcache_fp8_token as tt
import test_gpu_ragged_fp8_token as tr
import test_host_paged as hp
from test_gpu_kvcache import window_of

FORCED = [n for n in td.SPLITS if n > 0]


def test_constants_are_the_ones_the_reach_was_worked_out_for():
    assert td.GEOMS == [(32, 44), (96, 15), (128, 11), (160, 9), (224, 7)]
    assert [p // 32 for p, _ in td.GEOMS] == [1, 3, 4, 5, 7]                         # FastDiv's multiply path at 3, 5, 7
    assert all(44 <= page * mp // 32 <= 49 for page, mp in td.GEOMS)
    assert FORCED == [1, 2, 3, 5, 11] and 0 in td.SPLITS
    assert td.MASKS == tt.MASKS + [(False, (300, 8)), (True, (700, -1))] and len(tt.MASKS) == 3
    assert td.GROUPS == [(4, 4), (8, 2), (8, 1)] and td.SQS == (1, 3, 40)
    assert td.S_PACKED == [1, 3, 0, 40, 130, 1, 9] and td.PACKED_SPLITS == (1, 3, 11)
    # every geometry is run, the pages 96 and 128 with D and dtype crossed, and each D and dtype meets a geometry outside them
    assert {(page, mp) for page, mp, _, _ in td.CONFIGS} == set(td.GEOMS)
    for page in (96, 128):
        assert sorted((D, str(dt)) for p, _, D, dt in td.CONFIGS if p == page) == \
            sorted((D, str(dt)) for D in (64, 128) for dt in (td.F16, td.BF16))
    rest = [(D, dt) for p, _, D, dt in td.CONFIGS if p not in (96, 128)]
    assert {D for D, _ in rest} == {64, 128} and {dt for _, dt in rest} == {td.F16, td.BF16}
    assert td.PACKED_GEOMS == [(32, 44, 64, td.F16), (96, 15, 128, td.BF16), (128, 11, 128, td.F16), (224, 7, 64, td.BF16)]
    assert td.PACKED_256 == [(32, 44, 256, td.F16), (96, 15, 256, td.BF16), (224, 7, 256, td.F16)]
    for page, mp in td.GEOMS:
        assert len(td.packed_lens(page, mp)) == len(td.S_PACKED)
    # the inputs' condition and the bounds are the issue's and the project's
    assert (td.K_SPAN, td.V_SPAN, td.SMALL_V) == ((-6.0, 1.0), (-6.0, 6.0), (-6.0, -6.0)) and (td.BROAD, td.BROAD_FROM) == (0.05, 256)
    assert td.BOUND == {td.F16: 1e-3, td.BF16: 8e-3}
    # the soft-capped cases: the pages test_gpu_kvcache_quant_softcap.py's deep case (page 96) leaves out, both D and both dtypes
    assert [(p, mp) for p, mp, _, _ in td.CAPPED] == [(32, 44), (160, 9), (224, 7)] and td.CAP == 30.0
    assert {D for _, _, D, _ in td.CAPPED} == {64, 128} and {dt for _, _, _, dt in td.CAPPED} == {td.F16, td.BF16}
    assert td.CAPPED_PACKED == [(96, 15, 256, td.BF16), (224, 7, 128, td.F16)]
    assert td.CAPPED_SQS == (3, 40) and td.CAPPED_GROUPS == [(8, 2), (8, 1)]


def test_deep_shapes_reach_the_steady_state_of_the_lookup_pipeline():
    reach = hp.deep_reach(td.GEOMS, td.lengths, td.GROUPS, td.SQS, td.MASKS, FORCED)
    assert sorted(reach) == sorted(td.GEOMS)
    for (page, mp), (longest, longest3, midpage, last_third) in reach.items():
        assert longest >= 8, (page, mp, longest)                                    # 1. some wave runs at least 8 steps
        assert longest3 >= 4, (page, mp, longest3)                                  # 2. and at least 4 at three splits
        assert midpage or page == 32, (page, mp)                                    # 3. a split of >= 4 steps begins mid-page
        assert last_third, (page, mp)                                               # 4. a first tile in the table's last third
    # the same lists with max_pages cut to 3 reach none of the first two
    for (page, mp), (longest, longest3, _, _) in hp.deep_reach([(p, 3) for p, _ in td.GEOMS], td.lengths, td.GROUPS, td.SQS,
                                                               td.MASKS, FORCED).items():
        assert longest < 8 and longest3 < 4, (page, longest, longest3)
    # the soft-capped cases run a subset of these lists: they reach it on their own
    for (page, mp), (longest, longest3, midpage, last_third) in hp.deep_reach(
            [(p, mp) for p, mp, _, _ in td.CAPPED], td.lengths, td.CAPPED_GROUPS, td.CAPPED_SQS, td.MASKS, td.PACKED_SPLITS).items():
        assert longest >= 8 and longest3 >= 4 and (midpage or page == 32) and last_third, (page, mp)


def test_packed_shapes_reach_it_at_four_and_at_two_tiles_per_step():
    for rows, ng, groups in ((td.PACKED_GEOMS, 4, td.GROUPS), (td.PACKED_256, 2, td.GROUPS),
                             ([c for c in td.CAPPED_PACKED if c[2] != 256], 4, td.CAPPED_GROUPS),
                             ([c for c in td.CAPPED_PACKED if c[2] == 256], 2, td.CAPPED_GROUPS)):
        assert rows
        for page, mp, D, _ in rows:
            assert (D == 256) == (ng == 2)
            lens = td.packed_lens(page, mp)
            longest, longest3, midpage, last_third = hp.packed_reach(page, mp, td.S_PACKED, lens, ng, groups, td.MASKS, td.PACKED_SPLITS)
            assert longest >= 8 * (4 // ng), (page, D, longest)                     # at D = 256 the same tiles are twice the steps
            assert longest3 >= 4, (page, D, longest3)
            assert midpage or page == 32, (page, D)
            assert last_third, (page, D)
            # D = 256: an odd share of at least 4 steps (on its last step one pair only joins the barrier)
            if ng == 2:
                assert any(steps >= 4 and tiles % 2 == 1 for L, Sq in zip(lens, td.S_PACKED) if Sq
                           for n in td.PACKED_SPLITS for steps, tiles in hp.shares(L, n)), (page, D)


def test_out_of_range_entries_sit_where_a_wave_looks_them_up_inside_its_loop():
    """test 7 of the GPU module: at one split the entry of a tile t >= 3 NG comes from the loop's page_of(t + 3 NG), so an entry
    at table position i, whose first tile is i * (page // 32), is looked up inside the loop when that is at least 3 NG"""
    page, mp = 96, 15
    where = td.out_of_range_positions(page, mp)
    assert where == [(1, 0), (1, 6), (1, 7), (3, 1), (3, 14), (3, 7)]
    for NG in (4, 2):
        assert sum(i * (page // 32) >= 3 * NG for _, i in where) >= 4, NG
    assert td.GUARD == 4


def _longest(cases, ng):
    """the longest wave over (L, S_q, g, masks, split counts) cases"""
    longest = 0
    for L, Sq, g, masks, splits in cases:
        for is_causal, window in masks:
            for n in splits:
                for _, _, steps in hp._work_items(L, Sq, g, *window_of(is_causal, window), n, ng):
                    longest = max(longest, max(steps))
    return longest


def test_the_older_per_token_modules_stop_short_of_it():
    """The teeth: the same model over the shapes of the two older per-token modules (forced split counts; the formula's count is
    one of them or gives shorter waves).  At four tiles a step (D <= 128) their longest wave is 3 steps -- 9 and 10 tiles -- so
    the in-loop lookup, which needs 13 tiles in one split, never runs there and the in-loop page_desc once per wave.  At two
    tiles a step (D = 256) every test but one stops at 3 steps as well; the graph replay of tests/test_gpu_ragged_fp8_token.py
    runs 275, 288 and 320 keys at D = 256 and so reaches 5 steps -- one in-loop lookup that feeds a load, at page 64 (a shift)
    and the formula's split count only."""
    forced = [n for n in tt.SPLITS if n > 0]
    assert forced == [1, 2, 3] and [n for n in tr.SPLITS if n > 0] == forced
    assert tt.SC == tr.SC == 320 and max(tt.TILES + tt.ODD) == 288 and (tt.H, tt.HKV) == (tr.H, tr.HKV) == (8, 2)
    # padded and paged, D <= 128: every length up to the whole cache (the graph test fills it), S_q 1, 3, 9, H_kv 2 and MQA
    lens = sorted(set(tt.TILES + tt.ODD + [f + s for f in (31, 126, 0, 285) for s in (1, 3)] + [tt.SC, 1, 33, 64]))
    cases = [(L, Sq, g, tt.MASKS, forced) for L in lens for Sq in (1, 3, 9) for g in (4, 8)]
    assert _longest(cases, 4) == 3
    # packed, D <= 128
    assert max(max(v) for v in tr.LENS.values()) == 288 and tr.S == [9, 3, 1, 3]
    grown = [f + s for f, s in zip((30, 126, 0, 150), tr.S)]
    cases = [(L, Sq, 4, tt.MASKS, forced) for D in (64, 128) for L, Sq in list(zip(tr.LENS[D], tr.S)) + list(zip(grown, tr.S)) if Sq]
    assert _longest(cases, 4) == 3
    # packed, D = 256: the fp64 test, the sequence without queries (288 keys: no work), the unit scales, the append
    pairs = list(zip(tr.LENS[256], tr.S)) + list(zip([64, 288, 160, 96], [3, 0, 1, 9])) + list(zip(grown, tr.S))
    assert max(L for L, Sq in pairs if Sq) == 160
    assert _longest([(L, Sq, 4, tt.MASKS, forced) for L, Sq in pairs if Sq], 2) == 3
    # and the graph replay, causal only
    replay = list(zip(tr.LENS[256], tr.S)) + list(zip([275, 0, 160, 288], [3, 9, 1, 3])) + list(zip([320, 1, 33, 64], [1, 1, 13, 1]))
    assert _longest([(L, Sq, 4, [(True, (-1, -1))], [1]) for L, Sq in replay if Sq], 2) == 5
