"""CPU tests that pin the reach of tests/test_gpu_fp4_deep.py: the model of csrc/fa_decode_body.inc's tile and split arithmetic
(tests/test_host_paged.py's _work_items / deep_reach) over that module's own constants, at four tiles per loop step (D <= 128)
and at two (D = 256).  These are conditions on shapes, not measurements: the body looks a table entry up three steps ahead,
builds the page's descriptors -- with MXFP4, the two scale-pool descriptors and scale offsets too -- two steps ahead and loads
one ahead, so an entry looked up inside the loop feeds a load only in a wave that runs at least 4 loop steps, and the pipeline
is in steady state from about 8.  Whoever shrinks the shapes below that reach fails here, without a GPU.  The same model over
the shapes of tests/test_gpu_kvcache_fp4.py and tests/test_gpu_ragged_fp4.py shows what those modules cannot reach."""
import test_gpu_fp4_deep as fd
import test_gpu_kvcache_fp4 as t4
import test_gpu_ragged_fp4 as tr
import test_host_paged as hp

FORCED = [n for n in fd.SPLITS if n > 0]


def test_constants_are_the_ones_the_reach_was_worked_out_for():
    assert fd.GEOMS == [(32, 44), (96, 15), (128, 11), (160, 9), (224, 7)]
    assert [p // 32 for p, _ in fd.GEOMS] == [1, 3, 4, 5, 7]                         # FastDiv's multiply path at 3, 5, 7
    assert all(44 <= page * mp // 32 <= 49 for page, mp in fd.GEOMS)
    assert FORCED == [1, 2, 3, 5, 11] and 0 in fd.SPLITS
    assert fd.MASKS == t4.MASKS + [(False, (300, 8)), (True, (700, -1))]
    assert fd.GROUPS == [(4, 4), (8, 2), (8, 1)] and fd.SQS == (1, 3, 40)
    assert fd.S_PACKED == [1, 3, 0, 40, 130, 1, 9]
    # every geometry is run, the pages 96 and 128 with D and dtype crossed, and each D and dtype meets a geometry outside them
    assert {(page, mp) for page, mp, _, _ in fd.CONFIGS} == set(fd.GEOMS)
    for page in (96, 128):
        assert sorted((D, str(dt)) for p, _, D, dt in fd.CONFIGS if p == page) == \
            sorted((D, str(dt)) for D in (64, 128) for dt in (fd.F16, fd.BF16))
    rest = [(D, dt) for p, _, D, dt in fd.CONFIGS if p not in (96, 128)]
    assert {D for D, _ in rest} == {64, 128} and {dt for _, dt in rest} == {fd.F16, fd.BF16}
    assert len(fd.PACKED_GEOMS) == 4 and all((p, m) in fd.GEOMS and D in (64, 128) for p, m, D, _ in fd.PACKED_GEOMS)
    assert [(p, D) for p, _, D, _ in fd.PACKED_256] == [(32, 256), (96, 256), (224, 256)]
    assert all((p, m) in fd.GEOMS for p, m, _, _ in fd.PACKED_256)
    for page, mp in fd.GEOMS:
        assert len(fd.packed_lens(page, mp)) == len(fd.S_PACKED)


def test_deep_shapes_reach_the_steady_state_of_the_lookup_pipeline():
    reach = hp.deep_reach(fd.GEOMS, fd.lengths, fd.GROUPS, fd.SQS, fd.MASKS, FORCED)
    assert sorted(reach) == sorted(fd.GEOMS)
    for (page, mp), (longest, longest3, midpage, last_third) in reach.items():
        assert longest >= 8, (page, mp, longest)                                    # 1. some wave runs at least 8 steps
        assert longest3 >= 4, (page, mp, longest3)                                  # 2. and at least 4 at three splits
        assert midpage or page == 32, (page, mp)                                    # 3. a split of >= 4 steps begins mid-page
        assert last_third, (page, mp)                                               # 4. a first tile in the table's last third
    # the same lists with max_pages cut to 3 reach none of the first two
    for (page, mp), (longest, longest3, _, _) in hp.deep_reach([(p, 3) for p, _ in fd.GEOMS], fd.lengths, fd.GROUPS, fd.SQS,
                                                               fd.MASKS, FORCED).items():
        assert longest < 8 and longest3 < 4, (page, longest, longest3)


def packed_reach(page, mp, S, lens, ng):
    """test_host_paged.packed_reach over this module's head groups, masks and packed split counts"""
    return hp.packed_reach(page, mp, S, lens, ng, fd.GROUPS, fd.MASKS, fd.PACKED_SPLITS)


def test_packed_shapes_reach_it_at_four_and_at_two_tiles_per_step():
    assert fd.PACKED_SPLITS == (1, 3, 11)
    for rows, ng in ((fd.PACKED_GEOMS, 4), (fd.PACKED_256, 2)):
        for page, mp, D, _ in rows:
            assert (D == 256) == (ng == 2)
            longest, longest3, midpage, last_third = packed_reach(page, mp, fd.S_PACKED, fd.packed_lens(page, mp), ng)
            assert longest >= 8 * (4 // ng), (page, D, longest)                     # at D = 256 the same tiles are twice the steps
            assert longest3 >= 4, (page, D, longest3)
            assert midpage or page == 32, (page, D)
            assert last_third, (page, D)
            # D = 256: an odd share of at least 4 steps (on its last step one pair only joins the barrier)
            if ng == 2:
                assert any(steps >= 4 and tiles % 2 == 1
                           for L, Sq in zip(fd.packed_lens(page, mp), fd.S_PACKED) if Sq
                           for n in fd.PACKED_SPLITS for steps, tiles in _shares(L, n)), (page, D)


_shares = hp.shares


def test_the_older_mxfp4_modules_stop_short_of_it():
    """The teeth: the same model over the shapes of the two older MXFP4 modules.  Their longest waves are 2 steps (padded and
    packed, D <= 128), 3 (the paged case at page 96, 9 tiles) and 4 (D = 256, two tiles per step): the in-loop lookup, which
    needs 13 tiles in one split at D <= 128, never runs there, and the in-loop page_desc once at most."""
    old_splits = (1, 2, 3)
    groups = sorted({(H, Hkv) for H, Hkv, _ in t4.GEOMS} | {(4, 2), (8, 2)})
    sqs = sorted({Sq for _, _, Sq in t4.GEOMS})
    assert t4.SC == 224 and max(t4.LENS) == 200 and max(tr.LENS) == 200
    # padded: LENS, and the append that fills the cache to its end
    padded = hp.deep_reach([(32, 7)], lambda page, mp: t4.LENS + [t4.SC], groups, sqs, t4.MASKS, old_splits)[(32, 7)]
    assert padded[0] == 2, padded
    # paged: test_paged_has_the_bits_of_the_padded_call_on_the_gathered_cache, pages of 32 and 96 keys, fill levels after the append
    for page in (32, 96):
        mp = -(-t4.SC // page)
        fills = lambda page, mp: [L + 3 for L in (1, page - 1, 129, mp * page - 3, 40, 0)]
        got = hp.deep_reach([(page, mp)], fills, [(4, 2)], [3], t4.MASKS, old_splits)[(page, mp)]
        assert got[0] == {32: 2, 96: 3}[page], (page, got)
    # packed: S over LENS, with room for the appends (the graph test advances 200 by at most 3 * max(S) keys: still 7 tiles)
    grown = [L + 3 * max(tr.S) for L in tr.LENS]
    assert -(-max(grown) // 32) == 7
    for ng, want in ((4, 2), (2, 4)):
        longest = 0
        for lens in (tr.LENS, grown):
            for L, Sq in zip(lens, tr.S):
                for g in sorted({H // Hkv for H, Hkv in tr.GEOMS} | {4}):
                    for is_causal, window in tr.MASKS:
                        for n in old_splits:
                            for _, _, steps in hp._work_items(L, max(Sq, 1), g, *t4.window_of(is_causal, window), n, ng):
                                longest = max(longest, max(steps))
        assert longest == want, (ng, longest)
