"""CPU tests of the inputs of tests/test_gpu_groups.py: with the parameters chosen in tests/groups_ref.py (the cap, the
sinks, the ALiBi slopes) every score transform moves the fp64 output by its file's threshold at every geometry, and in
ALiBi decoding some visible key lies right of its query and that side matters; the geometries have the row-block
properties they are there for, and the cache "after the append" that the GPU file compares bits with is the padded cache
plus exactly the new rows.  No compute is launched on a GPU here."""
import pytest
import torch

import groups_ref as gr

F16, BF16 = gr.F16, gr.BF16


def test_geometries_cut_their_row_blocks_where_they_should():
    for H, Hkv, Sq in gr.GEOMS:
        g = H // Hkv
        assert H % Hkv == 0 and gr.row_blocks((H, Hkv, Sq)) >= 2
        if g & (g - 1):
            assert 32 % g != 0        # a 32-row boundary falls inside a query's heads
    assert sorted({H // Hkv for H, Hkv, _ in gr.GEOMS}) == [1, 3, 4, 5, 7, 12]
    assert all(Sq > 1 + 2 for _, _, Sq in gr.GEOMS if Sq != 3)
    # S_new alternates over the parametrisations of every (kind, geometry)
    for gi in range(len(gr.GEOMS)):
        assert {gr.s_new(gi, dt, D) for dt in (F16, BF16) for D in (64, 128)} == {0, 2}


@pytest.mark.parametrize("H", sorted({H for H, _, _ in gr.GEOMS}))
def test_slopes_and_sinks_are_distinct(H):
    s = gr.slopes_of(H)
    assert s.shape == (gr.B, H) and s.dtype == torch.float32 and s.flatten().unique().numel() == gr.B * H
    assert (s >= gr.SLOPE_LO).all()
    z = gr.sinks_of(H)
    assert z.unique().numel() == H and z[0] == gr.SINK_LO and z[-1] == gr.SINK_HI
    if H > 2:   # neighbouring heads are far apart: a neighbour's slope is a gross error
        assert (s[:, 1:] - s[:, :-1]).abs().min() >= 0.1


@pytest.mark.parametrize("kind", ["plain", "fp8_sink"])
def test_cache_after_the_append_is_the_padded_cache_plus_the_new_rows(kind):
    c = gr.make_case(kind, gr.GEOMS[0], BF16, 64, 2, "cpu")
    for b, (L0, L) in enumerate(zip(gr.FILL, c.Ls)):
        for before, after, ref in ((c.kc, c.k_after, c.kr), (c.vc, c.v_after, c.vr)):
            assert torch.equal(gr._bits(before)[b, :, :L0], gr._bits(after)[b, :, :L0])
            assert torch.isnan(after[b, :, L:].double()).all() and not torch.isnan(after[b, :, :L].double()).any()
            assert (ref[b, :, L:] == 0).all()
        new = c.kr[b, :, L0:L]
        if kind == "plain":
            assert torch.equal(new, c.kn[b].double())
        else:   # e4m3 under the cache's descale: within half a step of 2^-3 relative, or of the smallest step
            d = c.kd[b].double().reshape(-1, 1, 1)
            assert ((new - c.kn[b].double()).abs() <= (c.kn[b].double().abs() * 2.0 ** -4).clamp_min(d * 2.0 ** -10)).all()


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("gi", range(len(gr.GEOMS)), ids=[gr.geom_id(g) for g in gr.GEOMS])
@pytest.mark.parametrize("kind", sorted(gr.MATTERS))
def test_the_transform_matters_at_every_geometry(kind, gi, dtype, D):
    """The conditions test_gpu_groups.py asserts before it looks at the kernel's output, on the same inputs."""
    c = gr.make_case(kind, gr.GEOMS[gi], dtype, D, gr.s_new(gi, dtype, D), "cpu")
    truths = {w: gr.truth(c, w) for w in gr.WINDOWS}
    fig = gr.check_conditions(c, truths)
    print(kind, gr.geom_id(c.geom), dtype, D, " ".join("%s=%.3f" % kv for kv in fig.items()))
    assert "matters" in fig and (kind != "alibi" or len(fig) == 3)
    # L = 0 without an append is a sequence without keys; under window_right = 0 the rows at negative positions are keyless
    nokey = truths[(-1, 0)].nokey
    assert nokey.any() and not nokey.all()
    if c.snew == 0:
        assert truths[(-1, -1)].nokey[0].all()
