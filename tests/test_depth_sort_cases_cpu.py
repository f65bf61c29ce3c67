"""The depth-sort frames of tests/depth_sort_cases.py are what they claim to be: on the CPU oracle every tile's list has
exactly the designed length, every depth is the designed float32 bit for bit, the restated host rule picks the route each
frame was built for, and the frames together stand on every size edge, pattern and fallback of csrc/binning.hip's
per-tile sort.  (The GPU side is tests/test_depth_sort_gpu.py.)"""
import numpy as np
import pytest

import depth_sort_cases as dc

FRAMES = list(dc.FRAME_SPECS)


@pytest.mark.parametrize("name", FRAMES)
def test_frame_bins_to_the_designed_lists(name):
    fr = dc.build(name)
    geom, binning = dc.reference(name)
    T = (fr.W // 16) * (fr.H // 16)
    assert fr.lengths.shape == (T,) and fr.P == int(fr.lengths.sum()) and fr.P <= 70_000
    assert bool(geom.visible.all()) and int(geom.radii.max()) <= 3 and int(geom.radii.min()) >= 1
    assert np.array_equal(geom.tiles_touched, np.ones(fr.P, dtype=np.uint32))          # each touches its own tile only
    assert np.array_equal(geom.depth.view(np.uint32), fr.z.view(np.uint32))
    got = (binning.ranges[:, 1] - binning.ranges[:, 0]).astype(np.int64)
    assert np.array_equal(got, fr.lengths), (got, fr.lengths)
    assert binning.num_rendered == fr.route["L"] == fr.P
    # the tile each list sits in, and its order: (depth bits, id) ascending
    for tile, n, _ in fr.entries:
        r0, r1 = binning.ranges[tile]
        ids = binning.point_list[r0:r1].astype(np.int64)
        assert np.array_equal(fr.tile_of[ids], np.full(n, tile))
        key = (fr.z[ids].view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)
        assert bool((key[1:] > key[:-1]).all())


@pytest.mark.parametrize("name", FRAMES)
def test_frame_takes_the_route_it_was_built_for(name):
    fr = dc.build(name)
    r = fr.route
    assert r["name"] == dc.FRAME_ROUTES[name], r
    assert r["quad"] == (r["L"] > 512 * r["T"]) and r["heavy"] == (r["L"] > 1024 * r["T"])
    n = fr.lengths
    if r["quad"]:
        assert r["large"] == int(((n > 4096) & (n <= 16384)).sum()) and r["huge"] == int((n > 16384).sum())
    else:
        assert r["large"] == 0 and r["huge"] == 0
    # the speculative forward routes by its capacity (at least SPEC_SLACK = 65536): quad and heavy on these grids
    assert 65536 > 1024 * r["T"]
    if fr.family in ("light", "quad", "heavy"):
        assert r["name"] == fr.family
        assert fr.zero_fallbacks and fr.min_fallbacks == 0


@pytest.mark.parametrize("name", FRAMES)
def test_patterns_hold_what_they_promise(name):
    fr = dc.build(name)
    _, binning = dc.reference(name)
    for tile, n, p in fr.entries:
        if n == 0:
            continue
        r0, r1 = binning.ranges[tile]
        z = fr.z[binning.point_list[r0:r1]]
        assert float(z.min()) > 0.2
        counts = np.unique(z, return_counts=True)[1]
        assert int(counts.max()) == dc.MULTIPLICITY[p](n), (name, tile, p)
        bits = z.view(np.uint32).astype(np.int64)
        if p == "wide":
            assert bits.max() - bits.min() > 1 << 24
        if p == "ulps":
            assert bits.max() - bits.min() == n - 1
        if p == "outlier":
            assert int((z == np.float32(1000.0)).sum()) == 1 and float(np.sort(z)[-2]) <= 5.0 * (1 + 1.001e-3)
        if p in ("block65", "block64"):
            assert int((counts > 1).sum()) == 1
    assert (fr.min_fallbacks > 0) == any(p in dc.MUST_FALL_BACK and dc.sample_sort_class(n, fr.route["quad"])
                                         for _, n, p in fr.entries)


def _covered(edge):
    want_route, n, p = edge
    return [name for name in FRAMES
            if dc.build(name).route["name"] in want_route.split("|") and
            any(en == n and ep == p for _, en, ep in dc.build(name).entries)]


@pytest.mark.parametrize("edge", dc.EDGES, ids=lambda e: "%s-%d-%s" % e)
def test_every_edge_is_in_a_frame_of_its_route(edge):
    assert _covered(edge), f"no frame of route {edge[0]} holds a {edge[2]} list of {edge[1]}"


def test_edge_table_names_every_tier_edge_of_the_kernels():
    """The table itself against the restated constants: both sides of every tier edge, in the kernel that owns the tier."""
    have = {(r, n) for r, n, p in dc.EDGES if p == "smooth"}
    for e in (dc.K_NETWORK,) + dc.ONE_WAVE_EDGES[:4]:                      # light kernel: 128, 192, 256, 384, 512
        assert ("light", e) in have and ("light", e + 1) in have, e
    assert ("light", dc.K_WAVE) in have
    for e in dc.ONE_WAVE_EDGES[4:] + dc.FOUR_WAVE_EDGES:                   # quad kernel: 768 .. 4096
        assert ("quad", e) in have and ("quad", e + 1) in have, e
    for e in (dc.K_QUAD, dc.K_MID, dc.K_LARGE):                            # mid / big / huge on a heavy frame
        assert ("heavy", e + 1) in have, e
    assert ("heavy", dc.K_MID) in have and ("heavy", dc.K_LARGE) in have
    assert ("quad", dc.K_MID + 1) in have                                  # big kernel with large_lo = 0
    # every sorter the restated rule knows is reached by some frame
    reached = {dc.sorter(n, dc.build(name).route) for name in FRAMES for _, n, _ in dc.build(name).entries}
    want = {"none", "network2", "network16", "radix4", "radix16", "coop8", "coop16"}
    want |= {"sample1/kpl%d" % k for k in (3, 4, 6, 8, 12, 16)} | {"sample4/kpl%d" % k for k in (5, 6, 8, 10, 12, 16)}
    assert want <= reached, want - reached


def test_special_workgroups_are_present():
    assert any(dc.build(n).route["T"] % 4 for n in dc.family_frames("light"))             # the `tile < T` guard
    two = dc.build("light_two_crowded")
    assert not two.route["quad"] and int((two.lengths[:4] > 1024).sum()) == 2
    big = [int(dc.build(n).lengths.max()) for n in dc.family_frames("light")]
    assert any(1024 < b <= 4096 and b % 256 for b in big) and any(b > 4096 for b in big)
    q = dc.build("quad_tiers")
    first = q.lengths[:4]
    assert int(((first > 1024) & (first <= 4096)).sum()) >= 2 and int((first == 0).sum()) >= 1
    h = dc.build("heavy_classes")
    assert h.route["heavy"] and h.route["huge"] == 1 and int(((h.lengths > 1024) & (h.lengths <= 4096)).sum()) >= 2
