"""Trimming to the detail a set of views can reach (hgs.hierarchy.view_reach / trim_to_views, the numpy specs of
csrc/hier_reach.hip and of the keyed plan of csrc/hier_trim.hip) without a GPU.

The contract checked here: take any float32 viewpoint v inside any region of the view set, borders included, and any
granularity tau' >= result.tau.  Then result.exact_for(v, tau') is true, and the cut of the trimmed hierarchy (indices,
weight bit patterns, sibling counts) is the original's mapped through new_of_old.  It rests on four properties of the
reach, each a test below: (1) for a point region the reach term is lod_oracle.node_size bit for bit; (2) reach is the
maximum of the per-region terms bit for bit, so one sqrt and one division per node suffice; (3) no viewpoint inside a
region sees a node larger than the region's term; (4) where boxes nest and extents do not grow downwards, a parent's
reach is at least its child's, in float32.  Every comparison is on bits or integers.

Also: the documented sizes, the budget (a granularity, ties together, at most K nodes), a hand-built tree read by eye,
a hierarchy whose boxes do not nest, the C ABI's three additions, the command's parser and its cameras.json reader.
tests/test_trim_to_views_gpu.py holds the HIP calls against these specs."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from hgs import _lib, hierarchy
from hgs import trim_to_views as cmd
from oracle import lod_oracle as lo
from test_hier_trim_cpu import (ROI, ROOT, VIEWS, assert_cuts_equal_after_mapping, bits, check_layout, corruptions,
                                hand_tree, oracle_cut, scene2000, _view)

F = np.float32
FLT_MAX = F(3.4028234663852886e38)
INF = float("inf")
TAU = 0.2
KS = (1, 3, 100, 1001, 3998, 3999, 10 ** 9)
GOLDEN = os.path.join(ROOT, "tests", "golden")


@functools.lru_cache(maxsize=None)
def view_sets():
    """The three view sets of the documented sizes: the outside views of the trim tests, a 65-point street-level path,
    one region around that path."""
    return dict(views=hierarchy.view_regions(points=VIEWS),
                path=hierarchy.view_regions(points=[(float(x), 2.0, -8.0) for x in np.linspace(-30.0, 30.0, 65)]),
                box=hierarchy.view_regions(boxes=[(-30.0, 0.0, -10.0, 30.0, 4.0, -6.0)]))


DOCUMENTED = dict(views=(2631, 491), path=(2285, 519), box=(2523, 502))      # kept nodes, stubs at tau = 0.2


@functools.lru_cache(maxsize=None)
def trimmed(name):
    return hierarchy.trim_to_views(scene2000()[0], view_sets()[name], TAU)


@functools.lru_cache(maxsize=None)
def seeded_regions():
    """200 regions around and inside the scene, the first 100 of them points."""
    rng = np.random.default_rng(20)
    c = rng.uniform((-60.0, -50.0, -40.0), (60.0, 50.0, 70.0), size=(200, 3))
    half = rng.uniform(0.0, 6.0, size=(200, 3))
    half[:100] = 0.0
    half[100:110, 1:] = 0.0                                    # ten segments: flat on two axes
    lo_, hi_ = hierarchy.view_regions(boxes=np.concatenate([c - half, c + half], axis=1))
    assert np.array_equal(lo_[:100], hi_[:100]) and (lo_[110:] < hi_[110:]).all()
    return lo_, hi_


def terms(boxes, lo_, hi_):
    """ext / sqrt(d2(p, c)) or FLT_MAX, float32 [N, C]: the per-region term of the reach."""
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = hierarchy._reach_d2(boxes, lo_, hi_)
        return np.where(d2 > 0, boxes[:, None, 0, 3] / np.sqrt(d2), FLT_MAX).astype(F)


# ---- the four properties ---------------------------------------------------------------------------------------------
def test_property_1_a_point_region_gives_node_size():
    h, _ = scene2000()
    bx = h.boxes.numpy()
    lo_, hi_ = seeded_regions()
    t = terms(bx, lo_[:100], hi_[:100])
    ids = np.arange(bx.shape[0])
    for c in range(100):
        assert np.array_equal(t[:, c].view(np.uint32), lo.node_size(bx, ids, lo_[c]).view(np.uint32)), c
    inside = hierarchy.view_regions(points=[(0.0, 0.0, 10.0)])
    r = hierarchy.view_reach(h, inside)
    assert np.array_equal(r.view(np.uint32), lo.node_size(bx, ids, (0.0, 0.0, 10.0)).view(np.uint32))
    assert r[0] == FLT_MAX and (r == FLT_MAX).sum() > 5


def test_property_2_reach_is_the_maximum_of_the_terms():
    h, _ = scene2000()
    lo_, hi_ = seeded_regions()
    r = hierarchy.view_reach(h, (lo_, hi_))
    assert r.dtype == np.float32 and r.shape == (3999,)
    assert np.array_equal(r.view(np.uint32), terms(h.boxes.numpy(), lo_, hi_).max(1).view(np.uint32))
    assert (r == FLT_MAX).any() and (r < FLT_MAX).any()
    # the chunking of the spec does not show: one region at a time gives the same bits
    one = np.stack([hierarchy.view_reach(h, (lo_[c:c + 1], hi_[c:c + 1])) for c in range(0, 200, 7)])
    sub = hierarchy.view_reach(h, (lo_[::7], hi_[::7]))
    assert np.array_equal(one.max(0).view(np.uint32), sub.view(np.uint32))


def test_property_3_no_viewpoint_inside_a_region_sees_a_node_larger():
    h, _ = scene2000()
    bx = h.boxes.numpy()
    lo_, hi_ = seeded_regions()
    t = terms(bx, lo_, hi_)
    rng = np.random.default_rng(21)
    ids = np.arange(bx.shape[0])
    for c in range(100, 200):
        corners = np.array([[(lo_[c], hi_[c])[(k >> a) & 1][a] for a in range(3)] for k in range(8)], dtype=F)
        inner = np.clip((lo_[c] + rng.uniform(size=(4, 3)) * (hi_[c] - lo_[c])).astype(F), lo_[c], hi_[c])
        for v in np.concatenate([corners, inner]):
            assert (lo.node_size(bx, ids, v) <= t[:, c]).all(), (c, v)
    # ... and the bound is attained at a corner for a node outside the region's slab on every axis
    assert any((lo.node_size(bx, ids, lo_[c]) == t[:, c]).any() for c in range(110, 200))


def test_property_4_a_parents_reach_is_at_least_its_childs():
    h, _ = scene2000()
    nd, bx = h.nodes.numpy(), h.boxes.numpy()
    par = nd[1:, 1]
    assert (bx[1:, 0, :3] >= bx[par, 0, :3]).all() and (bx[1:, 1, :3] <= bx[par, 1, :3]).all()      # the boxes nest
    assert (bx[1:, 0, 3] <= bx[par, 0, 3]).all()                                                    # extents do not grow
    for regions in (seeded_regions(),) + tuple(view_sets().values()):
        r = hierarchy.view_reach(h, regions)
        assert (r[par] >= r[1:]).all()


# ---- regions -----------------------------------------------------------------------------------------------------------
def test_view_regions():
    lo_, hi_ = hierarchy.view_regions(points=[(1.0, 2.0, 3.0), (0.1, 0.2, 0.3)], pad=0.5)
    assert lo_.dtype == hi_.dtype == np.float32 and lo_.shape == hi_.shape == (2, 3)
    assert lo_[0].tolist() == [0.5, 1.5, 2.5] and hi_[0].tolist() == [1.5, 2.5, 3.5]
    assert lo_[1, 0] == F(0.1 - 0.5) and hi_[1, 2] == F(0.3 + 0.5)                   # one rounding, of the padded number
    lo_, hi_ = hierarchy.view_regions(points=torch.tensor([[1.0, 2.0, 3.0]]), boxes=[[(0, 0, 0), (1, 1, 1)], [(2, 2, 2), (2, 2, 5)]])
    assert lo_.tolist() == [[1, 2, 3], [0, 0, 0], [2, 2, 2]] and hi_.tolist() == [[1, 2, 3], [1, 1, 1], [2, 2, 5]]
    for kw, word in ((dict(), "empty"), (dict(points=[]), "empty"), (dict(points=[(0, 0, 0), (0, float("nan"), 0)]), "view point 1"),
                     (dict(points=[(0, 0, 0)], boxes=[(0, 0, 0, 1, 1, 1), (0, 0, 0, INF, 1, 1)]), "view box 1"),
                     (dict(boxes=[(0, 0, 2, 1, 1, 1)]), "view box 0: lo > hi"), (dict(points=[(0, 0, 0)], pad=-1.0), "pad"),
                     (dict(points=[(0, 0, 0)], pad=float("nan")), "pad"), (dict(points=[(1e39, 0, 0)]), "view point 0")):
        with pytest.raises(ValueError, match=word):
            hierarchy.view_regions(**kw)
    h, _ = scene2000()
    for bad in ((np.zeros((0, 3)), np.zeros((0, 3))), (np.zeros((2, 3)), np.zeros((3, 3))), (np.ones((1, 3)), np.zeros((1, 3)))):
        with pytest.raises(ValueError):
            hierarchy.view_reach(h, bad)
    with pytest.raises(ValueError, match="NaN"):
        hierarchy.trim_to_views(h, view_sets()["views"], float("nan"))


# ---- a tree that can be read by eye --------------------------------------------------------------------------------------
def test_hand_built_tree_under_two_point_views():
    """hand_tree(): root [0,8]^3 (extent 8), node 1 [0,2]^3 (2), node 2 [4,8]^3 (4), unit leaves 3 [0,1]^3, 4 [1,2]^3,
    5 [4,5]^3, 6 [7,8]^3.  View A = (-8, 1, 1) is 8 away from the root, node 1 and leaf 3 along x; view B = (16, 6, 6)
    is 8 away from the root and node 2."""
    h = hand_tree()
    regions = hierarchy.view_regions(points=[(-8.0, 1.0, 1.0), (16.0, 6.0, 6.0)])
    r = hierarchy.view_reach(h, regions)
    s = lambda e, d2: F(e) / np.sqrt(F(d2))
    want = [1.0, 0.25, 0.5, 0.125, max(s(1, 81), s(1, 196 + 16 + 16)), max(s(1, 144 + 9 + 9), s(1, 121 + 1 + 1)),
            max(s(1, 225 + 36 + 36), s(1, 64 + 1 + 1))]
    assert r.tolist() == [float(F(x)) for x in want]
    t = hierarchy.trim_to_views(h, regions, 0.3)
    # test: the root (1.0) and node 2 (0.5) pass, node 1 (0.25) does not: its children go, it becomes a stub
    assert t.old_of_new.tolist() == [0, 1, 2, 5, 6] and t.new_of_old.tolist() == [0, 1, 2, -1, -1, 3, 4]
    assert t.hierarchy.nodes.tolist() == [[0, -1, 0, 0, 1, 1, 2], [1, 0, 1, 1, 0, 0, 0], [1, 0, 2, 0, 1, 3, 2],
                                          [2, 2, 3, 1, 0, 0, 0], [2, 2, 4, 1, 0, 0, 0]]
    assert t.stubs == 1 and t.stub_ids.tolist() == [1] and t.tau == float(F(0.3)) and t.min_extent == 0.0
    for k in ("xyz", "shs", "alpha", "log_scales", "rots", "boxes"):
        assert torch.equal(bits(getattr(t.hierarchy, k)), bits(getattr(h, k)[torch.tensor([0, 1, 2, 5, 6])])), k
    # the test is closed: 0.25 keeps node 1's children, the next float above does not
    assert hierarchy.trim_to_views(h, regions, 0.25).hierarchy.num_nodes == 7
    assert hierarchy.trim_to_views(h, regions, float(np.nextafter(F(0.25), F(1)))).hierarchy.num_nodes == 5
    assert hierarchy.trim_to_views(h, regions, 0.6).old_of_new.tolist() == [0, 1, 2]
    assert hierarchy.trim_to_views(h, regions, 1.5).old_of_new.tolist() == [0]
    # view A alone: node 2 is 0.314 from it; the extent floor and the region are further conjuncts
    a = hierarchy.view_regions(points=[(-8.0, 1.0, 1.0)])
    assert hierarchy.trim_to_views(h, a, 0.3).old_of_new.tolist() == [0, 1, 2, 5, 6]
    assert hierarchy.trim_to_views(h, a, 0.32).old_of_new.tolist() == [0, 1, 2]
    assert hierarchy.trim_to_views(h, regions, 0.2, min_extent=3.0).old_of_new.tolist() == [0, 1, 2, 5, 6]
    assert hierarchy.trim_to_views(h, regions, 0.2, roi=((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))).old_of_new.tolist() == [0, 1, 2, 3, 4]
    # covers: inside a region (here: at the point) and tau at least the one used
    assert t.covers((-8.0, 1.0, 1.0), 0.3) and t.covers(torch.tensor([16.0, 6.0, 6.0]), 1.0)
    assert not t.covers((-8.0, 1.0, 1.0), 0.29) and not t.covers((-8.0, 1.0, 1.5), 0.3)


def test_equal_reaches_go_in_together_or_not_at_all():
    h = hand_tree()
    everywhere = hierarchy.view_regions(boxes=[(-1.0, -1.0, -1.0, 9.0, 9.0, 9.0)])
    assert (hierarchy.view_reach(h, everywhere) == FLT_MAX).all()
    for K, n, tau in ((1, 1, INF), (3, 1, INF), (6, 1, INF), (7, 7, float(FLT_MAX)), (100, 7, float(FLT_MAX))):
        t = hierarchy.trim_to_views(h, everywhere, 0.0, max_nodes=K)
        assert (t.hierarchy.num_nodes, t.tau) == (n, tau), K
    t = hierarchy.trim_to_views(h, everywhere, 0.0, max_nodes=6)
    assert t.hierarchy.nodes.tolist() == [[0, -1, 0, 1, 0, 0, 0]] and t.stubs == 1
    # two views: the candidates' reaches are 1.0, 0.5, 0.25: 3, 5, 7 nodes
    two = hierarchy.view_regions(points=[(-8.0, 1.0, 1.0), (16.0, 6.0, 6.0)])
    for K, n, tau in ((2, 1, INF), (3, 3, 1.0), (4, 3, 1.0), (5, 5, 0.5), (6, 5, 0.5), (7, 7, 0.25)):
        t = hierarchy.trim_to_views(h, two, 0.0, max_nodes=K)
        assert (t.hierarchy.num_nodes, t.tau) == (n, tau), K
    # the larger of the given tau and the budget's is used
    assert hierarchy.trim_to_views(h, two, 0.6, max_nodes=7).hierarchy.num_nodes == 3
    assert hierarchy.trim_to_views(h, two, 0.1, max_nodes=5).tau == 0.5


# ---- the 2 000-leaf scene ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DOCUMENTED))
def test_the_scene_trims_to_the_documented_sizes(name):
    h, _ = scene2000()
    t = trimmed(name)
    assert (h.num_nodes, t.hierarchy.num_nodes, t.stubs, t.stub_ids.numel()) == (3999,) + DOCUMENTED[name] + (DOCUMENTED[name][1],)
    assert t.tau == float(F(TAU)) and t.min_extent == 0.0
    assert np.array_equal(t.regions[0], view_sets()[name][0]) and np.array_equal(t.regions[1], view_sets()[name][1])
    check_layout(t.hierarchy.nodes.numpy())
    # kept iff the parent's reach is at least tau
    r = hierarchy.view_reach(h, view_sets()[name])
    assert np.array_equal((t.new_of_old.numpy() >= 0)[1:], r[h.nodes[1:, 1].numpy()] >= F(TAU))


def contract_viewpoints(name):
    """Float32 viewpoints inside the regions of a view set: every corner of a few regions, and points drawn inside."""
    lo_, hi_ = view_sets()[name]
    rng = np.random.default_rng(22)
    out = []
    for c in sorted({0, lo_.shape[0] // 2, lo_.shape[0] - 1}):
        corners = {tuple((lo_[c], hi_[c])[(k >> a) & 1][a] for a in range(3)) for k in range(8)}
        out += [np.array(v, dtype=F) for v in sorted(corners)]
        if len(corners) > 1:
            out += list(np.clip((lo_[c] + rng.uniform(size=(3, 3)) * (hi_[c] - lo_[c])).astype(F), lo_[c], hi_[c]))
    return out


@pytest.mark.parametrize("name", list(DOCUMENTED))
def test_the_contract_against_the_oracle_cut(name):
    h, _ = scene2000()
    t = trimmed(name)
    m = t.new_of_old.numpy()
    views = contract_viewpoints(name)
    assert len(views) == {"views": 3, "path": 3, "box": 11}[name]
    stubs_met, below = 0, []
    for v in views:
        for tau in (F(TAU), F(2 * TAU)):
            assert t.covers(v, tau) and t.exact_for(v, tau) is True
            a, b = oracle_cut(h, tau, v), oracle_cut(t.hierarchy, tau, v)
            assert_cuts_equal_after_mapping(a, b, m)
            stubs_met += int(np.isin(b[2], t.stub_ids.numpy()).sum())
        below.append(t.exact_for(v, F(TAU) / F(4)))
        assert not t.covers(v, F(TAU) / F(4))
    assert stubs_met > 0                                  # the cuts do end at stubs: the equality is not vacuous
    assert not all(below)                                 # below tau nothing is promised, and somewhere it fails
    far = (200.0, 2.0, -8.0)
    assert not t.covers(far, TAU)


def test_identity_and_root_only():
    h, _ = scene2000()
    whole = hierarchy.view_regions(boxes=[(-100.0, -100.0, -100.0, 100.0, 100.0, 100.0)])
    for kw in (dict(regions=whole, tau=0.0), dict(regions=whole, tau=1e30), dict(regions=view_sets()["path"], tau=0.0),
               dict(regions=view_sets()["path"], tau=-1.0, max_nodes=3999)):
        t = hierarchy.trim_to_views(h, **kw)
        for k in ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes"):
            assert torch.equal(bits(getattr(t.hierarchy, k)), bits(getattr(h, k))), (kw, k)
        assert torch.equal(t.old_of_new, torch.arange(3999, dtype=torch.int32)) and t.stubs == 0
    for kw in (dict(tau=INF), dict(tau=0.0, max_nodes=1), dict(tau=0.0, min_extent=INF)):
        t = hierarchy.trim_to_views(h, view_sets()["path"], **kw)
        assert t.hierarchy.nodes.tolist() == [[0, -1, 0, 1, 0, 0, 0]] and t.stubs == 1
    assert hierarchy.trim_to_views(h, whole, INF).hierarchy.num_nodes == 1            # FLT_MAX < inf


def test_budget():
    h, _ = scene2000()
    nd = h.nodes.numpy()
    regions = view_sets()["path"]
    reach = hierarchy.view_reach(h, regions)
    values = np.unique(reach[nd[:, 6] > 0])
    sizes = {}
    for K in KS:
        t = hierarchy.trim_to_views(h, regions, 0.0, max_nodes=K)
        sizes[K] = t.hierarchy.num_nodes
        assert t.hierarchy.num_nodes <= K
        if t.tau == INF:
            assert t.hierarchy.num_nodes == 1 and hierarchy.trim_to_views(h, regions, float(values[-1])).hierarchy.num_nodes > K
            continue
        at = int(np.searchsorted(values, F(t.tau)))
        assert values[at] == F(t.tau)
        if at > 0:                                       # the next smaller distinct reach no longer fits
            assert hierarchy.trim_to_views(h, regions, float(values[at - 1])).hierarchy.num_nodes > K
        check_layout(t.hierarchy.nodes.numpy())
    assert sizes[1] == 1 and sizes[1001] == 1001 and sizes[3999] == sizes[10 ** 9] == 3999
    # a camera inside the root box: every node around it has the key FLT_MAX; they go in together or not at all
    inside = hierarchy.view_regions(points=[(0.0, 0.0, 10.0)])
    r = hierarchy.view_reach(h, inside)
    run = 1 + int(nd[(r == FLT_MAX) & (nd[:, 6] > 0), 6].sum())
    assert run > 5
    t = hierarchy.trim_to_views(h, inside, 0.0, max_nodes=run - 1)
    assert t.hierarchy.num_nodes == 1 and t.tau == INF
    t = hierarchy.trim_to_views(h, inside, 0.0, max_nodes=run)
    assert t.hierarchy.num_nodes == run and t.tau == float(FLT_MAX)
    # with a floor and a region
    _, med = scene2000()
    for K in (100, 1001):
        t = hierarchy.trim_to_views(h, regions, 0.05, min_extent=med / 2, roi=ROI, max_nodes=K)
        assert 1 < t.hierarchy.num_nodes <= K and t.tau >= float(F(0.05))
        check_layout(t.hierarchy.nodes.numpy())
        assert t.hierarchy.num_nodes <= hierarchy.trim_hierarchy(h, med / 2, ROI).hierarchy.num_nodes
    assert float(hierarchy.view_budget_tau(nd, h.boxes.numpy(), reach, 1001)) == hierarchy.trim_to_views(h, regions, 0.0, max_nodes=1001).tau
    with pytest.raises(ValueError):
        hierarchy.trim_to_views(h, regions, 0.0, max_nodes=0)


def test_boxes_that_do_not_nest_are_refused():
    """The closure case of the trim tests: node p's extent is a quarter of the floor while a child's is at least the
    floor.  From far away every distance is about the same, so p fails the reach test and that child passes it."""
    name, c, floor, check, _ = corruptions()[0]
    assert name == "closure" and check == 3
    regions = hierarchy.view_regions(points=[(0.0, 0.0, -500.0)])
    tau = floor / 550.0
    nd = c.nodes.numpy()
    test = hierarchy.view_reach(c, regions) >= F(tau)
    par = nd[:, 1]
    node = next(n for n in range(1, 3999) if par[n] > 0 and test[par[n]] and not test[par[par[n]]])
    with pytest.raises(hierarchy.HierarchyTrimError) as e:
        hierarchy.trim_to_views(c, regions, tau)
    assert e.value.check == hierarchy.TRIM_CHECKS[3] and e.value.node == node
    assert f"node {node}" in str(e.value) and "hgs.refit_hierarchy" in str(e.value)
    # the layout checks come first, as under trim_hierarchy
    for name, c, floor, check, node in corruptions()[1:]:
        with pytest.raises(hierarchy.HierarchyTrimError) as e:
            hierarchy.trim_to_views(c, regions, tau)
        assert e.value.check == hierarchy.TRIM_CHECKS[check] and e.value.node == node, name


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
HEADER = open(os.path.join(ROOT, "include", "hgs.h")).read()
NEW = ("hgs_hier_reach_tmp_bytes", "hgs_hier_reach", "hgs_hier_trim_plan_keyed")


def test_the_abi_declares_binds_and_exports_the_three_entries():
    import subprocess
    plain = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, plain), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        assert re.search(r"\b%s\b" % name, nm), name
    assert re.search(r"#define\s+HGS_ABI_VERSION\s+14\b", HEADER) and _lib.ABI_VERSION == 14
    assert C.sizeof(_lib.HierTrimArgs) == 32 and C.sizeof(_lib.HierTrimReport) == 32
    src = open(os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc", "hier_reach.hip")).read()
    assert int(re.search(r"kReachSlab\s*=\s*(\d+)", src).group(1)) == hierarchy.REACH_SLAB
    assert hierarchy.REACH_MAX_REGIONS == 1 << 24


def test_reach_tmp_bytes_needs_no_gpu():
    f = _lib.lib().hgs_hier_reach_tmp_bytes
    for N, C_ in ((0, 1), (-1, 1), (1 << 31, 1), (1 << 40, 1), (-(1 << 40), 1), (1, 0), (1, -1), (1, (1 << 24) + 1),
                  (1, 1 << 40), (0, 0)):
        assert f(N, C_) == 0, (N, C_)
    for N in (1, 256, 257, 2_097_153, (1 << 31) - 1):
        for C_ in (1, 20_000, 1 << 24):
            b = f(N, C_)
            assert b >= 4 * N and b % 256 == 0, (N, C_, b)               # D2's bit pattern per node
    assert f(1, 1) <= f(257, 1) < f(2_097_153, 1) < f((1 << 31) - 1, 1)


def test_bad_arguments_fail_before_any_hip_call():
    """(No GPU here: a call that got as far as HIP would return HGS_ERR_HIP, not HGS_ERR_INVALID.)"""
    lib = _lib.lib()
    a = 4096
    reach = [((a, 0, a, 1, a, a), b"bad sizes"), ((a, 1 << 31, a, 1, a, a), b"bad sizes"), ((a, 5, a, 0, a, a), b"bad sizes"),
             ((a, 5, a, (1 << 24) + 1, a, a), b"bad sizes"), ((a, 5, a, -3, a, a), b"bad sizes"),
             ((None, 5, a, 1, a, a), b"null"), ((a, 5, None, 1, a, a), b"null"), ((a, 5, a, 1, None, a), b"null"),
             ((a, 5, a, 1, a, None), b"null"), ((a + 8, 5, a, 1, a, a), b"16-byte"), ((a, 5, a + 2, 1, a, a), b"4-byte"),
             ((a, 5, a, 1, a + 1, a), b"4-byte"), ((a, 5, a, 1, a, a + 64), b"256-byte")]
    for (boxes, N, regions, C_, out, tmp), word in reach:
        assert lib.hgs_hier_reach(boxes, N, regions, C_, out, tmp, None, 0) == 1, word
        assert word in lib.hgs_last_error(), (word, lib.hgs_last_error())
    rep, args = _lib.HierTrimReport(), _lib.HierTrimArgs(1.0, 0)
    nan = _lib.HierTrimArgs(float("nan"), 0)
    nan_roi = _lib.HierTrimArgs(0.0, 1)
    nan_roi.roi_lo[2] = float("nan")
    keyed = [((_view(0), args, a, 0.5, a, rep), b"bad sizes"), ((_view(1 << 31), args, a, 0.5, a, rep), b"bad sizes"),
             ((_view(5, G=4), args, a, 0.5, a, rep), b"bad sizes"), ((_view(5, M=65), args, a, 0.5, a, rep), b"bad sizes"),
             ((_view(5, nodes=0), args, a, 0.5, a, rep), b"null"), ((_view(5), args, None, 0.5, a, rep), b"null"),
             ((_view(5), args, a, 0.5, None, rep), b"null"), ((_view(5, boxes=a + 4), args, a, 0.5, a, rep), b"16-byte"),
             ((_view(5), args, a + 2, 0.5, a, rep), b"4-byte"), ((_view(5), nan, a, 0.5, a, rep), b"NaN"),
             ((_view(5), nan_roi, a, 0.5, a, rep), b"NaN"), ((_view(5), args, a, float("nan"), a, rep), b"NaN"),
             ((_view(5), args, a, 0.5, a + 64, rep), b"256-byte")]
    for (v, ar, key, floor, tmp, rp), word in keyed:
        assert lib.hgs_hier_trim_plan_keyed(C.byref(v), C.byref(ar), key, floor, tmp, C.byref(rp), None, 0) == 1, word
        assert word in lib.hgs_last_error(), (word, lib.hgs_last_error())
    assert lib.hgs_hier_trim_plan_keyed(None, C.byref(args), a, 0.5, a, C.byref(rep), None, 0) == 1
    assert lib.hgs_hier_trim_plan_keyed(C.byref(_view(5)), C.byref(args), a, 0.5, a, None, None, 0) == 1
    # a refused keyed plan registers nothing: apply still has no plan on this tmp
    v = _view(5)
    assert lib.hgs_hier_trim_apply(C.byref(v), C.byref(_view(3)), a, a, a, None, 0) == 1
    assert b"no successful hgs_hier_trim_plan" in lib.hgs_last_error()


# ---- the command ---------------------------------------------------------------------------------------------------------
def test_the_command_parses_its_arguments(capsys):
    p = cmd.parse_args
    got = p(["a.hier", "b.hier", "--view", "0", "1", "-2", "--tau", "0.2"])
    assert got == dict(in_path="a.hier", out_path="b.hier", cameras=None, views=[(0.0, 1.0, -2.0)], view_boxes=[], pad=0.0,
                       tau=0.2, min_extent=0.0, max_nodes=None, roi=None)
    got = p(["--cameras", "c.json", "--pad", "1.5", "a.hier", "--tau-px", "3", "--tanfovx", "0.5", "--width", "1000",
             "b.hier", "--max-nodes", "1001", "--min-extent", "0.01", "--roi", "-2", "-2", "5", "2", "2", "12"])
    assert got["cameras"] == "c.json" and got["pad"] == 1.5 and got["max_nodes"] == 1001 and got["min_extent"] == 0.01
    assert got["roi"] == ((-2.0, -2.0, 5.0), (2.0, 2.0, 12.0))
    assert got["tau"] == (2 * (3 + 0.5)) * 0.5 / (0.5 * 1000) == cmd.tau_from_pixels(3.0, 0.5, 1000.0)
    got = p(["a.hier", "b.hier", "--view", "0", "0", "0", "--view", "1", "1", "1", "--view-box", "0", "0", "0", "1", "2", "3",
             "--tau", "0"])
    assert got["views"] == [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)] and got["view_boxes"] == [(0.0, 0.0, 0.0, 1.0, 2.0, 3.0)]
    ok = ["a.hier", "b.hier", "--view", "0", "0", "0"]
    bad = ([], ["a.hier"], ["a.hier", "b.hier"], ["a.hier", "b.hier", "--tau", "0.2"], ok, ok + ["--tau"],
           ok + ["--tau", "x"], ok + ["--tau", "nan"], ok + ["--tau", "0.2", "--tau", "0.3"],
           ok + ["--tau", "0.2", "--tau-px", "3", "--tanfovx", "0.5", "--width", "1000"],
           ok + ["--tau-px", "3"], ok + ["--tau-px", "3", "--tanfovx", "0.5"], ok + ["--tau-px", "3", "--tanfovx", "0.5", "--width", "0"],
           ok + ["--tau", "0.2", "--pad", "-1"], ok + ["--tau", "0.2", "--max-nodes", "0"], ok + ["--tau", "0.2", "--max-nodes", "1.5"],
           ok + ["--tau", "0.2", "--frobnicate"], ok + ["--tau", "0.2", "c.hier"], ok + ["--tau", "0.2", "--min-extent", "nan"],
           ["a.hier", "b.hier", "--view", "0", "0", "--tau", "0.2"], ["a.hier", "b.hier", "--view-box", "0", "0", "0", "1", "1", "--tau", "0.2"],
           ok + ["--tau", "0.2", "--roi", "0", "0", "0", "1", "1"], ["a.hier", "b.hier", "--view", "0", "nan", "0", "--tau", "0.2"])
    for argv in bad:
        assert p(argv) is None, argv
        assert cmd.main(argv) == 2, argv
    assert "usage: python -m hgs.trim_to_views" in capsys.readouterr().err
    assert cmd.main(["/nonexistent/in.hier", "out.hier", "--view", "0", "0", "0", "--tau", "1"]) == 2
    assert "does not exist" in capsys.readouterr().err
    # the other command's parser is its own: it knows nothing of views
    from hgs import trim_hierarchy
    assert trim_hierarchy.parse_args(["a.hier", "b.hier", "--view", "0", "0", "0", "--min-extent", "1"]) is None


def test_the_cameras_json_reader(tmp_path, capsys):
    path = os.path.join(GOLDEN, "cameras_two.json")
    assert cmd.read_camera_positions(path) == [[-12.5, 2.0, -8.0], [30.0, 2.0, 10.0]]
    lo_, hi_ = cmd.regions_of(path, views=[(0.0, 0.0, -5.0)], view_boxes=[(0.0, 0.0, 0.0, 1.0, 1.0, 1.0)], pad=0.5)
    assert lo_.tolist() == [[-13.0, 1.5, -8.5], [29.5, 1.5, 9.5], [-0.5, -0.5, -5.5], [0.0, 0.0, 0.0]]
    assert hi_.tolist() == [[-12.0, 2.5, -7.5], [30.5, 2.5, 10.5], [0.5, 0.5, -4.5], [1.0, 1.0, 1.0]]
    for k, text in enumerate(('[]', '{"position": [0, 0, 0]}', '[{"id": 0}]', '[{"position": [0, 0]}]',
                              '[{"position": [0, 0, 0]}, {"position": [0, "x", 0]}]', 'not json')):
        f = tmp_path / f"bad{k}.json"
        f.write_text(text)
        with pytest.raises(ValueError):
            cmd.read_camera_positions(str(f))
    f = tmp_path / "one.json"
    f.write_text('[{"position": [0, 0, 0]}, {"position": [0, 1e39, 0]}]')
    src = tmp_path / "in.hier"
    src.write_bytes(b"")
    assert cmd.main([str(src), str(tmp_path / "out.hier"), "--cameras", str(f), "--tau", "1"]) == 2
    assert "view point 1" in capsys.readouterr().err and not (tmp_path / "out.hier").exists()
    assert cmd.main([str(src), str(tmp_path / "out.hier"), "--cameras", str(tmp_path / "none.json"), "--tau", "1"]) == 2
    assert "does not exist" in capsys.readouterr().err
