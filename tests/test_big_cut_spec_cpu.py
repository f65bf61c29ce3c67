"""tests/big_cut_spec.py is the looped oracle: ``nested_cut_spec`` against ``frustum_spec.cut_view_spec`` (which walks
the tree and appends every entry in Python), every array equal and the weights equal as bit patterns, on the builder
hierarchies of the GPU cut tests and on the hand-built one with several rows per node."""
import functools

import numpy as np
import pytest
import torch

import big_cut_spec as bg
import budget_cut_cases as bc
import budget_cut_spec as bs
import frustum_cases as fc
import frustum_spec as fs
from hgs import hierarchy, synth

LEAVES = (1, 2, 3, 33, 128, 129, 1000, 20000)       # as tests/test_frustum_gpu.py
ALL_INSIDE = np.array([[0.0, 0.0, 1.0, 1e30]] * 5, dtype=np.float32)
TAUS_PX = fc.TAUS_PX + (-0.5, 1e6)                   # -0.5 px: tau = 0, every leaf; 10^6 px: what the camera is inside of
ARRAYS = ("render_indices", "parent_indices", "node_indices", "kids", "culled")


@functools.lru_cache(maxsize=None)
def _built(P):
    """(nodes, boxes, bounds) on the host: the hierarchies of tests/test_frustum_gpu.py."""
    if P == 20000:
        h, _, bounds = fc.hier20k()
        return h.nodes.numpy(), h.boxes.numpy(), bounds
    h = hierarchy.build_hierarchy(synth.make_scene(P, synth.make_camera(fc.W, fc.H), seed=2))
    return h.nodes.numpy(), h.boxes.numpy(), fs.bounds_spec(h.nodes.numpy(), h.xyz.numpy(), torch.exp(h.log_scales).numpy())


def _assert_same(got, want, what):
    assert (got["n"], got["n_unculled"]) == (want["n"], want["n_unculled"]), what
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f)
    assert got["weights"].dtype == np.float32
    assert np.array_equal(got["weights"].view(np.uint32), want["weights"].view(np.uint32)), (what, "weights")


def _compare(nodes, boxes, bounds, cam, tau):
    """Both the culled and the unculled cut of one (camera, tau) -> (kept, unculled) entries."""
    vp = cam.camera_center.numpy()
    planes, rs = fs.planes_spec(cam.world_view_transform.numpy(), cam.tanfovx, cam.tanfovy, fc.W, fc.H)
    culled = bg.nested_cut_spec(bs.View(nodes, boxes, vp, bounds, planes, rs), tau)
    _assert_same(culled, fs.cut_view_spec(nodes, boxes, bounds, tau, vp, planes, rs), ("culled", float(tau)))
    plain = bg.nested_cut_spec(bs.View(nodes, boxes, vp), tau)
    _assert_same(plain, fs.cut_view_spec(nodes, boxes, bounds, tau, vp, ALL_INSIDE, 1.0), ("plain", float(tau)))
    assert plain["n"] == plain["n_unculled"] == culled["n_unculled"] and not plain["culled"].any()
    return culled["n"], culled["n_unculled"]


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("P", LEAVES)
def test_the_vectorised_cut_is_the_looped_oracle(P, name):
    nodes, boxes, bounds = _built(P)
    cam = fc.camera(name)
    counts = {px: _compare(nodes, boxes, bounds, cam, fc.tau_of(cam, px)) for px in TAUS_PX}
    print(f"P {P} camera {name}: (kept, unculled) per granularity {counts}")
    assert counts[-0.5][1] == P                                  # tau = 0: the leaves
    assert counts[1e6][1] <= counts[40.0][1] <= counts[3.0][1] <= P
    if P >= 1000:
        assert 0 < counts[3.0][0] < counts[3.0][1]               # the cull keeps some and drops some


def test_nodes_of_several_rows():
    """budget_cut_cases.multi_row(): L > 1, M > 0, a node without rows and one with children AND leaf rows -- the counts
    L and L + M, the rows start + k and the parents' first rows all differ from the one-row-per-node case."""
    nodes, boxes, bounds, _, _ = bc.multi_row()
    assert (nodes[:, 3] > 1).any() and (nodes[:, 4] > 0).any() and ((nodes[:, 3] + nodes[:, 4]) == 0).any()
    sizes = set()
    for name in "AB":
        cam = fc.camera(name)
        for px in (-0.5, 3.0, 20.0, 40.0, 80.0, 1e6):
            sizes.add(_compare(nodes, boxes, bounds, cam, fc.tau_of(cam, px)))
    print("(kept, unculled) seen:", sorted(sizes))
    assert len({u for _, u in sizes}) >= 3                       # coarse, fine and mixed cuts
    assert any(k < u for k, u in sizes) and any(k == u > 0 for k, u in sizes)


def test_a_hierarchy_that_does_not_nest_is_refused():
    nodes, boxes, _ = _built(1000)
    bad = boxes.copy()
    bad[int(nodes[-1, 1]), 0, 3] = 1e6                           # the last leaf's parent: larger than its own parent
    cam = fc.camera("A")
    view = bs.View(nodes, bad, cam.camera_center.numpy())
    assert not view.nested()
    with pytest.raises(AssertionError, match="nested_cut_spec"):
        bg.nested_cut_spec(view, fc.tau_of(cam, 3.0))
