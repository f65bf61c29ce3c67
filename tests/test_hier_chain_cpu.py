"""The hierarchy tools applied to each other's outputs, with the numpy specs alone (no GPU): every ordered pair of the
eight tools of tests/hier_chain_cases.py on its four bases gives a hierarchy that passes the layout checks, nests and
has a non-empty cut; the derived hierarchies have the structure that justifies them (single-child nodes after a prune,
stubs after a trim, k = 3 below the root in a merge of merges, ``kids == 1`` entries in the cuts, culled and unculled
entries under a frustum); and a deliberately wrong cut -- every node with children taken to have exactly two -- agrees
with the oracle on what the builder makes and differs on every pruned case and on the merge of merges.
tests/test_hier_chain_gpu.py runs the device code on these cases."""
import numpy as np
import pytest
import torch

import budget_cut_cases as bc
import frustum_cases as fc
import frustum_spec as fs
import hier_chain_cases as cc
from hgs import hierarchy
from test_hier_refit_cpu import nested_np
from test_hier_trim_cpu import check_layout

CAMERA, TAU_PX = "B", 3.0          # the culled cut of the CPU tests: from inside the scenes, looking down +z


def culled_cut(h, cam_name=CAMERA, tau_px=TAU_PX):
    """frustum_spec.cut_view_spec of a host hierarchy with the spec's own bounds."""
    cam, planes, rs = bc.planes_of(cam_name)
    nd = h.nodes.numpy()
    bounds = fs.bounds_spec(nd, h.xyz.numpy(), torch.exp(h.log_scales).numpy())
    return fs.cut_view_spec(nd, h.boxes.numpy().reshape(-1, 2, 4), bounds, fc.tau_of(cam, tau_px), cam.camera_center.numpy(),
                            planes, rs)


# ---- every ordered pair ------------------------------------------------------------------------------------------------
def expected_refusal(base_name, a, b):
    """Removing everything under node 1 twice takes both children of a two-child root: the spec refuses the second call
    ("every leaf would be removed").  Under the merged base's root of three the same pair goes through."""
    return (a, b) == ("prune_under1", "prune_under1") and base_name != "merged"


@pytest.mark.parametrize("base_name", cc.BASES)
def test_every_ordered_pair_of_tools_gives_a_usable_hierarchy(base_name):
    for a, b in cc.PAIRS:
        mid = cc.after(a, base_name)
        assert not isinstance(mid, Exception), (a, mid)
        if expected_refusal(base_name, a, b):
            with pytest.raises(hierarchy.HierarchyPruneError) as e:
                cc.spec(b, cc.hier(mid))
            assert e.value.check == hierarchy.PRUNE_ROOT_DEAD and e.value.node == 0
            continue
        out = cc.hier(cc.spec(b, cc.hier(mid)))
        nd, bx = out.nodes.numpy(), out.boxes.numpy()
        check_layout(nd)
        assert nested_np(nd, bx), (a, b)
        assert out.shs.shape[1] == cc.base(base_name).shs.shape[1]
        assert len(cc.oracle_cut(out)[0]) > 0, (a, b)


def test_the_view_trim_keeps_between_a_quarter_and_three_quarters_of_every_base():
    for name in cc.BASES:
        h, r = cc.base(name), cc.after("trim_to_views", name)
        assert 0.25 * h.num_nodes < r.hierarchy.num_nodes < 0.75 * h.num_nodes, (name, r.hierarchy.num_nodes, h.num_nodes)
        assert r.stubs > 0


def test_the_transform_is_a_general_similarity():
    sim = cc.tool_args("transform", cc.base("built129"))[0][0]
    R = np.asarray(sim.R, dtype=np.float64)
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    axis /= np.linalg.norm(axis)
    assert np.abs(axis).max() < 0.95 and np.abs(R - np.eye(3)).max() > 0.1       # about no axis of the frame
    assert abs(float(sim.s) - 1.0) > 0.1 and np.abs(np.asarray(sim.t)).min() > 0.0


# ---- the cases are what they claim ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,base_name", cc.DERIVED)
def test_a_derived_hierarchy_has_the_structure_that_justifies_it(kind, base_name):
    h = cc.derived(kind, base_name)
    s = cc.structure(h)
    cut = cc.oracle_cut(h)
    spec = culled_cut(h)
    print(f"{kind}@{base_name}: N {h.num_nodes} {s} cut {len(cut[0])} kids==1 {int((cut[4] == 1).sum())} "
          f"culled {int(spec['culled'].sum())} of {spec['n_unculled']}")
    check_layout(h.nodes.numpy())
    assert nested_np(h.nodes.numpy(), h.boxes.numpy())
    assert h.num_nodes <= 2700
    if kind in cc.PRUNED_KINDS:
        assert s["single_child"] > 0
        # the root's own entry counts one sibling by definition: what is asked for is a node under a single-child parent
        assert int(((cut[4] == 1) & (h.nodes.numpy()[cut[2], 1] >= 0)).sum()) > 0
    if kind in ("pruned", "trimmed_pruned"):
        assert cc.derived_result(kind, base_name).single_child == s["single_child"]
    if kind == "pruned_trimmed":
        r = cc.derived_result(kind, base_name)
        assert r.stubs > 0 and s["early_leaves"] > 0
        assert (h.nodes.numpy()[r.stub_ids.numpy(), 6] == 0).all()
    if kind == "trimmed_pruned":
        assert hierarchy.trim_hierarchy(cc.base(base_name), cc.median_extent(cc.base(base_name))).stubs > 0
    if kind == "pruned_half":
        p = cc.derived("pruned", base_name)
        assert torch.equal(h.xyz, p.xyz) and torch.equal(h.nodes, p.nodes) and not torch.equal(h.shs, p.shs)
        assert torch.equal(h.shs, h.shs.half().float()) and torch.equal(h.rots, h.rots.half().float())
    if kind == "merged_of_merged":
        assert s["wide_below_root"] >= 2 and int(h.nodes[0, 6]) == 2 and h.nodes[1:3, 6].tolist() == [3, 3]
    if base_name == "merged":
        assert 0 < int(spec["culled"].sum()) < spec["n_unculled"] and spec["n"] > 0


@pytest.mark.parametrize("base_name", cc.BASES)
def test_the_bases_have_none_of_it(base_name):
    h = cc.base(base_name)
    s = cc.structure(h)
    cut = cc.oracle_cut(h)
    spec = culled_cut(h)
    print(f"{base_name}: N {h.num_nodes} {s} cut {len(cut[0])} kids==1 {int((cut[4] == 1).sum())} "
          f"culled {int(spec['culled'].sum())} of {spec['n_unculled']}")
    assert s["single_child"] == 0 and s["wide_below_root"] == 0
    assert int(((cut[4] == 1) & (h.nodes.numpy()[cut[2], 1] >= 0)).sum()) == 0


# ---- the cases discriminate ------------------------------------------------------------------------------------------------
TAUS = (0.0, cc.CUT_TAU, 0.1)


@pytest.mark.parametrize("kind,base_name", cc.DERIVED)
def test_a_cut_that_assumes_two_children_differs_on_every_derived_hierarchy(kind, base_name):
    h = cc.derived(kind, base_name)
    for tau in TAUS[:2]:
        assert not cc.same_cut(cc.oracle_cut(h, tau), cc.two_children_cut(h, tau)), (kind, base_name, tau)


@pytest.mark.parametrize("base_name", ("built129", "built257"))
def test_the_same_wrong_cut_passes_on_what_the_builder_makes(base_name):
    """... which is why no test on builder output can catch it."""
    h = cc.base(base_name)
    for tau in TAUS:
        assert cc.same_cut(cc.oracle_cut(h, tau), cc.two_children_cut(h, tau)), (base_name, tau)
    m = cc.base("merged")                      # one node of three children, the root: its third chunk is lost
    assert not cc.same_cut(cc.oracle_cut(m, 0.0), cc.two_children_cut(m, 0.0))


@pytest.mark.parametrize("base_name", cc.BASES)
def test_an_only_child_is_never_blended_with_its_parent(base_name):
    """A pruned node's box is the union of its surviving children's, so an only child has its parent's box, the two
    sizes are equal from every viewpoint and the child's interpolation weight is exactly 1: the k = 1 opacity remap
    meets a fractional weight only where a test forces one (tests/test_hier_chain_gpu.py does)."""
    h = cc.derived("pruned", base_name)
    nd, bx = h.nodes.numpy(), h.boxes.numpy()
    one = np.nonzero(nd[:, 6] == 1)[0]
    assert np.array_equal(bx[one, :, :3], bx[nd[one, 5], :, :3]) and np.array_equal(bx[one, 0, 3], bx[nd[one, 5], 0, 3])
    seen = 0
    for tau in (0.02, 0.1, 0.3, 1.0):
        for v in (cc.CUT_VIEW, (30.0, 2.0, 10.0), (0.0, 0.0, 0.0)):
            _, _, ni, w, kids = cc.oracle_cut(h, tau, v)
            only = (kids == 1) & (nd[ni, 1] >= 0)
            seen += int(only.sum())
            assert (w[only] == 1.0).all(), (tau, v)
    assert seen > 0
