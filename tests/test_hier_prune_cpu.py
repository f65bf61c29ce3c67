"""Leaf removal (hgs.hierarchy.prune_hierarchy, the numpy spec of csrc/hier_prune.hip) without a GPU: known answers on a
hand-built 7-node tree with equal weights, the properties of every output on built and merged hierarchies (layout,
nesting, inverse maps, clean rows bit for bit, idempotence), each criterion against a direct numpy statement with NaN
cases, the C ABI's declarations and host-only checks, the command's argument parsing and the anchors remap.
tests/test_hier_prune_gpu.py holds the HIP calls against this spec and imports the cases built here."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

from hgs import _lib, hierarchy
from hgs import prune_hierarchy as prune_cmd
from test_hier_refit_cpu import built, nested_np
from test_hier_trim_cpu import ARRAYS, HEADER, bits, check_layout, clone, merged_case

SIZES = (1, 2, 3, 128, 129, 257, 2000)
MASKS = ("none", "first_leaf", "last_leaf", "under_node_1", "every_second_leaf", "all_but_one_leaf")


def case(P):
    """The numpy builder's hierarchy over P leaves, or ("merged") three chunks under a root with k = 3."""
    return merged_case()[0] if P == "merged" else built(P)


def leaves_under(nodes, n):
    nd = np.asarray(nodes)
    todo, out = [n], []
    while todo:
        i = todo.pop()
        if nd[i, 6] == 0:
            out.append(i)
        todo.extend(range(nd[i, 5], nd[i, 5] + nd[i, 6]))
    return np.array(sorted(out), dtype=np.int64)


def removal_mask(h, kind):
    """uint8 [N] for one of MASKS (``under_node_1`` with a single node: nothing)."""
    nd = h.nodes.numpy()
    N = nd.shape[0]
    leaves = np.nonzero(nd[:, 6] == 0)[0]
    m = np.zeros(N, dtype=np.uint8)
    if kind == "first_leaf":
        m[leaves[0]] = 1
    elif kind == "last_leaf":
        m[leaves[-1]] = 1
    elif kind == "under_node_1" and N > 1:
        m[leaves_under(nd, 1)] = 1
    elif kind == "every_second_leaf":
        m[leaves[::2]] = 1
    elif kind == "all_but_one_leaf":
        m[leaves] = 1
        m[leaves[len(leaves) // 2]] = 0
    m[nd[:, 6] > 0] = 7                       # entries at nodes with children are ignored
    return m


def cov_of(log_scales, rots):
    q = np.asarray(rots, dtype=np.float64)
    R = hierarchy._rot_from_quat(q)
    return (R * np.exp(2.0 * np.asarray(log_scales, dtype=np.float64))[:, None, :]) @ R.transpose(0, 2, 1)


# ---- the hand-built tree: every node weighs alpha s0 s1 s2 = 0.5, so the moment match is checkable by hand -----------------
#        0
#    1       2
#  3   4   5   6
def hand_tree():
    nodes = torch.tensor([[0, -1, 0, 0, 1, 1, 2], [1, 0, 1, 0, 1, 3, 2], [1, 0, 2, 0, 1, 5, 2], [2, 1, 3, 1, 0, 0, 0],
                          [2, 1, 4, 1, 0, 0, 0], [2, 2, 5, 1, 0, 0, 0], [2, 2, 6, 1, 0, 0, 0]], dtype=torch.int32)
    xyz = torch.tensor([[3.5, 0, 0], [0.5, 0, 0], [6.5, 0, 0], [0, 0, 0], [1, 0, 0], [6, 0, 0], [7, 0, 0.0]])
    g = torch.Generator().manual_seed(2)
    shs = torch.randn(7, 16, 3, generator=g)
    alpha = torch.full((7, 1), 0.5)
    log_scales = torch.zeros(7, 3)
    log_scales[3:] = torch.log(torch.tensor([[1.0, 2.0, 3.0], [0.5, 1.0, 2.0], [1.0, 1.0, 2.0], [2.0, 1.0, 1.0]]))
    # equal weights: alpha * s0 * s1 * s2 = 0.5 at the leaves as at the nodes above them (alpha 0.5, unit scales)
    alpha[3:, 0] = (0.5 / torch.exp(log_scales[3:].double().sum(1))).float()
    rots = torch.tensor([[1.0, 0, 0, 0]] * 7)
    rots[4] = torch.tensor([0.5, 0.5, 0.5, 0.5])
    lo = xyz - 1.0
    hi = xyz + 1.0
    lo[1], hi[1], lo[2], hi[2] = torch.minimum(lo[3], lo[4]), torch.maximum(hi[3], hi[4]), torch.minimum(lo[5], lo[6]), torch.maximum(hi[5], hi[6])
    lo[0], hi[0] = torch.minimum(lo[1], lo[2]), torch.maximum(hi[1], hi[2])
    boxes = torch.zeros(7, 2, 4)
    boxes[:, 0, :3], boxes[:, 1, :3] = lo, hi
    boxes[:, 0, 3] = (hi - lo).max(1).values
    boxes[:, 1, 3] = torch.arange(7.0)              # the copied word
    return hierarchy.Hierarchy(xyz, shs, alpha, log_scales, rots, nodes, boxes)


def mask_of(*ids):
    m = np.zeros(7, dtype=np.uint8)
    m[list(ids)] = 1
    return m


def test_remove_one_leaf():
    h = hand_tree()
    r = hierarchy.prune_hierarchy(h, remove=mask_of(3))
    assert r.old_of_new.tolist() == [0, 1, 2, 4, 5, 6] and r.new_of_old.tolist() == [0, 1, 2, -1, 3, 4, 5]
    assert r.old_of_new.dtype == torch.int32 and r.new_of_old.dtype == torch.int32
    assert r.hierarchy.nodes.tolist() == [[0, -1, 0, 0, 1, 1, 2], [1, 0, 1, 0, 1, 3, 1], [1, 0, 2, 0, 1, 4, 2],
                                          [2, 1, 3, 1, 0, 0, 0], [2, 2, 4, 1, 0, 0, 0], [2, 2, 5, 1, 0, 0, 0]]
    assert (r.removed_leaves, r.dead, r.dirty, r.single_child) == (1, 1, 2, 1)
    o = r.hierarchy
    # node 1 has one child, the sibling 4: its mean, SH and alpha are the sibling's, its covariance too
    assert torch.equal(o.xyz[1], h.xyz[4]) and torch.equal(o.shs[1], h.shs[4]) and torch.equal(o.alpha[1], h.alpha[4])
    assert np.allclose(cov_of(o.log_scales[1:2], o.rots[1:2]), cov_of(h.log_scales[4:5], h.rots[4:5]), rtol=1e-6, atol=1e-7)
    assert o.boxes[1, :, :3].tolist() == h.boxes[4, :, :3].tolist() and float(o.boxes[1, 1, 3]) == 1.0
    assert float(o.boxes[1, 0, 3]) == 2.0
    # the root: its children are the new node 1 (one surviving leaf: weight 0.5) and the untouched node 2, which weighs
    # what its two leaves weigh, 1.0 -- the carried weight, not alpha s0 s1 s2 = 0.5 of its own row
    want = (0.5 * h.xyz[4].double() + 1.0 * h.xyz[2].double()) / 1.5
    assert np.allclose(o.xyz[0].double().numpy(), want.numpy(), rtol=1e-6)
    assert abs(float(o.alpha[0]) - (0.5 * float(h.alpha[4]) + 1.0 * 0.5) / 1.5) <= 1e-6
    assert np.allclose(o.shs[0].numpy(), ((0.5 * h.shs[4] + 1.0 * h.shs[2]) / 1.5).numpy(), atol=1e-6)
    d1, d2 = (h.xyz[4].double() - want).numpy(), (h.xyz[2].double() - want).numpy()
    c = (0.5 * (cov_of(o.log_scales[1:2], o.rots[1:2])[0] + np.outer(d1, d1)) + 1.0 * (np.eye(3) + np.outer(d2, d2))) / 1.5
    assert np.allclose(cov_of(o.log_scales[:1], o.rots[:1])[0], c, rtol=1e-5, atol=1e-6)
    # clean: node 2 and the leaves, bit for bit
    for k in ARRAYS[:5] + ("boxes",):
        assert torch.equal(bits(getattr(o, k)[2:]), bits(getattr(h, k)[[2, 4, 5, 6]])), k
    assert nested_np(o.nodes.numpy(), o.boxes.numpy())


def test_equal_weights_average_the_children():
    h = hand_tree()
    r = hierarchy.prune_hierarchy(h, remove=mask_of(), remerge="all")
    o = r.hierarchy
    assert r.dead == 0 and r.dirty == 0 and torch.equal(o.nodes, h.nodes) and torch.equal(bits(o.boxes), bits(h.boxes))
    # leaves 3 and 4 weigh 0.5 each: node 1 is their plain average
    assert np.allclose(o.xyz[1].numpy(), [0.5, 0, 0]) and np.allclose(o.shs[1].numpy(), 0.5 * (h.shs[3] + h.shs[4]).numpy(), atol=1e-6)
    c = 0.5 * (cov_of(h.log_scales[3:4], h.rots[3:4])[0] + cov_of(h.log_scales[4:5], h.rots[4:5])[0]) + np.diag([0.25, 0, 0])
    assert np.allclose(cov_of(o.log_scales[1:2], o.rots[1:2])[0], c, rtol=1e-5, atol=1e-6)
    assert abs(float(o.alpha[1]) - 0.5 * float(h.alpha[3] + h.alpha[4])) <= 1e-6
    # nodes 1 and 2 carry two leaves each, 1.0: the root is the plain average of their re-merged rows
    assert np.allclose(o.xyz[0].numpy(), 0.5 * (o.xyz[1] + o.xyz[2]).numpy(), atol=1e-6)
    assert np.allclose(o.xyz[0].numpy(), h.xyz[3:].mean(0).numpy(), atol=1e-6)           # = the mean over the four leaves
    ls = o.log_scales.numpy()
    assert (ls[:3, 0] <= ls[:3, 1]).all() and (ls[:3, 1] <= ls[:3, 2]).all()
    assert np.allclose(np.linalg.norm(o.rots.double().numpy(), axis=1), 1.0, atol=1e-6)


def test_remove_a_whole_subtree():
    h = hand_tree()
    r = hierarchy.prune_hierarchy(h, remove_boxes=[((-0.5, -1, -1), (1.5, 1, 1))])
    assert r.old_of_new.tolist() == [0, 2, 5, 6] and r.new_of_old.tolist() == [0, -1, 1, -1, -1, 2, 3]
    assert r.hierarchy.nodes.tolist() == [[0, -1, 0, 0, 1, 1, 1], [1, 0, 1, 0, 1, 2, 2], [2, 1, 2, 1, 0, 0, 0], [2, 1, 3, 1, 0, 0, 0]]
    assert (r.removed_leaves, r.dead, r.dirty, r.single_child) == (2, 3, 1, 1)
    o = r.hierarchy
    assert torch.equal(o.xyz[0], h.xyz[2]) and torch.equal(o.shs[0], h.shs[2]) and torch.equal(o.alpha[0], h.alpha[2])
    assert o.boxes[0, :, :3].tolist() == h.boxes[2, :, :3].tolist() and float(o.boxes[0, 1, 3]) == 0.0
    for k in ARRAYS[:5] + ("boxes",):
        assert torch.equal(bits(getattr(o, k)[1:]), bits(getattr(h, k)[[2, 5, 6]])), k


def test_remove_all_but_one_leaf():
    h = hand_tree()
    r = hierarchy.prune_hierarchy(h, keep_box=((5.5, -1, -1), (6.5, 1, 1)))
    assert r.old_of_new.tolist() == [0, 2, 5]
    assert r.hierarchy.nodes.tolist() == [[0, -1, 0, 0, 1, 1, 1], [1, 0, 1, 0, 1, 2, 1], [2, 1, 2, 1, 0, 0, 0]]
    assert (r.removed_leaves, r.dead, r.dirty, r.single_child) == (3, 4, 2, 2)
    o = r.hierarchy
    for n in (0, 1):                                   # a chain of single-child nodes: each is the leaf again
        assert torch.equal(o.xyz[n], h.xyz[5]) and torch.equal(o.shs[n], h.shs[5]) and torch.equal(o.alpha[n], h.alpha[5])
        assert np.allclose(cov_of(o.log_scales[n:n + 1], o.rots[n:n + 1]), cov_of(h.log_scales[5:6], h.rots[5:6]), rtol=1e-6)
        assert o.boxes[n, :, :3].tolist() == h.boxes[5, :, :3].tolist()
    q = hierarchy.prune_hierarchy(h, keep_box=((5.5, -1, -1), (6.5, 1, 1)), remerge="none")
    assert torch.equal(q.hierarchy.nodes, o.nodes) and torch.equal(bits(q.hierarchy.boxes), bits(o.boxes))
    for k in ARRAYS[:5]:
        assert torch.equal(bits(getattr(q.hierarchy, k)), bits(getattr(h, k)[[0, 2, 5]])), k


def test_remove_all_leaves_is_refused():
    h = hand_tree()
    for kw in ({"remove": mask_of(3, 4, 5, 6)}, {"min_opacity": 2.0}, {"max_scale": 1e-3}, {"keep_box": ((50, 50, 50), (60, 60, 60))}):
        with pytest.raises(hierarchy.HierarchyPruneError) as e:
            hierarchy.prune_hierarchy(h, **kw)
        assert e.value.check == hierarchy.PRUNE_ROOT_DEAD and e.value.node == 0 and "every leaf would be removed" in str(e.value)


def test_remove_nothing_returns_the_bits():
    h = hand_tree()
    for kw in ({}, {"remove": mask_of(0, 1, 2)}, {"min_opacity": 0.0}, {"max_scale": 100.0}, {"remove_boxes": []},
               {"keep_box": ((-9, -9, -9), (9, 9, 9))}, {"remerge": "none"}):
        r = hierarchy.prune_hierarchy(h, **kw)
        for k in ARRAYS:
            assert torch.equal(bits(getattr(r.hierarchy, k)), bits(getattr(h, k))), (kw, k)
        assert r.old_of_new.tolist() == list(range(7)) == r.new_of_old.tolist()
        assert (r.removed_leaves, r.dead, r.dirty, r.single_child) == (0, 0, 0, 0)


# ---- built and merged hierarchies ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pruned(P, kind, remerge="dirty"):
    """The spec's result (or None where the root dies) -- computed once, shared with the GPU tests; do not modify."""
    h = case(P)
    try:
        return hierarchy.prune_hierarchy(h, remove=removal_mask(h, kind), remerge=remerge)
    except hierarchy.HierarchyPruneError:
        return None


def dirty_new(h, r):
    """bool [N']: the output nodes that are ancestors of a dead node."""
    parent, m = h.nodes.numpy()[:, 1], r.new_of_old.numpy()
    above = np.zeros(m.shape[0], dtype=bool)             # old ids: a dead node somewhere below
    front = np.unique(parent[m < 0])
    while front.size:
        front = front[(front >= 0) & ~above[np.maximum(front, 0)]]
        above[front] = True
        front = np.unique(parent[front])
    return (above & (m >= 0))[r.old_of_new.numpy()]


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("P", SIZES + ("merged",))
def test_properties_of_every_output(P, kind):
    h, r = case(P), pruned(P, kind)
    nd = h.nodes.numpy()
    mask = removal_mask(h, kind)
    leaves = nd[:, 6] == 0
    if r is None:
        assert (mask[leaves] != 0).all()             # refused exactly where every leaf goes (P = 1, a root-only tree, ...)
        return
    o = r.hierarchy
    out = o.nodes.numpy()
    check_layout(out)
    assert nested_np(out, o.boxes.numpy())
    old, new = r.old_of_new.numpy(), r.new_of_old.numpy()
    assert np.array_equal(new[old], np.arange(old.size)) and int((new >= 0).sum()) == old.size and (np.diff(old) > 0).all()
    assert np.array_equal(np.nonzero(new < 0)[0][leaves[new < 0]], np.nonzero(leaves & (mask != 0))[0])
    assert r.removed_leaves == int((leaves & (mask != 0)).sum()) and r.dead == nd.shape[0] - old.size
    d = dirty_new(h, r)
    assert r.dirty == int(d.sum()) and r.single_child == int((out[:, 6] == 1).sum())
    assert np.array_equal(out[:, [0, 3, 4]], nd[old][:, [0, 3, 4]])
    clean = torch.from_numpy(~d)
    for k in ARRAYS[:5] + ("boxes",):
        assert torch.equal(bits(getattr(o, k)[clean]), bits(getattr(h, k)[torch.from_numpy(old)][clean])), k
    assert torch.equal(bits(o.boxes[:, 1, 3]), bits(h.boxes[torch.from_numpy(old), 1, 3]))
    # the same criteria again remove nothing and return the same bits
    again = hierarchy.prune_hierarchy(o, remove=mask[old])
    assert again.dead == 0 and again.dirty == 0
    for k in ARRAYS:
        assert torch.equal(bits(getattr(again.hierarchy, k)), bits(getattr(o, k))), k
    # a topology-only prune: every row a bit copy, the same records and boxes
    t = pruned(P, kind, "none")
    assert torch.equal(t.hierarchy.nodes, o.nodes) and torch.equal(bits(t.hierarchy.boxes), bits(o.boxes))
    for k in ARRAYS[:5]:
        assert torch.equal(bits(getattr(t.hierarchy, k)), bits(getattr(h, k)[torch.from_numpy(old)])), k


def test_the_dirty_rows_carry_nothing_of_what_was_removed():
    """A box of leaves removed: whatever the removed leaves held -- here their rows are replaced by rubbish before a
    second run with the same mask -- no bit of the output changes, at any level.  (What is checked here is that nothing
    of the removed leaves is left in any row; the hand-built tree above and tests/test_hier_merge_rule_on_host.py check
    that the merge of the survivors is the rule's.)"""
    h = built(2000)
    x = h.xyz.numpy()
    nd = h.nodes.numpy()
    lo, hi = np.quantile(x, 0.3, axis=0), np.quantile(x, 0.7, axis=0)
    r = hierarchy.prune_hierarchy(h, remove_boxes=[(lo, hi)])
    o = r.hierarchy
    assert 50 < r.removed_leaves < 600 and r.dirty > 10
    out_leaf = o.nodes[:, 6].numpy() == 0
    inside = ((o.xyz.numpy() >= lo.astype(np.float32)) & (o.xyz.numpy() <= hi.astype(np.float32))).all(1)
    assert not (out_leaf & inside).any()
    gone = (nd[:, 6] == 0) & (r.new_of_old.numpy() < 0)
    mask = gone.astype(np.uint8)
    c = clone(h)
    g = torch.Generator().manual_seed(11)
    n = int(gone.sum())
    gi = torch.from_numpy(np.nonzero(gone)[0])
    c.xyz[gi] = 1e3 * torch.randn(n, 3, generator=g)
    c.shs[gi] = 50 * torch.randn(n, 16, 3, generator=g)
    c.alpha[gi] = torch.rand(n, 1, generator=g)
    c.log_scales[gi] = 3 * torch.randn(n, 3, generator=g)
    c.rots[gi] = torch.randn(n, 4, generator=g)
    c.boxes[gi] = 1e3 * torch.randn(n, 2, 4, generator=g)
    for mode in ("dirty", "all"):
        a, b = hierarchy.prune_hierarchy(h, remove=mask, remerge=mode), hierarchy.prune_hierarchy(c, remove=mask, remerge=mode)
        for k in ARRAYS:
            assert torch.equal(bits(getattr(a.hierarchy, k)), bits(getattr(b.hierarchy, k))), (mode, k)
    # the mask and the box select the same leaves, so the two results are the same bits
    a = hierarchy.prune_hierarchy(h, remove=mask)
    for k in ARRAYS:
        assert torch.equal(bits(getattr(a.hierarchy, k)), bits(getattr(o, k))), k
    # every re-merged mean lies in the box of its surviving children's means
    d = np.nonzero(dirty_new(h, r))[0]
    on, ox = o.nodes.numpy(), o.xyz.numpy()
    for i in d:
        kids = ox[on[i, 5]:on[i, 5] + on[i, 6]]
        assert (ox[i] >= kids.min(0) - 1e-5).all() and (ox[i] <= kids.max(0) + 1e-5).all(), i


@pytest.mark.parametrize("P", (257, 2000))
def test_remerge_all_with_nothing_removed_gives_the_builders_rows_back(P):
    """The weights are the builder's (carried up from the leaves), so every interior row comes back within the builder's
    bounds: mean, SH, opacity 1e-5 (parity.assert_stats), covariance 1e-5 Frobenius per node."""
    import parity as pa
    h = built(P)
    o = hierarchy.prune_hierarchy(h, remerge="all").hierarchy
    s = h.nodes[:, 6] > 0
    pa.assert_stats("all vs the input", {k: pa.err_stats(getattr(o, k)[s], getattr(h, k)[s]) for k in ("xyz", "shs", "alpha")},
                    rel_tol=1e-5)
    unit = lambda q: (q.double() / q.double().norm(dim=1, keepdim=True)).numpy()
    cg, cw = cov_of(o.log_scales[s], unit(o.rots[s])), cov_of(h.log_scales[s], unit(h.rots[s]))
    rel = np.linalg.norm(cg - cw, axis=(1, 2)) / np.linalg.norm(cw, axis=(1, 2))
    assert float(rel.max()) <= 1e-5, float(rel.max())
    assert torch.equal(o.nodes, h.nodes) and torch.equal(bits(o.boxes), bits(h.boxes))


def test_each_criterion_selects_what_a_direct_statement_selects():
    h = clone(built(2000))
    nd = h.nodes.numpy()
    N = nd.shape[0]
    leaf = nd[:, 6] == 0
    ids = np.nonzero(leaf)[0]
    h.xyz[ids[3], 1] = float("nan")                   # a NaN mean: in no remove box, outside every keep box
    h.alpha[ids[5], 0] = float("nan")                 # a NaN opacity fails every floor
    h.log_scales[ids[7], 0] = float("nan")            # a NaN log-scale (not the largest) fails every ceiling
    h.log_scales[ids[7], 1:] = -9.0
    x, a, ls = h.xyz.numpy(), h.alpha.numpy().reshape(-1), h.log_scales.numpy()
    lo, hi = np.quantile(x[leaf & ~np.isnan(x).any(1)], 0.25, axis=0).astype(np.float32), \
        np.quantile(x[leaf & ~np.isnan(x).any(1)], 0.75, axis=0).astype(np.float32)
    A = np.float32(np.nanquantile(a[leaf], 0.1))
    S = float(np.exp(np.nanquantile(ls[leaf].max(1), 0.9)))

    def removed_by(**kw):
        r = hierarchy.prune_hierarchy(h, remerge="none", **kw)
        return leaf & (r.new_of_old.numpy() < 0), r

    def in_box(lo_, hi_):
        with np.errstate(invalid="ignore"):
            return np.array([all(lo_[k] <= x[i, k] <= hi_[k] for k in range(3)) for i in range(N)])
    got, _ = removed_by(remove_boxes=[(lo, hi)])
    assert np.array_equal(got, leaf & in_box(lo, hi)) and not got[ids[3]] and 100 < got.sum() < 1900
    lo2, hi2 = lo + 2.0, hi + 2.0
    got, _ = removed_by(remove_boxes=[(lo, hi), (lo2, hi2)])
    assert np.array_equal(got, leaf & (in_box(lo, hi) | in_box(lo2, hi2)))
    got, _ = removed_by(keep_box=(lo, hi))
    assert np.array_equal(got, leaf & ~in_box(lo, hi)) and got[ids[3]]
    got, _ = removed_by(min_opacity=A)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got, leaf & ~(a >= A)) and got[ids[5]] and 100 < got.sum() < 400
    got, _ = removed_by(max_scale=S)
    L = np.float32(np.log(np.float64(S)))
    with np.errstate(invalid="ignore"):
        want = leaf & np.array([not (ls[i, 0] <= L and ls[i, 1] <= L and ls[i, 2] <= L) for i in range(N)])
    assert np.array_equal(got, want) and got[ids[7]] and 100 < got.sum() < 400
    mask = (np.arange(N) % 5 == 0).astype(np.uint8)
    got, _ = removed_by(remove=mask)
    assert np.array_equal(got, leaf & (mask != 0))
    got, _ = removed_by(remove=torch.from_numpy(mask).bool())
    assert np.array_equal(got, leaf & (mask != 0))
    got, r = removed_by(remove_boxes=[(lo, hi)], min_opacity=A, max_scale=S, remove=mask)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got, leaf & (in_box(lo, hi) | ~(a >= A) | want | (mask != 0)))
    assert r.removed_leaves == int(got.sum())
    # closed boxes: a leaf on the face is inside
    p = x[ids[20]]
    got, _ = removed_by(remove_boxes=[(p, p)])
    assert got[ids[20]]
    for bad in ({"remove_boxes": [((0, 0, 0), (1, 1, 1))] * 17}, {"min_opacity": float("nan")}, {"max_scale": 0.0},
                {"max_scale": float("nan")}, {"keep_box": ((0, 0, float("nan")), (1, 1, 1))}, {"remove": np.zeros(N - 1)},
                {"remerge": "some"}):
        with pytest.raises(ValueError):
            hierarchy.prune_hierarchy(h, **bad)


def test_rejections_name_their_node():
    from test_hier_refit_cpu import corruptions
    seen = 0
    for name, c, mode, check, node in corruptions():
        if check is not None and check >= 6:
            continue                                  # the leaf-box kinds are the refit's alone
        with pytest.raises(hierarchy.HierarchyPruneError) as e:
            hierarchy.prune_hierarchy(c, min_opacity=0.01)
        want = hierarchy.PRUNE_CHILDREN_SUM if check is None else hierarchy.PRUNE_CHECKS[check]
        assert e.value.check == want and e.value.node == node, (name, e.value.check, e.value.node)
        seen += 1
    assert seen == 11 and hierarchy.PRUNE_CHECKS == hierarchy.REFIT_CHECKS[:6]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
NAMES = ("hgs_hier_prune_tmp_bytes", "hgs_hier_prune_plan", "hgs_hier_prune_apply")


def test_the_abi_declares_and_binds_the_three_entries():
    plain = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, plain), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert re.search(r"#define\s+HGS_ABI_VERSION\s+14\b", HEADER) and _lib.ABI_VERSION == 14
    assert re.search(r"#define\s+HGS_HIER_PRUNE_MAX_BOXES\s+16\b", HEADER) and _lib.HIER_PRUNE_MAX_BOXES == 16
    assert C.sizeof(_lib.HierPruneArgs) == 16 + 2 * 16 * 12 + 24 + 8 and C.sizeof(_lib.HierPruneReport) == 32 + 6 * 8
    assert _lib.HierPruneArgs.remove_hi.offset == 16 + 192 and _lib.HierPruneArgs.keep_lo.offset == 16 + 384
    assert _lib.HierPruneReport.kept.offset == 32 and _lib.HierPruneReport.children_sum.offset == 72
    assert hierarchy.PRUNE_REMERGE == {"none": _lib.HIER_PRUNE_REMERGE_NONE, "dirty": _lib.HIER_PRUNE_REMERGE_DIRTY,
                                       "all": _lib.HIER_PRUNE_REMERGE_ALL}
    for k, v in (("NONE", 0), ("DIRTY", 1), ("ALL", 2)):
        assert re.search(r"#define\s+HGS_HIER_PRUNE_REMERGE_%s\s+%d\b" % (k, v), HEADER)


def test_tmp_bytes_needs_no_gpu():
    lib = _lib.lib()
    for N in (0, -1, 1 << 31, 1 << 40, -(1 << 40)):
        assert lib.hgs_hier_prune_tmp_bytes(N) == 0, N
    grid = (1, 2, 255, 256, 257, 8191, 8192, 8193, 2_097_151, 2_097_152, 2_097_153, 50_000_000, (1 << 31) - 1)
    sizes = [lib.hgs_hier_prune_tmp_bytes(N) for N in grid]
    assert all(b > 0 and b % 256 == 0 for b in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    # the report block, three words, a flag byte and two doubles per node, the sort's own workspace
    for N, b in zip(grid[:-1], sizes):
        assert b >= 1024 + 29 * N + lib.hgs_sort_tmp_bytes(N), (N, b)


def _view(N, G=None, M=16, base=4096, **at):
    a = {k: base for k in ARRAYS}
    a.update(at)
    return _lib.HierView(N if G is None else G, N, M, 0, *(a[k] for k in ARRAYS))


def test_bad_arguments_fail_before_any_hip_call():
    """(No GPU here: a call that got as far as HIP would return HGS_ERR_HIP, not HGS_ERR_INVALID.)"""
    lib = _lib.lib()
    rep, ok = _lib.HierPruneReport(), _lib.HierPruneArgs()
    a = 4096

    def args(**kw):
        x = _lib.HierPruneArgs()
        for k, v in kw.items():
            setattr(x, k, v)
        return x
    nan_box = args(remove_boxes=2)
    nan_box.remove_hi[1][2] = float("nan")
    nan_keep = args(use_keep_box=1)
    nan_keep.keep_lo[0] = float("nan")
    plan = [((_view(0), ok, None, a, rep), b"bad sizes"), ((_view(1 << 31), ok, None, a, rep), b"bad sizes"),
            ((_view(-3), ok, None, a, rep), b"bad sizes"), ((_view(5, G=4), ok, None, a, rep), b"bad sizes"),
            ((_view(5, M=0), ok, None, a, rep), b"bad sizes"), ((_view(5, M=65), ok, None, a, rep), b"bad sizes"),
            ((_view(5, xyz=0), ok, None, a, rep), b"null"), ((_view(5, nodes=0), ok, None, a, rep), b"null"),
            ((_view(5), ok, None, None, rep), b"null"), ((_view(5, rots=a + 8), ok, None, a, rep), b"16-byte"),
            ((_view(5, boxes=a + 4), ok, None, a, rep), b"16-byte"), ((_view(5, alpha=a + 2), ok, None, a, rep), b"4-byte"),
            ((_view(5), ok, None, a + 64, rep), b"256-byte"),
            ((_view(5), args(remove_boxes=17), None, a, rep), b"remove boxes"),
            ((_view(5), args(remove_boxes=-1), None, a, rep), b"remove boxes"),
            ((_view(5), nan_box, None, a, rep), b"NaN"), ((_view(5), nan_keep, None, a, rep), b"NaN"),
            ((_view(5), args(use_min_opacity=1, min_opacity=float("nan")), None, a, rep), b"NaN"),
            ((_view(5), args(use_max_scale=1, log_max_scale=float("nan")), None, a, rep), b"NaN")]
    for (v, ar, mask, tmp, rp), word in plan:
        assert lib.hgs_hier_prune_plan(C.byref(v), C.byref(ar), mask, tmp, C.byref(rp), None, 0) == 1, word
        assert word in lib.hgs_last_error(), (word, lib.hgs_last_error())
    assert lib.hgs_hier_prune_plan(None, C.byref(ok), None, a, C.byref(rep), None, 0) == 1 and b"null" in lib.hgs_last_error()
    assert lib.hgs_hier_prune_plan(C.byref(_view(5)), None, None, a, C.byref(rep), None, 0) == 1 and b"null" in lib.hgs_last_error()
    assert lib.hgs_hier_prune_plan(C.byref(_view(5)), C.byref(ok), None, a, None, None, 0) == 1 and b"null" in lib.hgs_last_error()
    # a NaN in a bound that is not in use is not looked at: the call gets past the criteria (and fails at tmp here)
    unused = args(min_opacity=float("nan"))
    assert lib.hgs_hier_prune_plan(C.byref(_view(5)), C.byref(unused), None, a + 64, C.byref(rep), None, 0) == 1
    assert b"256-byte" in lib.hgs_last_error()
    far = a + (1 << 20)
    vin, vout = _view(5), _view(3, base=far)
    plan = [((_view(0), vout, a, 1, far, far), b"bad sizes"), ((vin, _view(3, G=2, base=far), a, 1, far, far), b"bad sizes"),
            ((vin, _view(3, M=4, base=far), a, 1, far, far), b"M="), ((vin, vout, None, 1, far, far), b"null"),
            ((vin, vout, a, 1, None, far), b"null"), ((vin, vout, a, 1, far, None), b"null"),
            ((vin, vout, a + 64, 1, far, far), b"256-byte"), ((vin, vout, a, 1, far + 2, far), b"4-byte"),
            ((vin, _view(3, base=far, rots=far + 8), a, 1, far, far), b"16-byte"),
            ((vin, vout, a, 3, far, far), b"remerge"), ((vin, vout, a, -1, far, far), b"remerge"),
            ((vin, vout, a, 1, far, far), b"no successful hgs_hier_prune_plan")]
    for (vi, vo, tmp, mode, oon, noo), word in plan:
        assert lib.hgs_hier_prune_apply(C.byref(vi), C.byref(vo), tmp, mode, oon, noo, None, 0) == 1, word
        assert word in lib.hgs_last_error(), (word, lib.hgs_last_error())
    assert lib.hgs_hier_prune_apply(None, C.byref(vout), a, 1, far, far, None, 0) == 1 and b"null" in lib.hgs_last_error()


def test_the_gpu_function_has_no_cpu_fallback():
    if torch.cuda.is_available():
        return                      # (with a GPU the call runs: tests/test_hier_prune_gpu.py)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hierarchy.prune_hierarchy_gpu(built(2), min_opacity=0.5)


# ---- the command ---------------------------------------------------------------------------------------------------------
def test_the_command_parses_its_arguments(capsys):
    p = prune_cmd.parse_args
    got = p(["a.hier", "b.hier", "--min-opacity", "0.05"])
    assert got == dict(in_path="a.hier", out_path="b.hier", remove_boxes=[], keep_box=None, min_opacity=0.05, max_scale=None,
                       mask=None, remerge="dirty", align=False, half=False)
    got = p(["--remove-box", "0", "0", "0", "1", "1", "1", "a.hier", "--remove-box", "-1", "-2", "-3", "4", "5", "6", "b.hier",
             "--keep-box", "0", "0", "0", "9", "9", "9", "--max-scale", "2", "--mask", "m.npy", "--remerge", "all", "--align", "--half"])
    assert got["remove_boxes"] == [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((-1.0, -2.0, -3.0), (4.0, 5.0, 6.0))]
    assert got["keep_box"] == ((0.0, 0.0, 0.0), (9.0, 9.0, 9.0)) and got["max_scale"] == 2.0 and got["mask"] == "m.npy"
    assert got["remerge"] == "all" and got["align"] and got["half"] and (got["in_path"], got["out_path"]) == ("a.hier", "b.hier")
    assert p(["a.hier", "b.hier", "--min-opacity", "0.1", "--min-opacity", "0.2", "--remerge", "none"])["min_opacity"] == 0.2
    box = ["--remove-box", "0", "0", "0", "1", "1", "1"]
    bad = ([], ["a.hier", "b.hier"], ["a.hier", "b.hier", "--remerge", "all"], ["a.hier", "b.hier", "--align", "--half"],
           ["a.hier", "--min-opacity", "0.1"], ["a.hier", "b.hier", "c.hier", "--min-opacity", "0.1"],
           ["a.hier", "b.hier", "--remove-box", "0", "0", "0", "1", "1"], ["a.hier", "b.hier", "--keep-box", "0", "0", "0"],
           ["a.hier", "b.hier", "--min-opacity"], ["a.hier", "b.hier", "--min-opacity", "x"], ["a.hier", "b.hier", "--max-scale", "0"],
           ["a.hier", "b.hier", "--max-scale", "nan"], ["a.hier", "b.hier", "--min-opacity", "0.1", "--remerge", "some"],
           ["a.hier", "b.hier", "--min-opacity", "0.1", "--frobnicate"], ["a.hier", "b.hier", "--frobnicate", "--min-opacity", "0.1"],
           ["a.hier", "b.hier"] + box * 17)
    for argv in bad:
        assert p(argv) is None, argv
        assert prune_cmd.main(argv) == 2, argv
    assert "usage: python -m hgs.prune_hierarchy" in capsys.readouterr().err
    assert p(["a.hier", "b.hier"] + box * 16) is not None
    assert prune_cmd.main(["/nonexistent/in.hier", "out.hier", "--min-opacity", "0.1"]) == 2
    assert "does not exist" in capsys.readouterr().err


def test_the_anchors_remap(tmp_path):
    new_of_old = np.array([0, 1, -1, 2, -1, -1, 3, 4], dtype=np.int32)
    kept, dropped = prune_cmd.remap_anchors([7, 2, 3, 3, 5, 0, 6], new_of_old)
    assert kept.tolist() == [4, 2, 2, 0, 3] and kept.dtype == np.int32 and dropped == 2
    kept, dropped = prune_cmd.remap_anchors(np.array([], dtype=np.int32), new_of_old)
    assert kept.tolist() == [] and dropped == 0
    kept, dropped = prune_cmd.remap_anchors([8, -1, 1], new_of_old)        # outside the map: dropped
    assert kept.tolist() == [1] and dropped == 2
    # the file: an int32 count, then the indices, little-endian, as the reference's loader reads it
    path = str(tmp_path / "anchors.bin")
    prune_cmd.write_anchors(path, [4, 2, 2, 0, 3])
    raw = open(path, "rb").read()
    assert len(raw) == 24 and int.from_bytes(raw[:4], "little") == 5
    assert np.frombuffer(raw[4:], dtype=np.int32).tolist() == [4, 2, 2, 0, 3]
    assert prune_cmd.read_anchors(path).tolist() == [4, 2, 2, 0, 3]
    (tmp_path / "in").mkdir()
    (tmp_path / "out").mkdir()
    prune_cmd.write_anchors(str(tmp_path / "in" / "anchors.bin"), [7, 2, 3])
    (tmp_path / "in" / "exposure.json").write_text('{"a": [1, 0, 0]}')
    done = prune_cmd.carry_side_files(str(tmp_path / "in" / "x.hier"), str(tmp_path / "out" / "y.hier"), new_of_old)
    assert done == dict(anchors=(3, 1), exposure=True)
    assert prune_cmd.read_anchors(str(tmp_path / "out" / "anchors.bin")).tolist() == [4, 2]
    assert (tmp_path / "out" / "exposure.json").read_text() == '{"a": [1, 0, 0]}'
