"""The trimming rule (hgs.hierarchy.trim_hierarchy, the numpy spec of csrc/hier_trim.hip) without a GPU: a hand-built
tree with its expected output written out, the budget's tie rule, identity and root-only, the exactness contract against
oracle/lod_oracle.py on a 2 000-leaf scene (cuts equal after mapping, weights as bit patterns) and the graceful relation
where it does not hold, a region, the node budget, a merged hierarchy, the four rejections, the C ABI's declarations and
host-only entry, the command's argument parsing.  tests/test_hier_trim_gpu.py holds the HIP calls against this spec."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from hgs import _lib, hierarchy, synth
from hgs import trim_hierarchy as trim_cmd
from oracle import lod_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = synth.make_camera(256, 160)
ARRAYS = ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes")
VIEWS = ((0.0, 0.0, -5.0), (30.0, 2.0, 10.0), (0.0, 40.0, 10.0))      # all outside the scene's root box
ROI = ((-2.0, -2.0, 5.0), (2.0, 2.0, 12.0))
INF = float("inf")


def bits(t):
    return t.contiguous().view(torch.int32)


def clone(h):
    return hierarchy.Hierarchy(*(getattr(h, k).clone() for k in ARRAYS))


# ---- the hand-built tree -------------------------------------------------------------------------------------------
#        0 (extent 8)
#    1 (2)        2 (4)
#  3 (1) 4 (1)  5 (1) 6 (1)
def hand_tree(e1=2.0, e2=4.0):
    nodes = torch.tensor([[0, -1, 0, 0, 1, 1, 2], [1, 0, 1, 0, 1, 3, 2], [1, 0, 2, 0, 1, 5, 2], [2, 1, 3, 1, 0, 0, 0],
                          [2, 1, 4, 1, 0, 0, 0], [2, 2, 5, 1, 0, 0, 0], [2, 2, 6, 1, 0, 0, 0]], dtype=torch.int32)
    lo_ = [[0, 0, 0], [0, 0, 0], [4, 4, 4], [0, 0, 0], [1, 1, 1], [4, 4, 4], [7, 7, 7]]
    hi_ = [[8, 8, 8], [2, 2, 2], [8, 8, 8], [1, 1, 1], [2, 2, 2], [5, 5, 5], [8, 8, 8]]
    boxes = torch.zeros(7, 2, 4)
    boxes[:, 0, :3], boxes[:, 1, :3] = torch.tensor(lo_, dtype=torch.float32), torch.tensor(hi_, dtype=torch.float32)
    boxes[:, 0, 3] = torch.tensor([8.0, e1, e2, 1.0, 1.0, 1.0, 1.0])
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g)
    return hierarchy.Hierarchy(r(7, 3), r(7, 16, 3), r(7, 1).abs(), r(7, 3), r(7, 4), nodes, boxes)


def test_hand_built_tree_at_a_floor():
    h = hand_tree()
    r = hierarchy.trim_hierarchy(h, min_extent=3.0)
    # test: 0 and 2 pass; kept: 0, its children 1 and 2, the children 5 and 6 of 2; node 1 lost its children: a stub
    assert r.old_of_new.tolist() == [0, 1, 2, 5, 6] and r.old_of_new.dtype == torch.int32
    assert r.new_of_old.tolist() == [0, 1, 2, -1, -1, 3, 4] and r.new_of_old.dtype == torch.int32
    assert r.hierarchy.nodes.tolist() == [[0, -1, 0, 0, 1, 1, 2], [1, 0, 1, 1, 0, 0, 0], [1, 0, 2, 0, 1, 3, 2],
                                          [2, 2, 3, 1, 0, 0, 0], [2, 2, 4, 1, 0, 0, 0]]
    assert r.stubs == 1 and r.stub_ids.tolist() == [1] and r.min_extent == 3.0
    keep = torch.tensor([0, 1, 2, 5, 6])
    for k in ARRAYS[:5] + ("boxes",):
        assert torch.equal(bits(getattr(r.hierarchy, k)), bits(getattr(h, k)[keep])), k
    # the same set from a region that only node 2's side meets
    q = hierarchy.trim_hierarchy(h, roi=((5.0, 5.0, 5.0), (6.0, 6.0, 6.0)))
    assert q.old_of_new.tolist() == [0, 1, 2, 5, 6] and q.stubs == 1
    assert torch.equal(q.hierarchy.nodes, r.hierarchy.nodes)
    # a closed region: touching counts
    assert hierarchy.trim_hierarchy(h, roi=((2.0, 2.0, 2.0), (3.0, 3.0, 3.0))).old_of_new.tolist() == [0, 1, 2, 3, 4]
    assert hierarchy.trim_hierarchy(h, roi=((2.5, 2.5, 2.5), (3.0, 3.0, 3.0))).old_of_new.tolist() == [0, 1, 2]


def test_equal_extents_go_in_together_or_not_at_all():
    h = hand_tree(4.0, 4.0)
    nd, bx = h.nodes.numpy(), h.boxes.numpy()
    # candidates: 8 (2 children) then 4, 4 (2 + 2 children): 1 + 2 = 3 nodes, or all 7
    for K, want, n in ((2, INF, 1), (3, 8.0, 3), (4, 8.0, 3), (5, 8.0, 3), (6, 8.0, 3), (7, 4.0, 7), (100, 4.0, 7)):
        assert float(hierarchy.trim_budget_extent(nd, bx, K)) == want, K
        r = hierarchy.trim_hierarchy(h, max_nodes=K)
        assert r.hierarchy.num_nodes == n and r.min_extent == want, K
    r = hierarchy.trim_hierarchy(h, max_nodes=5)
    assert r.stubs == 2 and r.hierarchy.nodes.tolist() == [[0, -1, 0, 0, 1, 1, 2], [1, 0, 1, 1, 0, 0, 0], [1, 0, 2, 1, 0, 0, 0]]
    # the larger of the budget's floor and the given one is used
    assert hierarchy.trim_hierarchy(h, min_extent=9.0, max_nodes=7).hierarchy.num_nodes == 1
    assert hierarchy.trim_hierarchy(h, min_extent=1.0, max_nodes=5).min_extent == 8.0


# ---- the 2 000-leaf scene --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene2000():
    """(hierarchy, the median extent of its nodes with children)."""
    h = hierarchy.build_hierarchy(synth.make_scene_trained_like(2000, CAM, seed=5))
    ext = h.boxes[:, 0, 3].numpy()
    return h, float(np.median(ext[h.nodes[:, 6].numpy() > 0]))


@functools.lru_cache(maxsize=None)
def trimmed2000():
    h, med = scene2000()
    return hierarchy.trim_hierarchy(h, med)


def oracle_cut(h, tau, v):
    nd, bx = h.nodes.numpy(), h.boxes.numpy()
    ri, pi, ni = lo.expand_to_size(nd, bx, tau, v)
    w, kids = lo.get_interpolation_weights(ni, tau, nd, bx, v)
    return ri, pi, ni, w, kids


def stub_tau(r, v):
    """The smallest granularity at which every stub of ``r`` is fine enough from v: nextafter(the largest stub size)."""
    s = lo.node_size(r.hierarchy.boxes.cpu().numpy(), r.stub_ids.cpu().numpy().astype(np.int64), v)
    assert np.isfinite(s).all() and s.max() < lo.FLT_MAX
    return np.nextafter(np.float32(s.max()), np.float32(np.inf))


def assert_cuts_equal_after_mapping(orig_cut, trimmed_cut, new_of_old):
    (ri, pi, ni, w, kids), (tri, tpi, tni, tw, tkids) = orig_cut, trimmed_cut
    m = np.asarray(new_of_old)
    assert len(ri) == len(tri) > 0
    for a, b in ((ri, tri), (pi, tpi), (ni, tni)):
        assert (m[a] >= 0).all() and np.array_equal(m[a], b)
    assert np.array_equal(np.asarray(w).view(np.uint32), np.asarray(tw).view(np.uint32))
    assert np.array_equal(kids, tkids)


def nearest_kept_ancestors(nodes, new_of_old, ids):
    """Every node of ``ids`` replaced by its nearest kept ancestor (itself if kept), each once, ascending, new numbering."""
    parent, m = np.asarray(nodes)[:, 1], np.asarray(new_of_old)
    out = set()
    for n in ids:
        n = int(n)
        while m[n] < 0:
            n = int(parent[n])
        out.add(int(m[n]))
    return np.array(sorted(out), dtype=np.int64)


def assert_graceful(h, r, tau, v, orig_ni, trimmed_ni, trimmed_w):
    want = nearest_kept_ancestors(h.nodes.numpy(), r.new_of_old.cpu().numpy(), orig_ni)
    assert np.array_equal(np.asarray(trimmed_ni, dtype=np.int64), want)
    stubs = r.stub_ids.cpu().numpy().astype(np.int64)
    size = lo.node_size(r.hierarchy.boxes.cpu().numpy(), np.asarray(trimmed_ni, dtype=np.int64), v)
    coarse_stub = np.isin(trimmed_ni, stubs) & (size >= np.float32(tau))
    assert coarse_stub.any()
    assert np.array_equal(np.asarray(trimmed_w)[coarse_stub].view(np.uint32),
                          np.ones(int(coarse_stub.sum()), dtype=np.float32).view(np.uint32))


def test_the_scene_trims_to_the_documented_sizes():
    h, med = scene2000()
    r = trimmed2000()
    assert (h.num_nodes, r.hierarchy.num_nodes, r.stubs, r.stub_ids.numel()) == (3999, 2001, 435, 435)
    assert r.min_extent == float(np.float32(med))
    # the builder's extents are monotone from parent to child: the keep set is closed by construction
    ext, parent = h.boxes[:, 0, 3].numpy(), h.nodes[:, 1].numpy()
    assert (ext[1:] <= ext[parent[1:]]).all()


@pytest.mark.parametrize("v,emitted", list(zip(VIEWS, ((107, 399), (120, 517), (266, 799)))))
def test_exactness_from_outside_views(v, emitted):
    h, _ = scene2000()
    r = trimmed2000()
    tau = stub_tau(r, v)
    a, b = oracle_cut(h, tau, v), oracle_cut(r.hierarchy, tau, v)
    assert_cuts_equal_after_mapping(a, b, r.new_of_old.numpy())
    n_stubs = int(np.isin(b[2], r.stub_ids.numpy()).sum())
    assert n_stubs >= 1 and (n_stubs, len(b[0])) == emitted
    assert r.exact_for(v, tau) is True and r.exact_for(torch.tensor(v), float(tau)) is True
    assert r.exact_for(v, tau / np.float32(10)) is False
    assert r.exact_for(v, np.nextafter(tau, np.float32(0))) is False        # the bound is sharp
    # a tenth of that: stubs stand in for what was dropped
    t10 = tau / np.float32(10)
    a, b = oracle_cut(h, t10, v), oracle_cut(r.hierarchy, t10, v)
    assert len(a[0]) > len(b[0])
    assert_graceful(h, r, t10, v, a[2], b[2], b[3])


def meets(boxes, roi):
    lo_, hi_ = np.asarray(roi[0], dtype=np.float32), np.asarray(roi[1], dtype=np.float32)
    return (boxes[:, 0, :3] <= hi_).all(1) & (boxes[:, 1, :3] >= lo_).all(1)


def check_layout(nodes):
    """The three layout checks, restated node by node."""
    nd = np.asarray(nodes)
    N = nd.shape[0]
    assert nd[0, 1] == -1
    for i in range(N):
        depth, parent, start, leafs, merged, sc, cc = (int(x) for x in nd[i])
        assert start == i and leafs + merged == 1, i
        assert cc >= 0 and (cc == 0 or (sc >= 1 and sc + cc <= N)), i
        if i:
            assert 0 <= parent < N and nd[parent, 5] <= i < nd[parent, 5] + nd[parent, 6], i
            assert depth == nd[parent, 0] + 1, i
    assert int(nd[:, 6].sum()) == N - 1


def test_region():
    h, _ = scene2000()
    r = hierarchy.trim_hierarchy(h, roi=ROI)
    assert r.hierarchy.num_nodes == 1323
    nd, bx = h.nodes.numpy(), h.boxes.numpy()
    m, inside = r.new_of_old.numpy(), meets(bx, ROI)
    leaves = np.nonzero((nd[:, 6] == 0) & inside)[0]
    assert leaves.size > 50
    for n in leaves:                                   # every leaf that meets the region, with its path to the root
        while n >= 0:
            assert m[n] >= 0
            n = nd[n, 1]
    dropped = np.nonzero(m < 0)[0]
    assert dropped.size == 3999 - 1323 and not inside[nd[dropped, 1]].any()
    check_layout(r.hierarchy.nodes.numpy())
    # with a floor as well: every dropped node's parent misses the region or lies below the floor
    _, med = scene2000()
    q = hierarchy.trim_hierarchy(h, med, ROI)
    d = np.nonzero(q.new_of_old.numpy() < 0)[0]
    pt = inside[nd[d, 1]] & (bx[nd[d, 1], 0, 3] >= np.float32(med))
    assert 1 < q.hierarchy.num_nodes < 1323 and not pt.any()
    check_layout(q.hierarchy.nodes.numpy())


def test_identity_and_root_only():
    h, _ = scene2000()
    for kw in ({}, {"min_extent": 0.0}, {"min_extent": -1.0}, {"max_nodes": 3999}, {"max_nodes": 10 ** 9}):
        r = hierarchy.trim_hierarchy(h, **kw)
        for k in ARRAYS:
            assert torch.equal(bits(getattr(r.hierarchy, k)), bits(getattr(h, k))), (kw, k)
        assert torch.equal(r.old_of_new, torch.arange(3999, dtype=torch.int32)) and r.stubs == 0
        assert torch.equal(r.new_of_old, torch.arange(3999, dtype=torch.int32))
        assert r.exact_for((0.0, 0.0, 0.0), 0.0)
    for kw in ({"min_extent": INF}, {"max_nodes": 1}, {"max_nodes": 2}):
        r = hierarchy.trim_hierarchy(h, **kw)
        assert r.hierarchy.nodes.tolist() == [[0, -1, 0, 1, 0, 0, 0]] and r.stubs == 1 and r.min_extent == INF
        assert r.old_of_new.tolist() == [0] and int((r.new_of_old >= 0).sum()) == 1
        assert torch.equal(bits(r.hierarchy.shs), bits(h.shs[:1]))


def test_budget():
    h, _ = scene2000()
    nd, ext = h.nodes.numpy(), h.boxes[:, 0, 3].numpy()
    values = np.unique(ext[nd[:, 6] > 0])
    for K in (3, 100, 1001, 2500, 3998):
        r = hierarchy.trim_hierarchy(h, max_nodes=K)
        assert r.hierarchy.num_nodes <= K
        if r.min_extent == INF:                          # (the root shares its extent with a child: 5 nodes or 1)
            assert r.hierarchy.num_nodes == 1 and hierarchy.trim_hierarchy(h, float(values[-1])).hierarchy.num_nodes > K
            continue
        at = int(np.searchsorted(values, np.float32(r.min_extent)))
        assert values[at] == np.float32(r.min_extent)
        if at > 0:                                       # the next smaller distinct extent no longer fits
            assert hierarchy.trim_hierarchy(h, float(values[at - 1])).hierarchy.num_nodes > K
        check_layout(r.hierarchy.nodes.numpy())
    assert hierarchy.trim_hierarchy(h, max_nodes=1001).hierarchy.num_nodes == 1001
    with pytest.raises(ValueError):
        hierarchy.trim_hierarchy(h, max_nodes=0)
    with pytest.raises(ValueError):
        hierarchy.trim_hierarchy(h, min_extent=float("nan"))


@functools.lru_cache(maxsize=None)
def merged_case():
    """Three chunks under a new root: depth is not monotone in index order."""
    chunks = []
    for i, P in enumerate((5, 64, 257)):
        sc = synth.make_scene_trained_like(P, CAM, seed=3 + i)
        xyz = sc.means3D + torch.tensor([3.0 * i, -2.0 * i, 0.0])
        chunks.append(hierarchy.build_hierarchy(synth.Scene(xyz.contiguous(), sc.scales, sc.rotations, sc.opacities,
                                                            sc.shs, sc.sh_degree)))
    hm = hierarchy.merge_hierarchies(chunks)
    ext = hm.boxes[:, 0, 3].numpy()
    return hm, float(np.median(ext[hm.nodes[:, 6].numpy() > 0]))


def test_a_merged_hierarchy():
    hm, med = merged_case()
    assert int(hm.nodes[0, 6]) == 3 and (np.diff(hm.nodes[:, 0].numpy()) < 0).any()
    r = hierarchy.trim_hierarchy(hm, med)
    assert 3 < r.hierarchy.num_nodes < hm.num_nodes and r.stubs > 0
    check_layout(r.hierarchy.nodes.numpy())
    v = (0.0, 0.0, -5.0)
    tau = stub_tau(r, v)
    a, b = oracle_cut(hm, tau, v), oracle_cut(r.hierarchy, tau, v)
    assert_cuts_equal_after_mapping(a, b, r.new_of_old.numpy())
    assert np.isin(b[2], r.stub_ids.numpy()).any() and r.exact_for(v, tau)


# ---- rejections ------------------------------------------------------------------------------------------------------
def corruptions():
    """-> [(name, hierarchy, floor, index into TRIM_CHECKS, first offending node)] on copies of the 2 000-leaf scene."""
    h, med = scene2000()
    nd, ext = h.nodes.numpy(), h.boxes[:, 0, 3].numpy()
    out = []
    # closure: p != 0 passes the test and so does one of its children; p's extent drops below the floor, so p's children
    # go while their children stay
    floor = np.float32(med)
    p = next(i for i in range(1, 3999) if nd[i, 6] > 0 and ext[i] >= floor
             and any(nd[c, 6] > 0 and ext[c] >= floor for c in range(nd[i, 5], nd[i, 5] + nd[i, 6])))
    c = clone(h)
    c.boxes[p, 0, 3] = float(floor) / 4
    first = min(int(nd[k, 5]) for k in range(nd[p, 5], nd[p, 5] + nd[p, 6]) if nd[k, 6] > 0 and ext[k] >= floor)
    out.append(("closure", c, float(floor), 3, first))
    c = clone(h)
    c.nodes[1234, 2] += 1
    out.append(("start_is_not_the_index", c, float(floor), 0, 1234))
    k = int(np.nonzero(nd[:, 6] > 0)[0][40])
    c = clone(h)
    c.nodes[k, 6] = 3999
    out.append(("children_range_outside", c, float(floor), 1, k))
    c = clone(h)
    assert not (nd[7, 5] <= 2500 < nd[7, 5] + nd[7, 6])
    c.nodes[2500, 1] = 7
    out.append(("parent_not_claiming", c, float(floor), 2, 2500))
    return out


@pytest.mark.parametrize("case", range(4), ids=["closure", "start", "children", "parent"])
def test_rejections_name_their_node(case):
    name, c, floor, check, node = corruptions()[case]
    with pytest.raises(hierarchy.HierarchyTrimError) as e:
        hierarchy.trim_hierarchy(c, floor)
    assert e.value.check == hierarchy.TRIM_CHECKS[check] and e.value.node == node, (name, e.value.check, e.value.node)
    assert f"node {node}" in str(e.value)
    assert hierarchy.TRIM_CHECKS[:3] == hierarchy.MERGE_CHECKS and len(hierarchy.TRIM_CHECKS) == 4


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
HEADER = open(os.path.join(ROOT, "include", "hgs.h")).read()


def header_struct_size(name):
    """sizeof a typedef'd struct of include/hgs.h whose fields are float / int32_t / int64_t scalars or arrays."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size, align = 0, 1
    for ctype, _, count in re.findall(r"(float|int32_t|int64_t)\s+(\w+)(?:\[(\d+)\])?;", body):
        w = 8 if ctype == "int64_t" else 4
        size = (size + w - 1) // w * w + w * int(count or 1)
        align = max(align, w)
    assert size > 0
    return (size + align - 1) // align * align


def test_the_abi_declares_and_binds_the_three_entries():
    plain = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("hgs_hier_trim_tmp_bytes", "hgs_hier_trim_plan", "hgs_hier_trim_apply"):
        assert re.search(r"\b%s\s*\(" % name, plain), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert re.search(r"#define\s+HGS_ABI_VERSION\s+14\b", HEADER) and _lib.ABI_VERSION == 14
    assert C.sizeof(_lib.HierTrimArgs) == header_struct_size("hgs_hier_trim_args") == 32
    assert C.sizeof(_lib.HierTrimReport) == header_struct_size("hgs_hier_trim_report") == 32
    assert _lib.HierTrimArgs.roi_lo.offset == 8 and _lib.HierTrimArgs.roi_hi.offset == 20
    assert _lib.HierTrimReport.kept.offset == 16 and _lib.HierTrimReport.stubs.offset == 24


def test_tmp_bytes_needs_no_gpu():
    lib = _lib.lib()
    for N in (0, -1, 1 << 31, 1 << 40, -(1 << 40)):
        assert lib.hgs_hier_trim_tmp_bytes(N) == 0, N
    sizes = [lib.hgs_hier_trim_tmp_bytes(N) for N in (1, 256, 257, 2_097_153, (1 << 31) - 1)]
    assert all(b > 0 and b % 256 == 0 for b in sizes)
    assert sizes[0] <= sizes[1] < sizes[2] < sizes[3] < sizes[4], sizes
    # a flag byte per node, a sum per 256 nodes (+ total), a chain word per 8192 sums, the report
    for N, b in zip((1, 256, 257, 2_097_153), sizes):
        nblk = (N + 255) // 256
        assert b >= N + 4 * (nblk + 1) + 8 * ((nblk + 8191) // 8192) + 32, (N, b)


def _view(N, G=None, M=16, base=4096, **at):
    a = {k: base for k in ARRAYS}
    a.update(at)
    return _lib.HierView(N if G is None else G, N, M, 0, *(a[k] for k in ARRAYS))


def test_bad_arguments_fail_before_any_hip_call():
    """(No GPU here: a call that got as far as HIP would return HGS_ERR_HIP, not HGS_ERR_INVALID.)"""
    lib = _lib.lib()
    rep, args = _lib.HierTrimReport(), _lib.HierTrimArgs(1.0, 0)
    nan = _lib.HierTrimArgs(float("nan"), 0)
    nan_roi = _lib.HierTrimArgs(0.0, 1)
    nan_roi.roi_hi[1] = float("nan")
    a = 4096
    plan = [((_view(0), args, a, rep), b"bad sizes"), ((_view(1 << 31), args, a, rep), b"bad sizes"),
            ((_view(5, G=4), args, a, rep), b"bad sizes"), ((_view(5, M=0), args, a, rep), b"bad sizes"),
            ((_view(5, M=65), args, a, rep), b"bad sizes"), ((_view(5, xyz=0), args, a, rep), b"null"),
            ((_view(5), args, None, rep), b"null"), ((_view(5, rots=a + 8), args, a, rep), b"16-byte"),
            ((_view(5, boxes=a + 4), args, a, rep), b"16-byte"), ((_view(5, alpha=a + 2), args, a, rep), b"4-byte"),
            ((_view(5), nan, a, rep), b"NaN"), ((_view(5), nan_roi, a, rep), b"NaN"),
            ((_view(5), args, a + 64, rep), b"256-byte")]
    for (v, ar, tmp, rp), word in plan:
        assert lib.hgs_hier_trim_plan(C.byref(v), C.byref(ar), tmp, C.byref(rp), None, 0) == 1, word
        assert word in lib.hgs_last_error(), (word, lib.hgs_last_error())
    assert lib.hgs_hier_trim_plan(None, C.byref(args), a, C.byref(rep), None, 0) == 1
    assert lib.hgs_hier_trim_plan(C.byref(_view(5)), C.byref(args), a, None, None, 0) == 1
    apply_ = [((_view(5), _view(0), a, a, a), b"bad sizes"), ((_view(5), _view(3, M=4), a, a, a), b"bad sizes"),
              ((_view(5), _view(3, boxes=a + 8), a, a, a), b"16-byte"), ((_view(5), _view(3), a, None, a), b"null"),
              ((_view(5), _view(3), a, a, a + 2), b"4-byte"), ((_view(5), _view(3), a + 128, a, a), b"256-byte"),
              ((_view(5), _view(3), a, a, a), b"no successful hgs_hier_trim_plan")]
    for (vi, vo, tmp, oon, noo), word in apply_:
        assert lib.hgs_hier_trim_apply(C.byref(vi), C.byref(vo), tmp, oon, noo, None, 0) == 1, word
        assert word in lib.hgs_last_error(), (word, lib.hgs_last_error())
    # unaligned-by-4 xyz / alpha / log_scales (and shs: it falls back to 4-byte pieces) pass the alignment checks
    v = _view(5, xyz=a + 4, alpha=a + 4, log_scales=a + 12, shs=a + 4)
    assert lib.hgs_hier_trim_apply(C.byref(v), C.byref(v), a, a, a, None, 0) == 1
    assert b"no successful hgs_hier_trim_plan" in lib.hgs_last_error()


# ---- the command -------------------------------------------------------------------------------------------------------
def test_the_command_parses_its_arguments(capsys):
    p = trim_cmd.parse_args
    assert p(["a.hier", "b.hier", "--min-extent", "0.5"]) == ("a.hier", "b.hier", 0.5, None, None)
    assert p(["--max-nodes", "1001", "a.hier", "b.hier"]) == ("a.hier", "b.hier", 0.0, 1001, None)
    assert p(["a.hier", "--roi", "-2", "-2", "5", "2", "2", "12", "b.hier", "--min-extent", "0"]) == \
        ("a.hier", "b.hier", 0.0, None, ((-2.0, -2.0, 5.0), (2.0, 2.0, 12.0)))
    bad = ([], ["a.hier"], ["a.hier", "b.hier"], ["a.hier", "b.hier", "c.hier", "--min-extent", "1"],
           ["a.hier", "b.hier", "--roi", "0", "0", "0", "1", "1"], ["a.hier", "b.hier", "--roi", "0", "0", "0", "1", "1", "x"],
           ["a.hier", "b.hier", "--min-extent"], ["a.hier", "b.hier", "--min-extent", "big"],
           ["a.hier", "b.hier", "--max-nodes", "0"], ["a.hier", "b.hier", "--max-nodes", "1.5"],
           ["a.hier", "b.hier", "--min-extent", "nan"], ["a.hier", "b.hier", "--frobnicate"])
    for argv in bad:
        assert p(argv) is None, argv
        assert trim_cmd.main(argv) == 2, argv
    assert "usage: python -m hgs.trim_hierarchy" in capsys.readouterr().err
    assert trim_cmd.main(["/nonexistent/in.hier", "out.hier", "--min-extent", "1"]) == 2
    assert "does not exist" in capsys.readouterr().err
