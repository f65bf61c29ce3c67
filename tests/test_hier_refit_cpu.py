"""The box refit (hgs.hierarchy.refit_boxes, the float64 numpy spec of csrc/hier_refit.hip) without a GPU: ``keep`` returns
the bits of built and merged hierarchies, every mode nests (a numpy restatement of lod_nested_kernel's rule), the
ellipsoid box lies inside the cube, a refit after a transform lies inside the transformed boxes (under the five
rotations of the transform tests within one ulp; under signed permutations within the rounding of the inputs), hand-built
shapes, the rejections with their first offender, the C ABI's declarations and host-only checks, the command's argument
parsing.
tests/test_hier_refit_gpu.py holds the HIP call against this spec and imports the cases built here."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

from hgs import _lib, hierarchy, synth
from hgs import refit_hierarchy as refit_cmd
from hgs import transform_hierarchy as transform_cmd
from test_hier_transform_cpu import HALF_TURNS, general, random_rotations
from test_hier_trim_cpu import ARRAYS, CAM, HEADER, bits, clone, header_struct_size, scene2000

MODES = ("keep", "cube", "ellipsoid")
BUILT = (1, 2, 3, 5, 1000)
MERGED = (1, 2, 3, 5)


@functools.lru_cache(maxsize=None)
def built(P):
    """The numpy builder's hierarchy over P leaves (host tensors; do not modify)."""
    return scene2000()[0] if P == 2000 else hierarchy.build_hierarchy(synth.make_scene_trained_like(P, CAM, seed=5))


@functools.lru_cache(maxsize=None)
def merged(k):
    """k chunks of different sizes side by side under a new root (the torch spec of the merger)."""
    chunks = []
    for i, P in enumerate((5, 64, 257, 3, 130)[:k]):
        sc = synth.make_scene_trained_like(P, CAM, seed=3 + i)
        xyz = sc.means3D + torch.tensor([3.0 * i, -2.0 * i, 0.0])
        chunks.append(hierarchy.build_hierarchy(synth.Scene(xyz.contiguous(), sc.scales, sc.rotations, sc.opacities, sc.shs,
                                                            sc.sh_degree)))
    return hierarchy.merge_hierarchies(chunks)


def _hand(nodes, seed):
    """A hierarchy with the given records and random rows; leaf boxes valid (for ``keep``), interior boxes rubbish."""
    nodes = torch.tensor(nodes, dtype=torch.int32)
    N = nodes.shape[0]
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    xyz = 5 * r(N, 3)
    boxes = torch.zeros(N, 2, 4)
    half = r(N, 3).abs() + 0.01
    boxes[:, 0, :3], boxes[:, 1, :3] = xyz - half, xyz + half
    boxes[:, 0, 3] = (boxes[:, 1, :3] - boxes[:, 0, :3]).max(1).values
    boxes[:, 1, 3] = r(N)                                    # the copied word: anything
    interior = nodes[:, 6] > 0
    boxes[interior, :, :3] = 1e6 * r(int(interior.sum()), 2, 3)
    boxes[interior, 0, 3] = -1.0
    return hierarchy.Hierarchy(xyz, r(N, 16, 3), r(N, 1).abs(), 0.5 * r(N, 3) - 1.0, r(N, 4), nodes, boxes)


@functools.lru_cache(maxsize=None)
def chain(depth=40):
    """One node with children per level: node I_d at depth d < ``depth`` has the children 2 d + 1 (the next one) and
    2 d + 2 (a leaf); 2 depth + 1 nodes on depth + 1 levels."""
    rows = [[0, -1, 0, 0, 1, 1, 2]]
    for d in range(depth):
        p = 0 if d == 0 else 2 * d - 1
        last = d == depth - 1
        rows.append([d + 1, p, 2 * d + 1, 1, 0, 0, 0] if last else [d + 1, p, 2 * d + 1, 0, 1, 2 * d + 3, 2])
        rows.append([d + 1, p, 2 * d + 2, 1, 0, 0, 0])
    return _hand(rows, seed=depth)


@functools.lru_cache(maxsize=None)
def wide(k=70):
    """A root with k leaves: wider than a wave, walked by one thread."""
    return _hand([[0, -1, 0, 0, 1, 1, k]] + [[1, 0, 1 + c, 1, 0, 0, 0] for c in range(k)], seed=k)


def nested_np(nodes, boxes):
    """lod_nested_kernel's rule in numpy: every node with a parent lies inside its parent's box, has an extent that is
    not larger, and lo <= hi."""
    nd, b = np.asarray(nodes), np.asarray(boxes, dtype=np.float32).reshape(-1, 2, 4)
    par = nd[:, 1]
    c = np.nonzero(par >= 0)[0]
    if (par[c] >= nd.shape[0]).any():
        return False
    p = par[c]
    ok = (b[c, 0, :3] >= b[p, 0, :3]).all(1) & (b[c, 1, :3] <= b[p, 1, :3]).all(1) & (b[c, 0, 3] <= b[p, 0, 3]) & \
        (b[c, 0, :3] <= b[c, 1, :3]).all(1)
    return bool(ok.all())


def assert_only_boxes_changed(out, h):
    for k in ARRAYS[:6]:
        assert torch.equal(bits(getattr(out, k)), bits(getattr(h, k))), k
    assert out.boxes.shape == h.boxes.shape
    assert torch.equal(bits(out.boxes[:, 1, 3]), bits(h.boxes[:, 1, 3])), "boxes[n,1,3] is copied"


# ---- the spec ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", BUILT)
def test_keep_returns_the_bits_of_builder_output(P):
    h = built(P)
    out = hierarchy.refit_boxes(h, "keep")
    assert torch.equal(bits(out.boxes), bits(h.boxes))
    assert_only_boxes_changed(out, h)


@pytest.mark.parametrize("k", MERGED)
def test_keep_returns_the_bits_of_a_merge(k):
    hm = merged(k)
    assert int(hm.nodes[0, 6]) == k
    out = hierarchy.refit_boxes(hm, "keep")
    assert torch.equal(bits(out.boxes), bits(hm.boxes)), "the merged root included"
    assert_only_boxes_changed(out, hm)


@pytest.mark.parametrize("mode", MODES)
def test_every_mode_nests(mode):
    for h in [built(P) for P in BUILT + (2000,)] + [merged(k) for k in MERGED] + [chain(), wide()]:
        out = hierarchy.refit_boxes(h, mode)
        assert nested_np(out.nodes.numpy(), out.boxes.numpy()), (mode, h.num_nodes)
        assert_only_boxes_changed(out, h)
        b = out.boxes.numpy()
        e = b[:, 1, :3] - b[:, 0, :3]
        inner = h.nodes[:, 6].numpy() > 0
        want = np.maximum(np.maximum(e[:, 0], e[:, 1]), e[:, 2])
        sel = inner if mode == "keep" else np.ones_like(inner)
        assert np.array_equal(b[sel, 0, 3].view(np.uint32), want[sel].view(np.uint32)), "the extent of the rounded box"
    assert not nested_np(chain().nodes.numpy(), chain().boxes.numpy())        # the rule can fail: rubbish interiors


def test_interiors_are_the_union_of_their_children_by_a_plain_loop():
    """The vectorised spec against the rule read literally, on the shapes with a wide node and a deep chain."""
    for h in (merged(5), chain(), wide(), built(5)):
        for mode in ("cube", "keep"):
            out = hierarchy.refit_boxes(h, mode).boxes.numpy()
            nd = h.nodes.numpy()
            for n in np.argsort(-nd[:, 0], kind="stable"):
                if nd[n, 6] > 0:
                    kids = out[nd[n, 5]:nd[n, 5] + nd[n, 6]]
                    assert np.array_equal(out[n, 0, :3], kids[:, 0, :3].min(0)) and np.array_equal(out[n, 1, :3], kids[:, 1, :3].max(0))


def test_a_wide_node_and_a_deep_chain_have_the_shapes_they_claim():
    c, w = chain(), wide()
    assert c.num_nodes == 81 and int(c.nodes[:, 0].max()) == 40 and int((c.nodes[:, 6] > 0).sum()) == 40
    assert all(int(((c.nodes[:, 0] == d) & (c.nodes[:, 6] > 0)).sum()) == 1 for d in range(40))
    assert w.num_nodes == 71 and int(w.nodes[0, 6]) == 70 > 64
    assert int(merged(5).nodes[0, 6]) == 5 and (np.diff(merged(3).nodes[:, 0].numpy()) < 0).any()


def test_the_leaf_rules():
    h = built(1000)
    x, ls, q = h.xyz.numpy(), h.log_scales.numpy(), h.rots.numpy()
    clo, chi = hierarchy.leaf_boxes(x, ls, q, "cube", round32=False)
    elo, ehi = hierarchy.leaf_boxes(x, ls, q, "ellipsoid", round32=False)
    assert clo.dtype == np.float64
    assert (elo >= clo).all() and (ehi <= chi).all(), "the ellipsoid's box lies inside the cube, before rounding"
    assert float((elo - clo).max()) > 1e-3                                      # and is not the cube
    # the cube: 3 times the largest scale around the mean; the ellipsoid of an axis-aligned frame: 3 s_a
    s = np.exp(ls.astype(np.float64))
    assert np.array_equal(chi - clo, (x.astype(np.float64) + 3 * s.max(1, keepdims=True)) - (x.astype(np.float64) - 3 * s.max(1, keepdims=True)))
    ident = np.tile(np.array([2.0, 0.0, 0.0, 0.0], dtype=np.float32), (x.shape[0], 1))      # (norm 2: normalised first)
    ilo, ihi = hierarchy.leaf_boxes(x, ls, ident, "ellipsoid", round32=False)
    assert np.array_equal(ihi, x.astype(np.float64) + 3.0 * np.sqrt(s * s))
    # rounded once, float32 out
    rlo, rhi = hierarchy.leaf_boxes(x, ls, q, "ellipsoid")
    assert rlo.dtype == np.float32 and np.array_equal(rlo, elo.astype(np.float32)) and np.array_equal(rhi, ehi.astype(np.float32))
    with pytest.raises(ValueError):
        hierarchy.leaf_boxes(x, ls, q, "keep")


def five_transforms():
    """The five transforms of tests/test_hier_transform_gpu.py (restated: that module needs nothing from here)."""
    tiny = 1e-4
    return {"identity": hierarchy.similarity(),
            "half_turn_s2": hierarchy.similarity(R=HALF_TURNS[1], scale=2.0),
            "quarter_turn_t": hierarchy.similarity(R=np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), translate=(0.5, -4.0, 2.0)),
            "tiny_rotation": hierarchy.similarity(quat=(np.cos(tiny / 2), 0.0, np.sin(tiny / 2) * 0.6, np.sin(tiny / 2) * 0.8)),
            "general": general()}


def _ulp32(x):
    a = np.abs(np.asarray(x, dtype=np.float32))
    return np.nextafter(a, np.float32(np.inf)) - a


def five_test_rotations():
    """The five rotations under which tests/test_hier_transform_cpu.py::test_nesting_survives_rounding_exactly moves the
    2 000-leaf scene, with its scales and translations (restated: random_rotations(5, 21))."""
    return [hierarchy.similarity(R=R, scale=(0.37, 1.0, 1.7, 12.5, 3.0)[k], translate=(0.1 * k, -7.3, 100.0 * k))
            for k, R in enumerate(random_rotations(5, 21))]


@pytest.mark.parametrize("k", range(5))
def test_a_refit_after_a_transform_lies_inside_the_transformed_boxes(k):
    """sum_b |R_ab| >= 1, so the AABB of the rotated leaf cube contains the axis cube of the moved leaf; unions keep the
    relation.  Slack: one float32 ulp per coordinate.  Under these five rotations the smallest row sum of |R| is 1.34,
    and the refit box lies 770 to 3 400 ulp INSIDE the transformed one at its closest coordinate.  (Where the row sums
    are 1 exactly -- signed permutations -- rounding decides and one ulp is not enough: the next test.)"""
    h, _ = scene2000()
    sim = five_test_rotations()[k]
    assert float(np.abs(sim.R).sum(1).min()) > 1.3
    moved = hierarchy.transform_hierarchy(h, sim)
    refit = hierarchy.refit_boxes(moved, "cube")
    t, r = moved.boxes.numpy(), refit.boxes.numpy()
    over_lo = (t[:, 0, :3] - r[:, 0, :3]) / _ulp32(t[:, 0, :3])          # > 0: the refit box sticks out below
    over_hi = (r[:, 1, :3] - t[:, 1, :3]) / _ulp32(t[:, 1, :3])
    worst = float(max(over_lo.max(), over_hi.max()))
    print(f"rotation {k}: the refit box sticks out of the transformed box by at most {worst:.3g} ulp; root extent "
          f"{t[0, 0, 3]:.6g} -> {r[0, 0, 3]:.6g}")
    assert worst <= 1.0, worst
    assert float(r[0, 0, 3]) < float(t[0, 0, 3]), "the refit shrank what the rotation grew"
    assert nested_np(refit.nodes.numpy(), r)
    assert_only_boxes_changed(refit, moved)


@pytest.mark.parametrize("name", list(five_transforms()))
def test_a_refit_after_a_transform_within_the_rounding_of_its_inputs(name):
    """The containment under the five transforms of tests/test_hier_transform_gpu.py, three of which are signed
    permutations: sum_b |R_ab| = 1 exactly, the two boxes coincide up to rounding, and the refit box sticks out by up to
    114 ulp of a coordinate that happens to lie near 0 (3.8e-6 absolute at coordinates up to 40) -- the builder made its
    box from the scene's float32 scale s, the refit from exp(float32(log s)).  The slack the inputs allow, in absolute
    terms: with C the largest coordinate magnitude
    of either hierarchy: the moved mean x', the builder's box coordinate (scaled and rotated: a factor of at most
    s sum_b |R_ab| <= s sqrt 3 on half an ulp at C / s), the transformed and the refit coordinate are each rounded once,
    half an ulp(C) each at most: (3 + sqrt 3) / 2 < 2.5 ulp(C).  The half-edge: the builder used the scale s_k, the
    refit uses exp(f32(f32(log s_k) + log s)): two roundings of a logarithm of magnitude L = max(|log s_k|,
    |log s_k + log s|), each half an ulp(L) <= L 2^-24, so the half-edge e' = 3 s max_k s_k is off by at most
    e' (2 L 2^-24) (1 + 1e-6).  Unions are 1-Lipschitz in the largest leaf error, so the largest leaf bound holds
    for every node."""
    h, _ = scene2000()
    sim = five_transforms()[name]
    moved = hierarchy.transform_hierarchy(h, sim)
    refit = hierarchy.refit_boxes(moved, "cube")
    t, r = moved.boxes.numpy().astype(np.float64), refit.boxes.numpy().astype(np.float64)
    C_max = max(np.abs(t[:, :, :3]).max(), np.abs(r[:, :, :3]).max(), np.abs(h.boxes.numpy()[:, :, :3]).max() * sim.s)
    ls0, ls1 = h.log_scales.numpy().astype(np.float64), moved.log_scales.numpy().astype(np.float64)
    L = np.maximum(np.abs(ls0), np.abs(ls1)).max(1)
    e = 3.0 * np.exp(ls1).max(1)
    bound = 2.5 * float(_ulp32(C_max)) + float((e * 2 * L * 2.0 ** -24).max()) * (1 + 1e-6)
    worst = max(float((t[:, 0, :3] - r[:, 0, :3]).max()), float((r[:, 1, :3] - t[:, 1, :3]).max()))
    print(f"{name}: sticks out by {worst:.3g}, bound {bound:.3g}")
    assert worst <= bound, (worst, bound)


# ---- a hierarchy train_post.py has been through --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def perturbed2000():
    """The 2 000-leaf scene with its rows moved the way an optimiser moves them (means shifted, log-scales raised, a
    fixed seed) under the boxes it was loaded with: leaves stick out of their stale boxes."""
    h = clone(scene2000()[0])
    g = torch.Generator().manual_seed(19)
    h.xyz += 0.3 * torch.randn(h.xyz.shape, generator=g)
    h.log_scales += 0.4 * torch.rand(h.log_scales.shape, generator=g)
    return h


def stale_boxes(h):
    """What a loader that trusted the rows would see: the stale interior boxes over leaf boxes made from the moved rows
    (``refit`` of the leaves alone) -- the input on which the nested rule must fail."""
    out = clone(h)
    leaf = h.nodes[:, 6] == 0
    lo, hi = hierarchy.leaf_boxes(h.xyz.numpy(), h.log_scales.numpy(), h.rots.numpy(), "cube")
    b = out.boxes.numpy()
    b[leaf.numpy(), 0, :3], b[leaf.numpy(), 1, :3] = lo[leaf.numpy()], hi[leaf.numpy()]
    b[leaf.numpy(), 0, 3] = (hi - lo).max(1)[leaf.numpy()]
    return out


def test_the_perturbed_scene_does_not_nest_until_it_is_refit():
    h = stale_boxes(perturbed2000())
    assert nested_np(scene2000()[0].nodes.numpy(), scene2000()[0].boxes.numpy())
    assert not nested_np(h.nodes.numpy(), h.boxes.numpy())
    for mode in MODES:
        out = hierarchy.refit_boxes(h, mode)
        assert nested_np(out.nodes.numpy(), out.boxes.numpy()), mode
    # the leaves of the moved rows outside the boxes they were loaded with
    p = perturbed2000()
    lo, hi = hierarchy.leaf_boxes(p.xyz.numpy(), p.log_scales.numpy(), p.rots.numpy(), "cube")
    b, leaf = p.boxes.numpy(), p.nodes[:, 6].numpy() == 0
    outside = leaf & ((lo < b[:, 0, :3]).any(1) | (hi > b[:, 1, :3]).any(1))
    assert int(outside.sum()) > 1000


# ---- rejections ------------------------------------------------------------------------------------------------------
def corruptions():
    """-> [(name, hierarchy, leaf mode, index into REFIT_CHECKS or None for the children sum, first offending node)]
    on copies of the 257-leaf hierarchy (N = 513): the aligner's and the trimmer's kinds, then the leaf kinds."""
    h = built_small()
    nd = h.nodes.numpy()
    N = h.num_nodes
    leaf = N - 1
    assert nd[leaf, 6] == 0 and nd[300, 6] == 0 and nd[77, 6] > 0
    out = []

    def add(name, mode, check, node, edit):
        c = clone(h)
        edit(c)
        out.append((name, c, mode, check, node))

    def set_node(n, col, v):
        return lambda c: c.nodes.__setitem__((n, col), v)
    add("depth_off_by_one", "cube", 4, leaf, set_node(leaf, 0, int(nd[leaf, 0]) + 1))
    add("depth_too_large", "cube", 3, leaf, set_node(leaf, 0, 256))
    add("negative_depth", "cube", 3, 300, set_node(300, 0, -3))
    add("parent_out_of_range", "cube", 2, 77, set_node(77, 1, N))
    add("negative_parent", "cube", 2, 77, set_node(77, 1, -1))
    add("second_root", "cube", 5, leaf, set_node(leaf, 0, 0))
    add("interior_depth", "cube", 4, 5, set_node(5, 0, int(nd[5, 0]) + 1))
    add("start_is_not_the_index", "cube", 0, 400, set_node(400, 2, 401))
    k = int(np.nonzero(nd[:, 6] > 0)[0][40])
    add("children_range_outside", "cube", 1, k, set_node(k, 6, N))
    assert not (nd[7, 5] <= 450 < nd[7, 5] + nd[7, 6])
    add("parent_not_claiming", "cube", 2, 450, set_node(450, 1, 7))
    # leaf 300 claims the children of node 77 as well: every check passes, the children sum does not
    add("two_claims", "cube", None, None, lambda c: (c.nodes.__setitem__((300, 5), int(nd[77, 5])),
                                                     c.nodes.__setitem__((300, 6), int(nd[77, 6]))))
    add("nan_mean", "cube", 6, 300, lambda c: c.xyz.__setitem__((300, 1), float("nan")))
    add("nan_mean_ellipsoid", "ellipsoid", 6, 300, lambda c: c.xyz.__setitem__((300, 1), float("nan")))
    add("inf_log_scale", "cube", 6, leaf, lambda c: c.log_scales.__setitem__((leaf, 2), float("inf")))
    add("nan_small_log_scale", "cube", 6, leaf, lambda c: c.log_scales.__setitem__((leaf, int(nd[leaf, 0]) % 3), float("nan")))
    add("huge_log_scale", "ellipsoid", 6, 300, lambda c: c.log_scales.__setitem__((300, 0), 100.0))
    add("zero_quaternion", "ellipsoid", 6, 300, lambda c: c.rots.__setitem__(300, torch.zeros(4)))
    add("kept_box_lo_above_hi", "keep", 6, leaf, lambda c: c.boxes.__setitem__((leaf, 0, 1), float(c.boxes[leaf, 1, 1]) + 1.0))
    add("kept_box_nan", "keep", 6, 300, lambda c: c.boxes.__setitem__((300, 1, 2), float("nan")))
    add("two_leaves", "cube", 6, 300, lambda c: (c.xyz.__setitem__((leaf, 0), float("inf")), c.xyz.__setitem__((300, 0), float("-inf"))))
    return out


@functools.lru_cache(maxsize=None)
def built_small():
    return hierarchy.build_hierarchy(synth.make_scene(257, CAM, seed=3))


CORRUPTION_NAMES = ["depth_off_by_one", "depth_too_large", "negative_depth", "parent_out_of_range", "negative_parent",
                    "second_root", "interior_depth", "start_is_not_the_index", "children_range_outside",
                    "parent_not_claiming", "two_claims", "nan_mean", "nan_mean_ellipsoid", "inf_log_scale",
                    "nan_small_log_scale", "huge_log_scale", "zero_quaternion", "kept_box_lo_above_hi", "kept_box_nan",
                    "two_leaves"]


@pytest.mark.parametrize("case", range(len(CORRUPTION_NAMES)), ids=CORRUPTION_NAMES)
def test_rejections_name_their_node(case):
    name, c, mode, check, node = corruptions()[case]
    assert name == CORRUPTION_NAMES[case]
    with pytest.raises(hierarchy.HierarchyRefitError) as e:
        hierarchy.refit_boxes(c, mode)
    want = hierarchy.REFIT_CHILDREN_SUM if check is None else hierarchy.REFIT_CHECKS[check]
    assert e.value.check == want and e.value.node == node, (name, e.value.check, e.value.node)
    if node is not None:
        assert f"node {node}" in str(e.value)
    # a corruption that another mode does not look at is accepted by it
    if name in ("zero_quaternion", "kept_box_lo_above_hi", "kept_box_nan"):
        hierarchy.refit_boxes(c, "cube")
    assert hierarchy.REFIT_CHECKS[:3] == hierarchy.MERGE_CHECKS and len(hierarchy.REFIT_CHECKS) == 7
    with pytest.raises(ValueError, match="one of"):
        hierarchy.refit_boxes(built(2), "sphere")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_the_abi_declares_and_binds_the_two_entries():
    plain = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("hgs_hier_refit_tmp_bytes", "hgs_hier_refit"):
        assert re.search(r"\b%s\s*\(" % name, plain), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert re.search(r"#define\s+HGS_ABI_VERSION\s+14\b", HEADER) and _lib.ABI_VERSION == 14
    assert C.sizeof(_lib.HierRefitReport) == header_struct_size("hgs_hier_refit_report") == 48
    assert _lib.HierRefitReport.levels.offset == 28 and _lib.HierRefitReport.leaves.offset == 32
    assert _lib.HierRefitReport.children_sum.offset == 40
    assert hierarchy.REFIT_LEAF_MODES == {"keep": _lib.HIER_REFIT_KEEP, "cube": _lib.HIER_REFIT_CUBE, "ellipsoid": _lib.HIER_REFIT_ELLIPSOID}
    assert (_lib.HIER_REFIT_KEEP, _lib.HIER_REFIT_CUBE, _lib.HIER_REFIT_ELLIPSOID) == (0, 1, 2)


def test_tmp_bytes_needs_no_gpu():
    lib = _lib.lib()
    for N in (0, -1, 1 << 31, 1 << 40, -(1 << 40)):
        assert lib.hgs_hier_refit_tmp_bytes(N) == 0, N
    sizes = [lib.hgs_hier_refit_tmp_bytes(N) for N in (1, 256, 257, 2_097_153, (1 << 31) - 1)]
    assert all(b > 0 and b % 256 == 0 for b in sizes)
    assert sizes[0] <= sizes[1] < sizes[2] < sizes[3] < sizes[4], sizes
    # the report block, three words per node (key, sorted key, node id), the sort's own workspace
    for N, b in zip((1, 256, 257, 2_097_153), sizes):
        assert b >= 1072 + 12 * N + lib.hgs_sort_tmp_bytes(N), (N, b)


def _view(N, G=None, M=16, base=4096, **at):
    a = {k: base for k in ARRAYS}
    a.update(at)
    return _lib.HierView(N if G is None else G, N, M, 0, *(a[k] for k in ARRAYS))


def test_bad_arguments_fail_before_any_hip_call():
    """(No GPU here: a call that got as far as HIP would return HGS_ERR_HIP, not HGS_ERR_INVALID.)"""
    lib = _lib.lib()
    rep = _lib.HierRefitReport()
    a = 4096
    far = a + (1 << 20)
    plan = [((_view(0), far, 1, a, rep), b"bad sizes"), ((_view(1 << 31), far + (1 << 40), 1, a, rep), b"bad sizes"),
            ((_view(-3), far, 1, a, rep), b"bad sizes"), ((_view(5, G=4), far, 1, a, rep), b"bad sizes"),
            ((_view(5, M=0), far, 1, a, rep), b"bad sizes"), ((_view(5, xyz=0), far, 1, a, rep), b"null"),
            ((_view(5, boxes=0), far, 1, a, rep), b"null"), ((_view(5), None, 1, a, rep), b"null"),
            ((_view(5), far, 1, None, rep), b"null"), ((_view(5, rots=a + 8), far, 1, a, rep), b"16-byte"),
            ((_view(5, boxes=a + 4), far, 1, a, rep), b"16-byte"), ((_view(5), far + 8, 1, a, rep), b"16-byte"),
            ((_view(5, alpha=a + 2), far, 1, a, rep), b"4-byte"),
            ((_view(5), a + 16, 1, a, rep), b"overlaps"), ((_view(5, boxes=a + 160), a + 16, 1, a, rep), b"overlaps"),
            ((_view(5), a + 5 * 32 - 16, 1, a, rep), b"overlaps"),
            ((_view(5), far, 3, a, rep), b"leaf mode"), ((_view(5), far, -1, a, rep), b"leaf mode"),
            ((_view(5), a, 7, a, rep), b"leaf mode"), ((_view(5), far, 1, a + 64, rep), b"256-byte")]
    for (v, out, mode, tmp, rp), word in plan:
        assert lib.hgs_hier_refit(C.byref(v), out, mode, tmp, C.byref(rp), None, 0) == 1, word
        assert word in lib.hgs_last_error(), (word, lib.hgs_last_error())
    assert lib.hgs_hier_refit(None, far, 1, a, C.byref(rep), None, 0) == 1 and b"null" in lib.hgs_last_error()
    assert lib.hgs_hier_refit(C.byref(_view(5)), far, 1, a, None, None, 0) == 1 and b"null" in lib.hgs_last_error()


def test_the_gpu_function_has_no_cpu_fallback():
    if torch.cuda.is_available():
        return                      # (with a GPU the call runs: tests/test_hier_refit_gpu.py)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hierarchy.refit_boxes_gpu(built(2))


# ---- the commands ------------------------------------------------------------------------------------------------------
def test_the_commands_parse_their_arguments(capsys):
    p = refit_cmd.parse_args
    assert p(["a.hier", "b.hier"]) == ("a.hier", "b.hier", "cube", False)
    assert p(["--leaf", "ellipsoid", "a.hier", "--half", "b.hier"]) == ("a.hier", "b.hier", "ellipsoid", True)
    assert p(["a.hier", "b.hier", "--leaf", "keep"]) == ("a.hier", "b.hier", "keep", False)
    bad = ([], ["a.hier"], ["a.hier", "b.hier", "c.hier"], ["a.hier", "b.hier", "--leaf"], ["a.hier", "b.hier", "--leaf", "sphere"],
           ["a.hier", "b.hier", "--frobnicate"])
    for argv in bad:
        assert p(argv) is None, argv
        assert refit_cmd.main(argv) == 2, argv
    assert "usage: python -m hgs.refit_hierarchy" in capsys.readouterr().err
    assert refit_cmd.main(["/nonexistent/in.hier", "out.hier"]) == 2
    assert "does not exist" in capsys.readouterr().err
    t = transform_cmd.parse_args
    assert t(["a.hier", "b.hier", "--scale", "2"])["refit"] is None
    assert t(["a.hier", "b.hier", "--scale", "2", "--refit", "ellipsoid"])["refit"] == "ellipsoid"
    assert t(["a.hier", "--refit", "keep", "b.hier", "--translate", "1", "2", "3"])["refit"] == "keep"
    for argv in (["a.hier", "b.hier", "--scale", "2", "--refit"], ["a.hier", "b.hier", "--scale", "2", "--refit", "tight"],
                 ["a.hier", "b.hier", "--refit", "cube"]):
        assert t(argv) is None, argv
