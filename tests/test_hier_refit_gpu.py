"""The HIP box refit (hgs.hierarchy.refit_boxes_gpu, csrc/hier_refit.hip) against the numpy spec hgs.hierarchy.refit_boxes:
through the C ABI on guarded buffers, every interior box and extent equals the numpy union of the DEVICE's own leaf
boxes bit for bit, kept leaves keep their bits, cube and ellipsoid leaves lie within one float32 ulp of the spec (the
double exp is the one operation the two sides may round differently); shapes: node counts on both sides of a wave and a
workgroup, merged roots of 1 to 5 children, a chain 40 levels deep, a node with 70 children, a trimmed hierarchy with
stubs, tails behind the nodes; ``keep`` on device-built and device-merged hierarchies; a hierarchy whose boxes do not
nest is refused by cut_views and cut_to_budget and accepted after the refit; malformed input named and left untouched;
the two commands; a render of a cut of a refit hierarchy against the float64 oracle."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import parity as pa
import ws_guard as wg
from hgs import _lib, hierarchy, synth
from test_hier_merge_gpu import _chunk
from test_hier_refit_cpu import (CORRUPTION_NAMES, MODES, built, chain, corruptions, merged, nested_np, perturbed2000,
                                 stale_boxes, wide)
from test_hier_transform_gpu import _oracle_lod_render
from test_hier_trim_cpu import ARRAYS, CAM, VIEWS, bits, clone, scene2000
from test_hier_trim_gpu import _gpu_cuts, _render

pytestmark = pytest.mark.gpu


def to_dev(h, gpu):
    return hierarchy.Hierarchy(*(getattr(h, k).to(gpu).clone().contiguous() for k in ARRAYS))


def to_host(h):
    return hierarchy.Hierarchy(*(getattr(h, k).cpu() for k in ARRAYS))


def with_tail(h, tail):
    """``tail`` rows behind the node rows that must never be read: every float of them is a NaN."""
    more = lambda t: torch.cat([t, torch.full((tail, *t.shape[1:]), float("nan"))]) if tail else t
    return hierarchy.Hierarchy(more(h.xyz), more(h.shs), more(h.alpha), more(h.log_scales), more(h.rots), h.nodes, h.boxes)


@functools.lru_cache(maxsize=None)
def shape(name):
    kind, _, arg = name.partition(":")
    if kind == "built":
        return built(int(arg))
    if kind == "merged":
        return merged(int(arg))
    if kind == "tail":
        return with_tail(built(257), int(arg))
    if kind == "trimmed":
        h, med = scene2000()
        r = hierarchy.trim_hierarchy(h, med)
        assert r.stubs > 0
        return r.hierarchy
    return {"chain": chain, "wide": wide}[kind]()


SHAPES = [f"built:{P}" for P in (1, 2, 3, 5, 255, 256, 257, 2000)] + [f"merged:{k}" for k in (1, 2, 3, 5)] + \
    ["chain", "wide", "trimmed"] + [f"tail:{t}" for t in (0, 1, 100)]


def ulps(a, b):
    o = lambda x: (lambda i: np.where(i < 0, -(i & 0x7FFFFFFF), i))(np.ascontiguousarray(x).view(np.int32).astype(np.int64))
    return np.abs(o(a) - o(b))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class AbiRun:
    """One hierarchy laid out in guarded allocations, one per array, with a guarded boxes_out and a guarded tmp, for
    hgs_hier_refit."""

    def __init__(self, h, gpu, out_fill=0xFF, tmp_fill=0x00):
        self.h, self.gpu, self.N, self.G = h, gpu, h.num_nodes, int(h.xyz.shape[0])
        self.inputs = {}
        for k in ARRAYS:
            src = getattr(h, k).contiguous().reshape(-1).view(torch.uint8).to(gpu)
            g = wg.guarded(src.numel(), gpu, 0xFF, "in." + k)
            g.body.copy_(src)
            self.inputs[k] = g
        self.out = wg.guarded(self.N * 32, gpu, out_fill, "boxes_out")
        self.out_fill = out_fill
        self.tmp = wg.guarded(_lib.lib().hgs_hier_refit_tmp_bytes(self.N), gpu, tmp_fill, "tmp")
        self.report = _lib.HierRefitReport()

    def call(self, mode, inplace=False):
        v = _lib.HierView(self.G, self.N, 16, 0, *(self.inputs[k].addr for k in ARRAYS))
        out = self.inputs["boxes"].addr if inplace else self.out.addr
        rc = _lib.lib().hgs_hier_refit(C.byref(v), out, hierarchy.REFIT_LEAF_MODES[mode], self.tmp.addr, C.byref(self.report),
                                       _stream(), self.gpu.index or 0)
        wg.check(*self.inputs.values(), self.out, self.tmp)
        return rc

    def boxes(self, inplace=False):
        torch.cuda.synchronize()
        g = self.inputs["boxes"] if inplace else self.out
        return g.view(torch.float32, self.N, 2, 4).cpu().clone()

    def inputs_untouched(self, but=()):
        torch.cuda.synchronize()
        for k in ARRAYS:
            if k not in but:
                src = getattr(self.h, k).contiguous().reshape(-1).view(torch.uint8)
                assert torch.equal(self.inputs[k].body.cpu(), src), f"input {k} was modified"

    def out_untouched(self):
        torch.cuda.synchronize()
        assert bool((self.out.body == self.out_fill).all()), "boxes_out was written"


def check_against_spec(h, got, mode, what):
    """got: the device's boxes [N,2,4] (host) for the host hierarchy ``h``.  -> (largest leaf difference in ulp, number
    of differing leaf coordinates, leaf coordinates)."""
    N = h.num_nodes
    spec = hierarchy.refit_boxes(h, mode).boxes.reshape(N, 2, 4)
    leaf = (h.nodes[:, 6] == 0).numpy()
    g, s = got.numpy(), spec.numpy()
    assert np.array_equal(g[:, 1, 3].view(np.uint32), h.boxes.reshape(N, 2, 4).numpy()[:, 1, 3].view(np.uint32)), (what, "boxes[n,1,3]")
    if mode == "keep":
        assert torch.equal(bits(got[leaf]), bits(h.boxes.reshape(N, 2, 4)[leaf])), (what, "kept leaves")
        u = np.zeros(1, dtype=np.int64)
    else:
        u = np.maximum(ulps(g[leaf, 0, :3], s[leaf, 0, :3]), ulps(g[leaf, 1, :3], s[leaf, 1, :3]))
        assert int(u.max()) <= 1, (what, f"a leaf coordinate {int(u.max())} ulp from the spec")
    # the numpy union of the device's own leaf boxes: the spec in keep mode on them
    mixed = hierarchy.Hierarchy(h.xyz, h.shs, h.alpha, h.log_scales, h.rots, h.nodes, got)
    union = hierarchy.refit_boxes(mixed, "keep").boxes
    assert torch.equal(bits(union), bits(got)), (what, "interior boxes and extents", int((bits(union) != bits(got)).sum()))
    if mode != "keep":                       # a leaf's extent is the largest edge of its rounded box
        e = g[leaf, 1, :3] - g[leaf, 0, :3]
        assert np.array_equal(g[leaf, 0, 3].view(np.uint32), np.maximum(np.maximum(e[:, 0], e[:, 1]), e[:, 2]).view(np.uint32)), what
    assert nested_np(h.nodes.numpy(), g), (what, "the output nests")
    return int(u.max()), int((u > 0).sum()), int(u.size)


@pytest.mark.parametrize("name", SHAPES)
def test_interiors_are_exact_and_leaves_within_one_ulp(gpu, name):
    h = shape(name)
    N = h.num_nodes
    depth = h.nodes[:, 0]
    for mode in MODES:
        run = AbiRun(h, gpu, out_fill=0xFF, tmp_fill=0x00)
        assert run.call(mode) == 0, _lib.lib().hgs_last_error()
        out = run.boxes()
        run.inputs_untouched()
        rep = run.report
        assert list(rep.first_bad) == [-1] * 7 and rep.levels == int(depth.max()) + 1
        assert rep.leaves == int((h.nodes[:, 6] == 0).sum()) and rep.children_sum == N - 1
        worst, differing, coords = check_against_spec(h, out, mode, (name, mode, "out of place"))
        print(f"{name} {mode}: leaves {worst} ulp at most, {differing} of {coords} coordinates differ")
        again = AbiRun(h, gpu, out_fill=0x00, tmp_fill=0xFF)
        assert again.call(mode, inplace=True) == 0, _lib.lib().hgs_last_error()
        again.inputs_untouched(but=("boxes",))
        again.out_untouched()
        assert torch.equal(bits(again.boxes(inplace=True)), bits(out)), (name, mode, "in place differs from out of place")


# ---- the plan kernel's second trip ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (262_145, 300_000))
def test_the_plan_walks_second_trip(gpu, P):
    """The plan kernel's grid is capped at 2048 workgroups of 256 threads: above 524 288 nodes a workgroup goes through
    its loop a second time, with its sums in registers and its depth bins in LDS from the first.  262 145 leaves are
    524 289 nodes (the second trip holds ONE node: the other 255 lanes of that workgroup, and every other workgroup's, have
    none); 300 000 leaves are 599 999 nodes (many workgroups make the trip, the last of them partly filled).  Built on the
    device; waves straddle level boundaries at both sizes.  The numpy spec at 599 999 nodes takes 0.2 s (keep) and 0.3 s
    (cube) on the CPU host these tests were written on, the union of the device's own leaf boxes as much again."""
    d = hierarchy.build_hierarchy_on_device(P, CAM, gpu, seed=3)
    h = to_host(d)
    nodes = h.nodes.numpy()
    N = h.num_nodes
    assert N == 2 * P - 1 and N > 2048 * 256
    first = np.flatnonzero(np.diff(nodes[:, 0])) + 1           # where a level begins (BFS order)
    assert (first % 64 != 0).any(), "no wave straddles a level boundary"
    for mode in ("keep", "cube"):
        rep, stats = _lib.HierRefitReport(), {}
        out = hierarchy.refit_boxes_gpu(d, mode, stats=stats, report=rep)
        assert list(rep.first_bad) == [-1] * 7
        assert rep.levels == stats["levels"] == int(nodes[:, 0].max()) + 1 == np.unique(nodes[:, 0]).size
        assert rep.leaves == stats["leaves"] == int((nodes[:, 6] == 0).sum()) and rep.children_sum == N - 1
        worst, differing, coords = check_against_spec(h, out.boxes.cpu().reshape(N, 2, 4), mode, (P, mode))
        print(f"{P} leaves, {mode}: leaves {worst} ulp at most, {differing} of {coords} coordinates differ")


# ---- keep on what the device built and merged ----------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", (False, True))
def test_keep_returns_the_bits_of_device_built_and_merged_hierarchies(gpu, inplace):
    cam = synth.make_camera(256, 160)
    cases = [hierarchy.build_hierarchy_gpu(synth.make_scene(P, cam, seed=3).to(gpu), gpu) for P in (1, 2, 257, 2000)]
    cases.append(hierarchy.merge_hierarchies_gpu([_chunk(P, seed=3 + i, dev=gpu, shift=(3.0 * i, -2.0 * i))
                                                  for i, P in enumerate((5, 64, 257))], gpu))
    for h in cases:
        before = to_host(h)
        stats = {}
        out = hierarchy.refit_boxes_gpu(h, "keep", inplace=inplace, stats=stats)
        assert (out is h) == inplace and stats["refit_ms"] > 0.0
        assert stats["levels"] == int(before.nodes[:, 0].max()) + 1 and stats["leaves"] == int((before.nodes[:, 6] == 0).sum())
        if not inplace:
            assert out.boxes.data_ptr() != h.boxes.data_ptr()
            assert all(getattr(out, k) is getattr(h, k) for k in ARRAYS[:6]), "the rows are shared, not copied"
        for o in (out, h):
            for k in ARRAYS:
                assert torch.equal(bits(getattr(o, k).cpu()), bits(getattr(before, k))), (k, h.num_nodes)


def test_modes_through_python_and_determinism(gpu):
    h = built(2000)
    d = to_dev(h, gpu)
    for mode in ("cube", "ellipsoid"):
        a = hierarchy.refit_boxes_gpu(d, mode)
        b = hierarchy.refit_boxes_gpu(d, mode)
        s1 = torch.cuda.Stream(gpu)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            c = hierarchy.refit_boxes_gpu(d, mode)
        torch.cuda.synchronize()
        assert torch.equal(bits(a.boxes), bits(b.boxes)) and torch.equal(bits(a.boxes), bits(c.boxes))
        worst, differing, coords = check_against_spec(h, a.boxes.cpu(), mode, mode)
        print(f"2 000 leaves, {mode}: leaves {worst} ulp at most, {differing} of {coords} coordinates differ "
              f"({differing / coords:.2e})")
        for k in ARRAYS:
            assert torch.equal(bits(getattr(d, k).cpu()), bits(getattr(h, k))), f"the input's {k}"
    e, c = hierarchy.refit_boxes_gpu(d, "ellipsoid").boxes, hierarchy.refit_boxes_gpu(d, "cube").boxes
    assert float(e[0, 0, 3]) < float(c[0, 0, 3])
    with pytest.raises(ValueError, match="one of"):
        hierarchy.refit_boxes_gpu(d, "sphere")
    with pytest.raises(ValueError, match="contiguous"):
        hierarchy.refit_boxes_gpu(hierarchy.Hierarchy(d.xyz, d.shs, d.alpha, d.log_scales, d.rots, d.nodes, d.boxes.cpu()))


# ---- nesting unlocks the calls that refuse ---------------------------------------------------------------------------------
def test_a_refit_unlocks_the_cuts_that_need_nested_boxes(gpu):
    from gaussian_hierarchy._C import _boxes_nested
    from hgs.frustum import cull_bounds, cut_to_budget, cut_view, cut_views
    h = stale_boxes(perturbed2000())
    assert not nested_np(h.nodes.numpy(), h.boxes.numpy()), "the precondition: the input does not nest"
    d = to_dev(h, gpu)
    assert not _boxes_nested(d.nodes, d.boxes)
    taus = [0.02, 0.05, 0.01]
    vps = torch.tensor(VIEWS)
    with pytest.raises(ValueError, match="boxes nest"):
        cut_views(d.nodes, d.boxes, None, taus, vps)
    with pytest.raises(ValueError, match="boxes nest"):
        cut_to_budget(d.nodes, d.boxes, None, 500, VIEWS[0])
    assert hierarchy.refit_boxes_gpu(d, "cube", inplace=True) is d
    assert _boxes_nested(d.nodes, d.boxes)
    assert nested_np(h.nodes.numpy(), d.boxes.cpu().numpy())
    bounds = cull_bounds(d.nodes, d.xyz.contiguous(), torch.exp(d.log_scales).contiguous())
    inside = torch.tensor([[0.0, 0.0, 1.0, 1e30]] * 5)
    same = lambda a, b: a.n == b.n and all(torch.equal(bits(x), bits(y)) for x, y in (
        (a.render_indices, b.render_indices), (a.parent_indices, b.parent_indices), (a.node_indices, b.node_indices),
        (a.weights, b.weights), (a.kids, b.kids)))
    cuts = cut_views(d.nodes, d.boxes, bounds, taus, vps, torch.stack([inside] * 3), [1.0] * 3)
    for tau, v, cv in zip(taus, VIEWS, cuts):
        ref = cut_view(d.nodes, d.boxes, bounds, tau, torch.tensor(v), inside, 1.0, nested=False)
        assert ref.n > 1 and same(cv, ref), (tau, v)
    bc = cut_to_budget(d.nodes, d.boxes, bounds, 500, VIEWS[0], inside, cost="entries")
    ref = cut_view(d.nodes, d.boxes, bounds, bc.tau, torch.tensor(VIEWS[0]), inside, 1.0, nested=False)
    assert 50 < bc.n <= 500 and same(bc, ref)


# ---- malformed input -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CORRUPTION_NAMES)), ids=CORRUPTION_NAMES)
def test_a_malformed_hierarchy_is_named_and_nothing_is_written(gpu, case):
    name, c, mode, check, node = corruptions()[case]
    N = c.num_nodes
    b = c.boxes.reshape(N, 2, 4).numpy()
    if mode == "keep":
        lo, hi = b[:, 0, :3], b[:, 1, :3]
    else:
        lo, hi = hierarchy.leaf_boxes(c.xyz.numpy(), c.log_scales.numpy(), c.rots.numpy(), mode)
    first_bad, children_sum = hierarchy.refit_first_bad(c.nodes.numpy(), lo, hi)
    want = hierarchy.REFIT_CHILDREN_SUM if check is None else hierarchy.REFIT_CHECKS[check]
    for inplace in (False, True):
        run = AbiRun(c, gpu)
        assert run.call(mode, inplace=inplace) == 1, (name, inplace)
        msg = _lib.lib().hgs_last_error().decode()
        assert list(run.report.first_bad) == first_bad and run.report.children_sum == children_sum, (name, list(run.report.first_bad))
        assert "nothing was written" in msg and (node is None or f"first offending node {node})" in msg), msg
        assert (check is None and "count_children sums to" in msg) or (check is not None and first_bad[check] == node)
        run.inputs_untouched()
        run.out_untouched()
        d = to_dev(c, gpu)
        with pytest.raises(hierarchy.HierarchyRefitError) as e:
            hierarchy.refit_boxes_gpu(d, mode, inplace=inplace)
        assert e.value.check == want and e.value.node == node, (name, e.value.check, e.value.node)
        for k in ARRAYS:
            assert torch.equal(bits(getattr(d, k).cpu()), bits(getattr(c, k))), f"{k} was modified"


# ---- the commands ------------------------------------------------------------------------------------------------------
def test_refit_command_round_trip(gpu, tmp_path, capsys):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from hgs import refit_hierarchy as cmd
    h = stale_boxes(perturbed2000())
    g = torch.Generator().manual_seed(4)
    tail = lambda t: torch.cat([t, torch.randn(5, *t.shape[1:], generator=g)])
    src, dst, half, again = (str(tmp_path / n) for n in ("in.hier", "out/refit.hier", "out/half.hier", "again.hier"))
    write_hierarchy(src, tail(h.xyz), tail(h.shs), tail(h.alpha).abs(), tail(h.log_scales), tail(h.rots), h.nodes, h.boxes)
    (tmp_path / "anchors.bin").write_bytes(b"anchors")
    h0 = hierarchy.Hierarchy(*load_hierarchy(src))
    assert cmd.main([src, dst]) == 0
    out = capsys.readouterr().out
    assert "N = 3999 nodes on 12 levels, 2000 leaves (--leaf cube)" in out and "5 rows behind the nodes left alone" in out
    assert "the input's boxes did NOT nest, the output's nest" in out and " ms on the device" in out
    assert "anchors.bin" in out and "copied beside the output" in out
    assert (tmp_path / "out" / "anchors.bin").read_bytes() == b"anchors"
    got = hierarchy.Hierarchy(*load_hierarchy(dst))
    assert got.xyz.shape[0] == 4004 and got.num_nodes == 3999
    for k in ARRAYS[:6]:
        assert torch.equal(bits(getattr(got, k)), bits(getattr(h0, k))), k
    want = hierarchy.refit_boxes_gpu(to_dev(h0, gpu), "cube").boxes.cpu()
    assert torch.equal(bits(got.boxes), bits(want))
    check_against_spec(h0, got.boxes, "cube", "the command")
    # a second refit of the output changes nothing; the input nested this time
    assert cmd.main([dst, again, "--leaf", "cube"]) == 0
    assert "the input's boxes nested, the output's nest" in capsys.readouterr().out
    assert open(again, "rb").read() == open(dst, "rb").read()
    # --half: the rows as the half writer stores them, the boxes of the float rows
    assert cmd.main([src, half, "--leaf", "ellipsoid", "--half"]) == 0
    plain_half = str(tmp_path / "plain_half.hier")
    write_hierarchy(plain_half, *(getattr(h0, k) for k in ARRAYS), half=True)
    a, b = hierarchy.Hierarchy(*load_hierarchy(half)), hierarchy.Hierarchy(*load_hierarchy(plain_half))
    for k in ARRAYS[:6]:
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert torch.equal(bits(a.boxes), bits(hierarchy.refit_boxes_gpu(to_dev(h0, gpu), "ellipsoid").boxes.cpu()))
    assert not torch.equal(bits(a.log_scales), bits(h0.log_scales))
    # a hierarchy that fails a check: named, nothing written, exit status 1
    bad = clone(h0)
    bad.xyz[3000, 0] = float("nan")
    assert int(bad.nodes[3000, 6]) == 0
    bad_path, never = str(tmp_path / "bad.hier"), str(tmp_path / "never.hier")
    write_hierarchy(bad_path, *(getattr(bad, k) for k in ARRAYS))
    assert cmd.main([bad_path, never]) == 1
    err = capsys.readouterr().err
    assert "node 3000" in err and "nothing written" in err and not (tmp_path / "never.hier").exists()


def test_transform_command_with_and_without_the_refit_flag(gpu, tmp_path, capsys):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from hgs import transform_hierarchy as cmd
    h = built(2000)
    src, plain, flagged, by_hand = (str(tmp_path / n) for n in ("in.hier", "plain.hier", "flagged.hier", "by_hand.hier"))
    write_hierarchy(src, *(getattr(h, k) for k in ARRAYS))
    h0 = hierarchy.Hierarchy(*load_hierarchy(src))
    argv = ["--scale", "1.7", "--axis-angle", "1", "2", "-0.5", "37", "--translate", "3", "-2", "9"]
    sim = cmd.build_similarity(cmd.parse_args([src, plain] + argv))
    # without the flag: the bytes of a transform written by hand
    assert cmd.main([src, plain] + argv) == 0
    assert "refit" not in capsys.readouterr().out
    moved = hierarchy.transform_hierarchy_gpu(to_dev(h0, gpu), sim)
    write_hierarchy(by_hand, *(getattr(moved, k).cpu() for k in ARRAYS))
    assert open(plain, "rb").read() == open(by_hand, "rb").read()
    # with it: a transform followed by a refit
    assert cmd.main([src, flagged] + argv + ["--refit", "cube"]) == 0
    assert "boxes refit in the new frame (--refit cube)" in capsys.readouterr().out
    got = hierarchy.Hierarchy(*load_hierarchy(flagged))
    want = hierarchy.refit_boxes_gpu(moved, "cube")
    for k in ARRAYS:
        assert torch.equal(bits(getattr(got, k)), bits(getattr(want, k).cpu())), k
    assert float(got.boxes[0, 0, 3]) < float(moved.boxes[0, 0, 3]), "a general rotation grew the boxes; the refit shrank them"


# ---- a render ----------------------------------------------------------------------------------------------------------
def test_a_cut_of_a_refit_hierarchy_renders_as_the_oracle_does(gpu):
    """The in-op LOD path on a cut made from refit boxes against the float64 oracle on the same cut, under the tolerances
    of tests/test_hier_align_gpu.py (1e-5 of the image's maximum, and in l2)."""
    h = perturbed2000()
    d = hierarchy.refit_boxes_gpu(to_dev(h, gpu), "ellipsoid", inplace=True)
    cam = synth.make_camera(64, 48)
    cv, _ = _gpu_cuts(d, 0.2, VIEWS[0], gpu)
    stale, _ = _gpu_cuts(to_dev(h, gpu), 0.2, VIEWS[0], gpu)
    assert 100 < cv.n < 2000 and int(((cv.weights > 0) & (cv.weights < 1)).sum()) > 100
    assert cv.n != stale.n or not torch.equal(cv.node_indices, stale.node_indices), "the refit changed the cut"
    color, radii = _render(gpu, cam, d, cv.render_indices, cv.parent_indices, cv.weights, cv.kids)
    assert float(color.max()) > 0.05 and int((radii > 0).sum()) > 0
    orc = _oracle_lod_render(cam, to_host(d), cv.render_indices.cpu(), cv.parent_indices.cpu(), cv.weights.cpu(), cv.kids.cpu())
    st = pa.err_stats(color.cpu(), orc)
    print(f"render of a refit hierarchy: {cv.n} entries, maxrel {st['maxrel']:.3g}, l2 {st['l2']:.3g}")
    assert st["maxrel"] <= 1e-5 and st["l2"] <= 1e-5, st
