"""The HIP view reach (hgs.hierarchy.view_reach_gpu, csrc/hier_reach.hip) and the keyed trim plan behind
hgs.hierarchy.trim_to_views_gpu (csrc/hier_trim.hip) against their numpy specs, bit for bit: node counts on both sides
of a wave and a workgroup crossed with region counts around the unroll, region counts around the kernel's slab (the
split over the second grid dimension and the integer minimum), few nodes under 20 000 views, 2 097 153 nodes; all seven
output tensors, both maps, the stub count, stub_ids and tau of the trim for three view sets, every SH width and the
budget; guarded buffers through the C ABI; determinism; the contract end to end (for viewpoints inside the view set and
tau' >= tau, GPU cuts and an in-op LOD render of the trimmed hierarchy equal the original's after mapping); the
command's round trip from a cameras.json."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import ws_guard as wg
from hgs import _lib, hierarchy, synth
from test_hier_trim_cpu import ARRAYS, ROI, bits, check_layout, corruptions, scene2000
from test_hier_trim_gpu import (ROWS, AbiRun, _against_spec, _args, _gpu_cuts, _render, _stream, assert_equals_spec, built,
                                to_dev, two_scan_chunks)
from test_trim_to_views_cpu import DOCUMENTED, FLT_MAX, GOLDEN, KS, TAU, view_sets

pytestmark = pytest.mark.gpu

F = np.float32
LEAVES = (1, 2, 128, 129, 257, 2000)          # N = 2 P - 1 = 1, 3, 255, 257, 513, 3999
SLAB = hierarchy.REACH_SLAB
COUNTS = (1, 2, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 1)


def regions_for(h, count, seed=0, whole=False):
    """``count`` seeded regions around and inside the hierarchy, every third a point; from the second on, one touches
    a face of an inner node's box (d2 == 0 on the border).  whole: the last one contains the root box (all FLT_MAX)."""
    bx = h.boxes.cpu().numpy().reshape(-1, 2, 4)
    rng = np.random.default_rng(100 + seed)
    mn, mx = bx[0, 0, :3].astype(np.float64), bx[0, 1, :3].astype(np.float64)
    size = np.maximum(mx - mn, 1.0)
    c = rng.uniform(mn - 1.5 * size, mx + 1.5 * size, size=(count, 3))
    half = rng.uniform(0.0, 0.1, size=(count, 3)) * size
    half[::3] = 0.0
    box = np.concatenate([c - half, c + half], axis=1)
    if count >= 2:
        k = bx.shape[0] // 2
        box[1] = np.concatenate([bx[k, 0, :3] - (1.0, 0.0, 0.0), (bx[k, 0, 0],) + tuple(bx[k, 1, 1:3])])
    if whole:
        box[-1] = np.concatenate([mn - 1.0, mx + 1.0])
    return hierarchy.view_regions(boxes=box)


def assert_reach_equals_spec(got, want):
    assert got.dtype == torch.float32 and got.shape == (want.shape[0],) and got.is_cuda
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- the reach ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("P", LEAVES)
def test_reach_sizes_and_region_counts(gpu, P, count):
    h, _ = built(P)
    regions = regions_for(h, count, seed=P)
    want = hierarchy.view_reach(h, regions)
    stats = {}
    got = hierarchy.view_reach_gpu(to_dev(h, gpu), regions, stats=stats)
    assert_reach_equals_spec(got, want)
    assert stats["reach_ms"] > 0.0
    if count >= 2 and P >= 2:
        assert want[h.num_nodes // 2] == FLT_MAX                      # the region that touches its box


@pytest.mark.parametrize("count", (1, 2, 65, 2 * SLAB + 1))
def test_a_region_around_the_whole_scene_reaches_everything(gpu, count):
    h, _ = built(257)
    regions = regions_for(h, count, seed=7, whole=True)
    want = hierarchy.view_reach(h, regions)
    assert (want == FLT_MAX).all()
    assert_reach_equals_spec(hierarchy.view_reach_gpu(to_dev(h, gpu), regions), want)


@functools.lru_cache(maxsize=None)
def many_views():
    """N = 3 999 under 20 000 regions: (regions, the spec's reach)."""
    h, _ = scene2000()
    regions = regions_for(h, 20_000, seed=9)
    return regions, hierarchy.view_reach(h, regions)


def test_few_nodes_under_many_views(gpu):
    """16 node workgroups: the region range is split over the second grid dimension and folded with the integer min."""
    h, _ = scene2000()
    regions, want = many_views()
    assert 100 < (want == FLT_MAX).sum() < 3999 and np.unique(want).size > 1000
    d = to_dev(h, gpu)
    a = hierarchy.view_reach_gpu(d, regions)
    b = hierarchy.view_reach_gpu(d, regions)
    assert_reach_equals_spec(a, want)
    assert torch.equal(bits(a), bits(b))


def test_reach_of_two_million_nodes(gpu):
    h, host, _ = two_scan_chunks()
    assert h.num_nodes == 2_097_153
    regions = regions_for(host, 5, seed=3)
    want = hierarchy.view_reach(host, regions)
    assert np.unique(want).size > 100_000
    assert_reach_equals_spec(hierarchy.view_reach_gpu(h, regions), want)


def test_nan_and_infinite_boxes_behave_as_in_the_spec(gpu):
    h, _ = built(129)
    h = hierarchy.Hierarchy(*(getattr(h, k).clone() for k in ARRAYS))
    h.boxes[5, 0, 0] = float("nan")
    h.boxes[6, 1, 2] = float("nan")
    h.boxes[8, 1, 1] = float("inf")
    h.boxes[9, 0, 1] = float("-inf")
    h.boxes[10, 0, 3] = float("inf")
    regions = regions_for(h, 65, seed=1)
    k = 11 + int(np.nonzero(hierarchy.view_reach(h, regions)[11:] < FLT_MAX)[0][0])       # a node no region touches
    h.boxes[k, 0, 3] = float("nan")
    want = hierarchy.view_reach(h, regions)
    assert np.isnan(want[k]) and int(np.isnan(want).sum()) == 1
    assert_reach_equals_spec(hierarchy.view_reach_gpu(to_dev(h, gpu), regions), want)


# ---- the trim ------------------------------------------------------------------------------------------------------------
def assert_view_trim_equals_spec(got, want):
    assert_equals_spec(got, want)
    assert got.tau == want.tau and isinstance(got, hierarchy.ViewTrimResult)
    assert np.array_equal(got.regions[0], want.regions[0]) and np.array_equal(got.regions[1], want.regions[1])


@pytest.mark.parametrize("name", list(DOCUMENTED))
def test_trim_equals_the_spec_for_the_three_view_sets(gpu, name):
    h, med = scene2000()
    d = to_dev(h, gpu)
    stats = {}
    got = hierarchy.trim_to_views_gpu(d, view_sets()[name], TAU, stats=stats)
    assert (got.hierarchy.num_nodes, got.stubs) == DOCUMENTED[name]
    assert_view_trim_equals_spec(got, hierarchy.trim_to_views(h, view_sets()[name], TAU))
    assert all(stats[k] > 0.0 for k in ("trim_ms", "reach_ms", "plan_ms", "apply_ms"))
    assert got.hierarchy.nodes.device == gpu and got.covers(view_sets()[name][0][0], TAU)
    kw = dict(tau=TAU / 2, min_extent=med / 2, roi=ROI)
    got = hierarchy.trim_to_views_gpu(d, view_sets()[name], **kw)
    assert 1 < got.hierarchy.num_nodes < 3999
    assert_view_trim_equals_spec(got, hierarchy.trim_to_views(h, view_sets()[name], **kw))


@pytest.mark.parametrize("M", (1, 4, 9, 16))
@pytest.mark.parametrize("P", (1, 2, 129, 257))
def test_trim_sh_widths_and_sizes(gpu, P, M):
    h, _ = built(P, M)
    regions = view_sets()["path"]
    tau = float(np.median(hierarchy.view_reach(h, regions)[h.nodes[:, 6].numpy() > 0])) if P > 1 else TAU
    got = hierarchy.trim_to_views_gpu(to_dev(h, gpu), regions, tau)
    want = hierarchy.trim_to_views(h, regions, tau)
    if P > 2:
        assert 1 < want.hierarchy.num_nodes < h.num_nodes and want.stubs > 0
    assert got.hierarchy.shs.shape[1:] == (M, 3)
    assert_view_trim_equals_spec(got, want)


def test_the_budget_on_the_device_is_the_specs(gpu):
    h, med = scene2000()
    d = to_dev(h, gpu)
    regions = view_sets()["path"]
    for K in KS:
        got = hierarchy.trim_to_views_gpu(d, regions, 0.0, max_nodes=K)
        assert_view_trim_equals_spec(got, hierarchy.trim_to_views(h, regions, 0.0, max_nodes=K))
        assert got.hierarchy.num_nodes <= K
    inside = hierarchy.view_regions(points=[(0.0, 0.0, 10.0)])
    for K in (10, 3000):
        got = hierarchy.trim_to_views_gpu(d, inside, 0.0, max_nodes=K)
        assert_view_trim_equals_spec(got, hierarchy.trim_to_views(h, inside, 0.0, max_nodes=K))
    assert hierarchy.trim_to_views_gpu(d, inside, 0.0, max_nodes=10).hierarchy.num_nodes == 1
    kw = dict(tau=0.05, min_extent=med / 2, roi=ROI, max_nodes=1001)
    got = hierarchy.trim_to_views_gpu(d, regions, **kw)
    assert_view_trim_equals_spec(got, hierarchy.trim_to_views(h, regions, **kw))
    check_layout(got.hierarchy.nodes.cpu().numpy())


def test_boxes_that_do_not_nest_are_refused_on_the_device(gpu):
    name, c, floor, check, _ = corruptions()[0]
    regions = hierarchy.view_regions(points=[(0.0, 0.0, -500.0)])
    tau = floor / 550.0
    with pytest.raises(hierarchy.HierarchyTrimError) as want:
        hierarchy.trim_to_views(c, regions, tau)
    with pytest.raises(hierarchy.HierarchyTrimError) as e:
        hierarchy.trim_to_views_gpu(to_dev(c, gpu), regions, tau)
    assert e.value.check == hierarchy.TRIM_CHECKS[3] == want.value.check and e.value.node == want.value.node
    assert f"node {e.value.node}" in str(e.value) and "hgs.refit_hierarchy" in str(e.value)


# ---- the C ABI on guarded buffers --------------------------------------------------------------------------------------
class KeyedRun(AbiRun):
    """AbiRun with the two new calls: the reach into an exactly sized guarded output with an exactly sized tmp, and the
    keyed plan on that reach."""

    def reach(self, regions, fill):
        lib = _lib.lib()
        lo_, hi_ = regions
        count = lo_.shape[0]
        self.regions = wg.guarded(count * 24, self.gpu, 0xFF, "regions")
        self.regions_src = torch.from_numpy(np.concatenate([lo_, hi_], axis=1)).reshape(-1).view(torch.uint8)
        self.regions.body[:] = self.regions_src.to(self.gpu)
        self.key = wg.guarded(self.N * 4, self.gpu, fill, "reach")
        self.reach_tmp = wg.guarded(lib.hgs_hier_reach_tmp_bytes(self.N, count), self.gpu, fill, "reach tmp")
        return lib.hgs_hier_reach(self.inputs["boxes"].addr, self.N, self.regions.addr, count, self.key.addr,
                                  self.reach_tmp.addr, _stream(), self.gpu.index or 0)

    def plan_keyed(self, args, floor):
        rep = _lib.HierTrimReport()
        rc = _lib.lib().hgs_hier_trim_plan_keyed(C.byref(self.view(self.inputs, self.G, self.N)), C.byref(args),
                                                 self.key.addr, float(floor), self.tmp.addr, C.byref(rep), _stream(),
                                                 self.gpu.index or 0)
        return rc, rep

    def guards(self):
        super().guards()
        wg.check(self.regions, self.key, self.reach_tmp)
        assert torch.equal(self.regions.body.cpu(), self.regions_src), "the regions were modified"


@pytest.mark.parametrize("fill", (0x00, 0xFF))
@pytest.mark.parametrize("P,M,count", [(1, 16, 1), (2, 16, 3), (129, 16, 65), (129, 9, SLAB + 1), (257, 16, 2 * SLAB + 1),
                                       (2000, 16, 65)])
def test_the_calls_stay_in_bounds(gpu, P, M, count, fill):
    """Inputs with a 5-row tail of 0xFF bytes; regions, the reach output and its tmp exactly sized between guards; the
    keyed plan on that reach, then the existing apply into outputs with 2 guard rows of their own."""
    h, _ = built(P, M)
    regions = view_sets()["path"] if count == 65 else regions_for(h, count, seed=P)
    spec_reach = hierarchy.view_reach(h, regions)
    inner = spec_reach[h.nodes[:, 6].numpy() > 0]
    tau = float(np.median(inner)) if inner.size else TAU
    want = hierarchy.trim_to_views(h, regions, tau, roi=ROI if P == 2000 else None)
    run = KeyedRun(h, gpu, tail=5)
    assert run.reach(regions, fill) == 0, _lib.lib().hgs_last_error()
    wg.check(run.key, run.reach_tmp, run.regions)
    assert np.array_equal(run.key.view(torch.int32).cpu().numpy().view(np.uint32), spec_reach.view(np.uint32))
    rc, rep = run.plan_keyed(_args(0.0, ROI if P == 2000 else None), tau)
    assert rc == 0 and list(rep.first_bad) == [-1] * 4, _lib.lib().hgs_last_error()
    assert (rep.kept, rep.stubs) == (want.hierarchy.num_nodes, want.stubs)
    kept = int(rep.kept)
    run.allocate(kept, fill, extra_rows=2)
    assert run.apply(kept, kept + 2) == 0, _lib.lib().hgs_last_error()
    run.guards()
    _against_spec(run, want, *run.result(kept))
    for k in ARRAYS + ("old_of_new",):                      # the rows behind N' still hold the fill
        w = 1 if k == "old_of_new" else run.width[k]
        rest = run.outputs[k].body[kept * w * 4:].cpu()
        assert rest.numel() == 2 * w * 4 and bool((rest == fill).all()), k
    run.inputs_unchanged()


def test_a_nan_key_never_passes_and_a_plain_plan_is_what_it_was(gpu):
    h, med = built(257)
    run = KeyedRun(h, gpu)
    regions = view_sets()["path"]
    assert run.reach(regions, 0xFF) == 0
    torch.cuda.synchronize()
    # a key of NaNs (0xFF bytes): only the root stays, whatever the floor
    run.key.body[:] = 0xFF
    rc, rep = run.plan_keyed(_args(0.0), -1e30)
    assert rc == 0 and (rep.kept, rep.stubs) == (1, 1)
    # the plain plan on the same tmp still gives the extent floor's result, and apply follows either
    want = hierarchy.trim_hierarchy(h, med)
    rc, rep = run.plan(_args(med))
    assert rc == 0 and (rep.kept, rep.stubs) == (want.hierarchy.num_nodes, want.stubs)
    run.allocate(int(rep.kept))
    assert run.apply(int(rep.kept)) == 0
    run.guards()
    _against_spec(run, want, *run.result(int(rep.kept)))
    # a key of +inf with a floor of +inf: the identity
    run.key.view(torch.float32)[:] = float("inf")
    rc, rep = run.plan_keyed(_args(0.0), float("inf"))
    assert rc == 0 and (rep.kept, rep.stubs) == (h.num_nodes, 0)


def test_apply_refuses_a_failed_keyed_plan(gpu):
    name, c, floor, check, _ = corruptions()[0]
    regions = hierarchy.view_regions(points=[(0.0, 0.0, -500.0)])
    with pytest.raises(hierarchy.HierarchyTrimError) as want:
        hierarchy.trim_to_views(c, regions, floor / 550.0)
    run = KeyedRun(c, gpu)
    run.allocate(c.num_nodes)
    assert run.reach(regions, 0x00) == 0
    rc, rep = run.plan_keyed(_args(0.0), floor / 550.0)
    node = want.value.node
    assert rc == 1 and rep.first_bad[3] == node and list(rep.first_bad).count(-1) == 3
    msg = _lib.lib().hgs_last_error()
    assert f"first offending node {node}".encode() in msg and b"hgs.refit_hierarchy" in msg
    assert run.apply(c.num_nodes) == 1 and b"no successful hgs_hier_trim_plan" in _lib.lib().hgs_last_error()
    run.guards()
    assert all(bool((g.body == 0xFF).all()) for g in run.outputs.values())
    run.inputs_unchanged()
    # a successful keyed plan that a failed one follows on the same tmp is forgotten as well
    rc, rep = run.plan_keyed(_args(0.0), float("inf"))
    assert rc == 0 and rep.kept == 1
    rc, _ = run.plan_keyed(_args(0.0), floor / 550.0)
    assert rc == 1 and run.apply(1) == 1


def test_determinism_and_untouched_inputs(gpu):
    h, med = scene2000()
    d = to_dev(h, gpu)
    before = [getattr(d, k).clone() for k in ARRAYS]
    regions = view_sets()["path"]
    kw = dict(tau=TAU, min_extent=med / 4, roi=ROI)
    a = hierarchy.trim_to_views_gpu(d, regions, **kw)
    b = hierarchy.trim_to_views_gpu(d, regions, **kw)
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    many, many_want = many_views()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        c = hierarchy.trim_to_views_gpu(d, regions, **kw)
        r1 = hierarchy.view_reach_gpu(d, many)
    with torch.cuda.stream(s2):
        e = hierarchy.trim_to_views_gpu(d, regions, **kw)
        r2 = hierarchy.view_reach_gpu(d, many)
    torch.cuda.synchronize()
    for other in (b, c, e):
        for k in ARRAYS:
            assert torch.equal(bits(getattr(a.hierarchy, k)), bits(getattr(other.hierarchy, k))), k
        assert torch.equal(a.old_of_new, other.old_of_new) and torch.equal(a.new_of_old, other.new_of_old)
        assert a.stubs == other.stubs and a.tau == other.tau and torch.equal(a.stub_ids, other.stub_ids)
    assert torch.equal(bits(r1), bits(r2))
    assert_reach_equals_spec(r1, many_want)
    for k, t in zip(ARRAYS, before):
        assert torch.equal(bits(getattr(d, k)), bits(t)), f"input {k} was modified"


# ---- the contract end to end ---------------------------------------------------------------------------------------------
def test_cuts_and_render_of_the_hierarchy_trimmed_to_the_path_are_the_originals(gpu):
    h, _ = scene2000()
    d = to_dev(h, gpu)
    r = hierarchy.trim_to_views_gpu(d, view_sets()["path"], TAU)
    assert (r.hierarchy.num_nodes, r.stubs) == DOCUMENTED["path"]
    m = r.new_of_old.long()
    lo_ = view_sets()["path"][0]
    cam = synth.make_camera(64, 48)
    stubs_met = 0
    for v, tau in ((lo_[0], TAU), (lo_[32], TAU), (lo_[64], 2 * TAU)):
        v = tuple(float(x) for x in v)
        tau = F(tau)
        assert r.covers(v, tau) and r.exact_for(v, tau)
        (cv_o, ex_o), (cv_t, ex_t) = _gpu_cuts(d, tau, v, gpu), _gpu_cuts(r.hierarchy, tau, v, gpu)
        assert cv_o.n == cv_t.n > 0
        stubs_met += int(torch.isin(cv_t.node_indices, r.stub_ids).sum())
        for o, t in (((cv_o.render_indices, cv_o.parent_indices, cv_o.node_indices, cv_o.weights, cv_o.kids),
                      (cv_t.render_indices, cv_t.parent_indices, cv_t.node_indices, cv_t.weights, cv_t.kids)), (ex_o, ex_t)):
            for k in range(3):
                assert torch.equal(m[o[k].long()].to(torch.int32), t[k]), k
            assert torch.equal(bits(o[3]), bits(t[3])) and torch.equal(o[4], t[4])
        color_o, radii_o = _render(gpu, cam, d, cv_o.render_indices, cv_o.parent_indices, cv_o.weights, cv_o.kids)
        color_t, radii_t = _render(gpu, cam, r.hierarchy, cv_t.render_indices, cv_t.parent_indices, cv_t.weights, cv_t.kids)
        assert int((radii_o > 0).sum()) > 0
        assert torch.equal(color_o, color_t) and torch.equal(radii_o, radii_t)
    assert stubs_met > 0
    assert not r.exact_for(tuple(float(x) for x in lo_[32]), F(TAU) / F(4))


# ---- the command ---------------------------------------------------------------------------------------------------------
def test_command_round_trip(gpu, tmp_path, capsys):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from hgs import trim_to_views as cmd
    h, _ = scene2000()
    g = torch.Generator().manual_seed(4)
    tail = lambda t: torch.cat([t, torch.randn(5, *t.shape[1:], generator=g)])
    src, dst, again = (str(tmp_path / n) for n in ("in.hier", "out/trimmed.hier", "again.hier"))
    write_hierarchy(src, tail(h.xyz), tail(h.shs), tail(h.alpha).abs(), tail(h.log_scales), tail(h.rots), h.nodes, h.boxes)
    (tmp_path / "exposure.json").write_text("{}")
    cameras = os.path.join(GOLDEN, "cameras_two.json")
    assert cmd.main([src, dst, "--cameras", cameras, "--pad", "0.5", "--tau", str(TAU)]) == 0
    out = capsys.readouterr().out
    regions = cmd.regions_of(cameras, pad=0.5)
    want = hierarchy.trim_to_views(h, regions, TAU)
    n = want.hierarchy.num_nodes
    assert 1 < n < 3999
    assert f"N = 3999 -> {n} nodes ({want.stubs} stubs), 2 view regions, tau 0.2" in out and "5 rows behind" in out
    assert all(w in out for w in ("reach ", "plan ", "apply ", " ms", "read ", "write "))
    assert "exposure.json beside the input is not copied" in out and "anchors.bin" not in out
    h0, got = hierarchy.Hierarchy(*load_hierarchy(src)), hierarchy.Hierarchy(*load_hierarchy(dst))
    assert got.num_nodes == n and got.xyz.shape[0] == n + 5
    for k in ROWS:
        assert torch.equal(bits(getattr(got, k)[:n]), bits(getattr(want.hierarchy, k))), k
        assert torch.equal(bits(getattr(got, k)[n:]), bits(getattr(h0, k)[3999:])), f"tail of {k}"
    assert torch.equal(got.nodes, want.hierarchy.nodes) and torch.equal(bits(got.boxes), bits(want.hierarchy.boxes))
    # the identity: tau = 0 and a region that contains the scene writes the input's bytes
    assert cmd.main([src, again, "--view-box", "-100", "-100", "-100", "100", "100", "100", "--tau", "0"]) == 0
    assert "N = 3999 -> 3999 nodes (0 stubs), 1 view regions" in capsys.readouterr().out
    assert open(again, "rb").read() == open(src, "rb").read()
    # --tau-px: the renderer's formula
    px = str(tmp_path / "px.hier")
    assert cmd.main([src, px, "--cameras", cameras, "--tau-px", "3", "--tanfovx", "0.5", "--width", "100", "--max-nodes", "1001"]) == 0
    want = hierarchy.trim_to_views(h, cmd.regions_of(cameras), cmd.tau_from_pixels(3.0, 0.5, 100.0), max_nodes=1001)
    assert hierarchy.Hierarchy(*load_hierarchy(px)).num_nodes == want.hierarchy.num_nodes <= 1001
    # a hierarchy that fails a check: named, nothing written, exit status 1
    bad = hierarchy.Hierarchy(*(getattr(h0, k).clone() for k in ARRAYS))
    bad.nodes[1234, 2] += 1
    bad_path, never = str(tmp_path / "bad.hier"), str(tmp_path / "never.hier")
    write_hierarchy(bad_path, bad.xyz, bad.shs, bad.alpha, bad.log_scales, bad.rots, bad.nodes, bad.boxes)
    assert cmd.main([bad_path, never, "--cameras", cameras, "--tau", "0.2"]) == 1
    err = capsys.readouterr().err
    assert "node 1234" in err and "nothing written" in err and not (tmp_path / "never.hier").exists()
