"""The device side of every hierarchy tool and every cut on the OTHER tools' outputs (tests/hier_chain_cases.py): nodes
with one child, leaves at mixed depths, k = 3 below the root, rows that went through half precision -- shapes the builder
never makes and no other GPU test feeds.  Every comparison is the tool's own committed contract, imported from its GPU
test: a. every ordered pair (A, B) of the eight tools on four bases, gpu_B(spec_A(base)) against spec_B(spec_A(base));
b. three chains run on the device, every stage against the spec applied to the stage's downloaded input, and the cut of
the last stage against the oracle; c. every cut call on every derived hierarchy against its numpy spec; d. a render
through the in-op LOD path against the python lerp route where almost every entry has one sibling; e. budgeted
residency at a quarter of the rows, float and half rows; f. the commands chained through files."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import budget_cut_spec as bs
import frustum_cases as fc
import frustum_spec as fs
import hier_chain_cases as cc
import parity as pa
from hgs import _lib, hierarchy, residency, synth
from test_budget_cut_gpu import _check as check_budget_cut
from test_cut_views_gpu import _assert_same as assert_same_cut
from test_cut_views_gpu import _call as call_cut_views
from test_cut_views_gpu import _single as single_cut_view
from test_cut_views_gpu import _view as view_of
from test_frustum_gpu import _assert_cut_equals_spec, _planes, _within_4_ulp_of_R
from test_hier_align_gpu import compare_to_spec as align_compare_to_spec
from test_hier_merge_gpu import compare_to_spec as merge_compare_to_spec
from test_hier_prune_cpu import dirty_new
from test_hier_prune_gpu import COUNTS, assert_within_builders_bounds, cov_rows, host
from test_hier_prune_gpu import assert_equals_spec as prune_assert_equals_spec
from test_hier_refit_cpu import nested_np
from test_hier_refit_gpu import check_against_spec as refit_check_against_spec
from test_hier_transform_gpu import assert_bits as transform_assert_bits
from test_hier_trim_cpu import ARRAYS, bits, check_layout
from test_hier_trim_gpu import assert_equals_spec as trim_assert_equals_spec
from test_hier_trim_gpu import to_dev
from test_lod_gpu import in_op_lod_against_python_glue
from test_residency_gpu import _reference as resident_reference
from test_residency_gpu import _render as render_arrays
from test_trim_to_views_gpu import assert_reach_equals_spec, assert_view_trim_equals_spec, regions_for

pytestmark = pytest.mark.gpu

LOD_VIEWPOINTS = ((0.0, 0.0, 0.0), (0.3, -0.1, 5.0), (1.0, 2.0, -4.0))       # tests/test_lod_gpu.py
LOD_TAUS = (0.0, 0.002, 0.01, 0.06, 0.5, 1e4)


# ---- one tool on the device, and its contract -------------------------------------------------------------------------------
def run_on_device(tool, d, args, kw, gpu, inplace=False):
    """``tool`` on the device hierarchy ``d`` with the arguments the spec got (``cc.tool_args`` of the host copy)."""
    if tool in ("prune", "prune_under1"):
        return hierarchy.prune_hierarchy_gpu(d, **kw)
    if tool == "trim":
        return hierarchy.trim_hierarchy_gpu(d, **kw)
    if tool == "trim_to_views":
        return hierarchy.trim_to_views_gpu(d, *args)
    if tool == "refit":
        return hierarchy.refit_boxes_gpu(d, inplace=inplace, **kw)
    if tool == "align":
        return hierarchy.align_hierarchy_gpu(d)                          # in place by definition
    if tool == "transform":
        return hierarchy.transform_hierarchy_gpu(d, *args, inplace=inplace)
    if tool == "merge":
        return hierarchy.merge_hierarchies_gpu([d] + [to_dev(c, gpu) for c in args[0][1:]], gpu)
    raise ValueError(tool)


def hold_against_spec(tool, inp, got, want, what):
    """``got`` (the device's result for the host hierarchy ``inp``) against ``want`` (the spec's) by the tool's contract."""
    N = inp.num_nodes
    if tool in ("prune", "prune_under1"):
        for k in COUNTS:
            assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))
        prune_assert_equals_spec(str(what), host(got.hierarchy), (got.old_of_new.cpu(), got.new_of_old.cpu()), want,
                                 dirty_new(inp, want))
    elif tool == "trim":
        trim_assert_equals_spec(got, want)
    elif tool == "trim_to_views":
        assert_view_trim_equals_spec(got, want)
    elif tool == "refit":
        refit_check_against_spec(inp, got.boxes.cpu().reshape(N, 2, 4), "cube", what)
        for k in ARRAYS[:6]:
            assert torch.equal(bits(getattr(got, k).cpu()), bits(getattr(inp, k))), (what, k)
    elif tool == "align":
        a = host(got)
        align_compare_to_spec(inp, a)
        for k in ("xyz", "shs", "alpha", "nodes", "boxes"):
            assert torch.equal(bits(getattr(a, k)), bits(getattr(inp, k))), (what, k)
    elif tool == "transform":
        transform_assert_bits(got, want, what)
    elif tool == "merge":
        merge_compare_to_spec(got, want)
    else:
        raise ValueError(tool)


def stage(tool, d, gpu, what, inplace=False):
    """One tool on the device hierarchy ``d``: its downloaded input through the spec, the device's result against it.
    -> the device's result; where the spec refuses, the device must refuse with the same check at the same node (None)."""
    inp = host(d)
    args, kw = cc.tool_args(tool, inp)
    try:
        want = cc.spec(tool, inp)
    except hierarchy.HierarchyCheckError as refusal:
        with pytest.raises(type(refusal)) as e:
            run_on_device(tool, d, args, kw, gpu, inplace)
        assert (e.value.check, e.value.node) == (refusal.check, refusal.node), what
        return None
    got = run_on_device(tool, d, args, kw, gpu, inplace)
    hold_against_spec(tool, inp, got, want, what)
    return got


# ---- a. every ordered pair ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", cc.TOOLS)
@pytest.mark.parametrize("a", cc.TOOLS)
@pytest.mark.parametrize("base_name", cc.BASES)
def test_every_tool_on_every_other_tools_output(gpu, base_name, a, b):
    inp = cc.hier(cc.after(a, base_name))
    got = stage(b, to_dev(inp, gpu), gpu, (base_name, a, b))
    refused = (a, b) == ("prune_under1", "prune_under1") and base_name != "merged"      # both children of the root gone
    assert (got is None) == refused
    if got is not None:
        check_layout(cc.hier(got).nodes.cpu().numpy())


# ---- b. chains on the device ---------------------------------------------------------------------------------------------
CHAINS = {"merge_align_transform_prune_trim_refit": ("merge", "align", "transform", "prune", "trim", "refit"),
          "prune_prune_trim_to_views_refit_merge": ("prune", "prune_under1", "trim_to_views", "refit", "merge"),
          "trim_prune_align_transform_in_place_refit": ("trim", "prune", "align", "transform", "refit")}


def device_cut(d, tau, v, gpu):
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    N = d.num_nodes
    ri = torch.zeros(N, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(N, device=gpu); ns = torch.zeros(N, dtype=torch.int32, device=gpu)
    n = expand_to_size(d.nodes, d.boxes, tau, torch.tensor(v).to(gpu), torch.zeros(3), ri, pi, ni)
    get_interpolation_weights(ni[:n], tau, d.nodes, d.boxes, torch.tensor(v), torch.zeros(3), w, ns)
    return tuple(t[:n].cpu().numpy() for t in (ri, pi, ni, w, ns))


def assert_cut_is_the_oracles(got, h, tau, v, what):
    want = cc.oracle_cut(h, tau, v)
    assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
    assert cc.same_cut(got, want), what


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("base_name", cc.BASES)
def test_a_chain_run_entirely_on_the_device(gpu, base_name, chain):
    from gaussian_hierarchy._C import _boxes_nested
    d = to_dev(cc.base(base_name), gpu)
    in_place = chain.endswith("in_place_refit")
    for k, tool in enumerate(CHAINS[chain]):
        got = stage(tool, d, gpu, (base_name, chain, k, tool), inplace=in_place and tool == "transform")
        assert got is not None
        if in_place and tool == "transform":
            assert got is d
        d = cc.hier(got)
        print(base_name, chain, k, tool, d.num_nodes, cc.structure(host(d)))
    h = host(d)
    check_layout(h.nodes.numpy())
    assert _boxes_nested(d.nodes, d.boxes) == nested_np(h.nodes.numpy(), h.boxes.numpy()) is True
    for v in LOD_VIEWPOINTS:
        for tau in LOD_TAUS:
            assert_cut_is_the_oracles(device_cut(d, tau, v, gpu), h, tau, v, (base_name, chain, v, tau))


# ---- c. every cut on every derived hierarchy ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def derived_on_device(kind, base_name):
    """(host hierarchy, the same on the device, its culling balls made there)."""
    from hgs.frustum import cull_bounds
    h = cc.derived(kind, base_name)
    d = to_dev(h, torch.device("cuda", torch.cuda.current_device()))
    return h, d, cull_bounds(d.nodes, d.xyz.contiguous(), torch.exp(d.log_scales).contiguous())


def cut_views_of(h):
    """(camera name, tau) of the cut tests: the three cameras of frustum_cases at its two granularities."""
    return [(name, fc.tau_of(fc.camera(name), px)) for name in "ABC" for px in fc.TAUS_PX]


@pytest.mark.parametrize("kind,base_name", cc.DERIVED)
def test_expand_and_weights_through_the_abi_on_both_routes(gpu, kind, base_name):
    from gaussian_hierarchy._C import _boxes_nested, get_interpolation_weights
    h, d, _ = derived_on_device(kind, base_name)
    N = h.num_nodes
    assert _boxes_nested(d.nodes, d.boxes) and nested_np(h.nodes.numpy(), h.boxes.numpy())
    lib, p = _lib.lib(), _lib.ptr
    ri = torch.zeros(N, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(N, device=gpu); ns = torch.zeros(N, dtype=torch.int32, device=gpu)
    tmp = torch.empty(lib.hgs_expand_tmp_bytes(N), dtype=torch.uint8, device=gpu)
    v3 = lambda t: (C.c_float * 3)(*[float(x) for x in t])
    single = 0
    for v in LOD_VIEWPOINTS + (cc.CUT_VIEW,):
        for tau in LOD_TAUS + (cc.CUT_TAU, 0.2):
            r_o, p_o, n_o, w_o, k_o = cc.oracle_cut(h, tau, v)
            for fn in (lib.hgs_expand_to_size_nested, lib.hgs_expand_to_size):
                cnt = C.c_int32(0)
                ri.fill_(-7); pi.fill_(-7); ni.fill_(-7)
                _lib.check(fn(p(d.nodes), p(d.boxes), N, float(tau), v3(v), v3((0.0, 0.0, 0.0)), p(ri), p(pi), p(ni), N, p(tmp),
                              C.byref(cnt), C.c_void_p(torch.cuda.current_stream().cuda_stream), 0), "expand")
                n = cnt.value
                assert n == len(r_o), (v, tau, n, len(r_o))
                assert np.array_equal(ri[:n].cpu().numpy(), r_o) and np.array_equal(pi[:n].cpu().numpy(), p_o)
                assert np.array_equal(ni[:n].cpu().numpy(), n_o)
            get_interpolation_weights(ni[:n], float(tau), d.nodes, d.boxes, torch.tensor(v), torch.zeros(3), w, ns)
            assert np.array_equal(ns[:n].cpu().numpy(), k_o), (v, tau)
            assert np.array_equal(w[:n].cpu().numpy().view(np.uint32), w_o.view(np.uint32)), (v, tau)
            single += int(((k_o == 1) & (h.nodes.numpy()[n_o, 1] >= 0)).sum())
    assert single > 0 or kind == "merged_of_merged"


@pytest.mark.parametrize("kind,base_name", cc.DERIVED)
def test_bounds_and_the_culled_cut_on_both_routes(gpu, kind, base_name):
    from hgs.frustum import cut_view
    h, d, bounds = derived_on_device(kind, base_name)
    nd, bx = h.nodes.numpy(), h.boxes.numpy().reshape(-1, 2, 4)
    got = bounds.cpu().numpy()
    _within_4_ulp_of_R(got, fs.bounds_spec(nd, h.xyz.numpy(), torch.exp(h.log_scales).numpy()))
    culled = unculled = 0
    for name, tau in cut_views_of(h):
        cam = fc.camera(name)
        planes, rs = _planes(cam)
        spec = fs.cut_view_spec(nd, bx, got, tau, cam.camera_center.numpy(), planes.numpy(), rs)
        culled += spec["n_unculled"] - spec["n"]
        unculled += spec["n"]
        for route in (True, False):
            _assert_cut_equals_spec(cut_view(d.nodes, d.boxes, bounds, tau, cam.camera_center, planes, rs, nested=route), spec)
    assert culled > 0 and unculled > 0


@pytest.mark.parametrize("cost", ["entries", "rows"])
@pytest.mark.parametrize("kind,base_name", cc.DERIVED)
def test_the_budget_cut_below_the_root_in_the_middle_and_above_everything(gpu, kind, base_name, cost):
    h, d, bounds = derived_on_device(kind, base_name)
    nd, bx = h.nodes.numpy(), h.boxes.numpy().reshape(-1, 2, 4)
    case = (nd, bx, d.nodes, d.boxes, None, None, bounds)
    ran = refused = 0
    for name in "AB":
        cam = fc.camera(name)
        vp = cam.camera_center.numpy()
        frustum = _planes(cam)
        for fr in (None, frustum):
            view = bs.View(nd, bx, vp) if fr is None else bs.View(nd, bx, vp, bounds.cpu().numpy(), fr[0].numpy(), fr[1])
            ev = bs.Events(view, cost)
            c_inf, c_all = ev.cost(bs.INF_BITS), ev.cost(bs.bits(0.0))
            seen = {}
            for budget in (c_inf - 1, (c_inf + c_all) // 2, c_all + 10):
                if budget < 0:
                    continue
                r = check_budget_cut(case, cam, fr, view, ev, cost, 0.0, budget, seen)
                ran += r is not None
                refused += r is None
    assert ran > 0 and refused > 0


@pytest.mark.parametrize("kind,base_name", cc.DERIVED)
def test_three_views_in_one_call_are_three_single_cuts(gpu, kind, base_name):
    h, d, bounds = derived_on_device(kind, base_name)
    views = [view_of("A", 3.0), view_of("B", 40.0), view_of("C", 3.0)]
    cuts = call_cut_views(d.nodes, d.boxes, bounds, views)
    assert len(cuts) == 3 and sum(cv.n for cv in cuts) > 0
    for k, (v, cv) in enumerate(zip(views, cuts)):
        assert_same_cut(cv, single_cut_view(d.nodes, d.boxes, bounds, v), f"view {k}")


@pytest.mark.parametrize("kind,base_name", cc.DERIVED)
def test_the_view_reach(gpu, kind, base_name):
    h, d, _ = derived_on_device(kind, base_name)
    for regions in (cc.view_regions(), regions_for(h, 65, seed=3)):
        assert_reach_equals_spec(hierarchy.view_reach_gpu(d, regions), hierarchy.view_reach(h, regions))


# ---- d. one sibling on almost every row, through the rasterizer ------------------------------------------------------------
@pytest.mark.parametrize("weights", ["the_cuts_own", "fractional_under_single_child_parents"])
def test_in_op_lod_on_a_pruned_hierarchy_matches_the_python_glue(gpu, weights):
    """A 256x160 frame of the pruned built(257) through the in-op LOD path and through the python lerp route, forward
    and backward: equal pixels, gradients within 2e-5 of the tensor's maximum, untouched rows exactly zero
    (tests/test_lod_gpu.py: in_op_lod_against_python_glue).  A node under a single-child parent has its parent's box
    (the prune makes a dirty node's box the union of its surviving children's), so the cut's own weight of such an
    entry is always exactly 1; the second case gives these entries the weights 0.25, 0.5, 0.75 in turn, so that the
    k = 1 opacity remap also runs between a node and its parent."""
    h = cc.derived("pruned", "built257")
    cam = synth.make_camera(256, 160)
    d = to_dev(h, gpu)
    N = h.num_nodes
    tau = (2 * (16 + 0.5)) * cam.tanfovx / (0.5 * cam.image_width)
    ri, pi, ni, w, ns = (torch.from_numpy(np.ascontiguousarray(a)) for a in device_cut(d, tau, cam.camera_center.tolist(), gpu))
    assert_cut_is_the_oracles(tuple(t.numpy() for t in (ri, pi, ni, w, ns)), h, tau, cam.camera_center.tolist(), "the cut")
    n = ri.numel()
    under_single = (ns == 1) & (h.nodes[ni.long(), 1] >= 0)
    inside = (w > 0) & (w < 1)
    assert 0 < n < N and int(under_single.sum()) >= 10 and int(inside.sum()) >= 10
    assert bool((w[under_single] == 1.0).all())
    if weights == "fractional_under_single_child_parents":
        w = w.clone()
        w[under_single] = torch.tensor([0.25, 0.5, 0.75]).repeat(n)[:int(under_single.sum())]
        assert int(((w > 0) & (w < 1) & under_single).sum()) == int(under_single.sum())
    full = lambda t, dtype: torch.cat([t.to(dtype), torch.zeros(N - n, dtype=dtype)]).to(gpu)
    in_op_lod_against_python_glue(gpu, h, cam, 0, n, full(ri, torch.int32), full(pi, torch.int32), full(w, torch.float32),
                                  full(ns, torch.int32))


# ---- e. residency at a quarter of the rows ---------------------------------------------------------------------------------
RESIDENCY_VIEWS = (((0.0, 0.0, -5.0), 0.0, 1.0), ((0.0, 0.0, -15.0), 0.0, 0.7), ((-12.0, 0.0, -8.0), 35.0, 0.7),
                   ((20.0, 0.0, -10.0), -40.0, 0.7))          # (camera centre, yaw in degrees, tau): all outside the root box


@pytest.mark.parametrize("rows", ["float", "half"])
def test_budgeted_rendering_of_a_pruned_and_trimmed_merge_is_bit_identical(gpu, rows):
    """tests/test_residency_gpu.py::test_budgeted_rendering_is_bit_identical_and_recycles_slots on the pruned, then
    trimmed merged case at a budget of a quarter of its rows; with half rows the fully resident reference holds
    ``round_rows_to_half`` of the attributes (tests/test_half_rows_gpu.py)."""
    from hgs.residency import BudgetedHierarchy
    h = cc.derived("pruned_trimmed", "merged")
    keys = ("means3D", "shs", "opacities", "scales", "rotations")
    attrs = dict(means3D=h.xyz, shs=h.shs, opacities=h.alpha.abs().reshape(-1, 1), scales=torch.exp(h.log_scales),
                 rotations=torch.nn.functional.normalize(h.rots))
    seen = attrs if rows == "float" else dict(zip(keys, residency.round_rows_to_half(*[attrs[k] for k in keys])))
    full = {k: v.to(gpu).contiguous() for k, v in seen.items()}
    nodes, boxes = h.nodes.to(gpu), h.boxes.to(gpu)
    G = h.num_nodes
    views = [(fc.yaw_camera(c, yaw), tau) for c, yaw, tau in RESIDENCY_VIEWS]
    refs = [resident_reference(gpu, cam, full, nodes, boxes, tau) for cam, tau in views]
    assert max(r[3] for r in refs) <= G // 4 and float(refs[0][0].max()) > 0.0 and int((refs[0][1] > 0).sum()) > 0
    bh = BudgetedHierarchy(*[attrs[k] for k in keys], gpu, budget_rows=G // 4, rows=rows)
    assert bh.B == G // 4
    for rnd in range(2):
        for (cam, tau), (color_ref, radii_ref, n_ref, rows_ref) in zip(views, refs):
            sel = bh.select(nodes, boxes, tau, cam.camera_center.to(gpu), cam.camera_center.cpu())
            assert sel.attempts == 1 and sel.tau == tau and sel.n == n_ref
            assert int(sel.render_indices.min()) >= 0 and int(sel.parent_indices.min()) >= 0
            assert int(sel.render_indices.max()) < bh.B
            arrays = dict(means3D=bh.means3D, shs=bh.shs, opacities=bh.opacities, scales=bh.scales, rotations=bh.rotations)
            color, radii = render_arrays(gpu, cam, arrays, sel.render_indices, sel.parent_indices, sel.weights, sel.kids)
            assert torch.equal(color, color_ref) and torch.equal(radii, radii_ref)
            assert bh.resident_rows <= bh.B
    assert bh.stats["evictions"] > 0 and bh.stats["retries"] == 0


# ---- f. the commands, chained through files ---------------------------------------------------------------------------------
def load(path):
    """A .hier file as a host Hierarchy with boxes [N,2,4]."""
    from gaussian_hierarchy._C import load_hierarchy
    h = hierarchy.Hierarchy(*load_hierarchy(str(path)))
    return hierarchy.Hierarchy(h.xyz, h.shs, h.alpha, h.log_scales, h.rots, h.nodes, h.boxes.reshape(-1, 2, 4))


def test_the_commands_chained_through_files(gpu, tmp_path, capsys):
    """merge, align, transform, prune, trim, refit, compress, each reading the file the one before wrote.  Every file is
    held against the spec applied to the file before it by that tool's contract (as in the chains above), and the last
    float file against the specs chained from the first files' arrays: the node records, both prune maps and the boxes
    up to the refit exactly -- boxes never depend on a recomputed row before it -- and the rows the prune re-merged
    within the builder's bounds and every row within the same 1e-5 on mean, SH, opacity and covariance (aligned and moved
    rows keep their own frames, so the builder's frame conventions are not theirs); the refit's leaf boxes, made from rows that agree to 1e-5, within 1e-4 of the root's extent.  The compressed
    file is the half round trip of the last float file bit for bit (a value on a rounding boundary of half precision
    may go either way between the device's chain and the specs', so it has no row bound of its own)."""
    from gaussian_hierarchy._C import write_hierarchy
    from hgs import (align_hierarchy, compress_hierarchy, merge_hierarchies, prune_hierarchy, refit_hierarchy,
                     transform_hierarchy, trim_hierarchy)
    chunks = [cc.base("built129"), hierarchy.transform_hierarchy(cc.base("built129"), cc.tool_args("transform", None)[0][0])]
    for k, c in enumerate(chunks):
        (tmp_path / "trained" / f"c{k}").mkdir(parents=True)
        write_hierarchy(str(tmp_path / "trained" / f"c{k}" / "hierarchy.hier"), c.xyz, c.shs, c.alpha, c.log_scales, c.rots,
                        c.nodes, c.boxes)
    f = {k: str(tmp_path / k / "h.hier") for k in ("merged", "aligned", "moved", "pruned", "trimmed", "refit", "half")}
    sim = cc.tool_args("transform", None)[0][0]
    text = lambda values: [repr(float(x)) for x in np.asarray(values, dtype=np.float64).reshape(-1)]
    assert merge_hierarchies.main([str(tmp_path / "trained"), "0", str(tmp_path / "chunks"), f["merged"], "c0", "c1"]) == 0
    merged = load(f["merged"])
    merge_compare_to_spec(merged, hierarchy.merge_hierarchies(chunks))
    assert align_hierarchy.main([f["merged"], f["aligned"]]) == 0
    aligned = load(f["aligned"])
    hold_against_spec("align", merged, aligned, None, "align")
    assert transform_hierarchy.main([f["aligned"], f["moved"], "--quat"] + text(sim.q_R) + ["--scale", repr(float(sim.s)),
                                    "--translate"] + text(sim.t)) == 0
    typed = hierarchy.similarity(quat=[float(x) for x in np.asarray(sim.q_R).reshape(-1)], scale=float(sim.s),
                                 translate=[float(x) for x in np.asarray(sim.t).reshape(-1)])
    moved = load(f["moved"])
    transform_assert_bits(moved, hierarchy.transform_hierarchy(aligned, typed), "transform")
    mask = cc.tool_args("prune", moved)[1]["remove"]
    np.save(str(tmp_path / "mask.npy"), mask)
    assert prune_hierarchy.main([f["moved"], f["pruned"], "--mask", str(tmp_path / "mask.npy")]) == 0
    pruned, want = load(f["pruned"]), hierarchy.prune_hierarchy(moved, remove=mask)
    remerged = dirty_new(moved, want)
    prune_assert_equals_spec("prune", pruned, (want.old_of_new, want.new_of_old), want, remerged)
    floor = cc.median_extent(pruned)
    assert trim_hierarchy.main([f["pruned"], f["trimmed"], "--min-extent", repr(floor)]) == 0
    trimmed, want = load(f["trimmed"]), hierarchy.trim_hierarchy(pruned, floor)
    assert want.stubs > 0
    for k in ARRAYS:
        assert torch.equal(bits(getattr(trimmed, k)), bits(getattr(want.hierarchy, k))), k
    assert refit_hierarchy.main([f["trimmed"], f["refit"], "--leaf", "cube"]) == 0
    refit = load(f["refit"])
    hold_against_spec("refit", trimmed, refit, None, "refit")
    assert compress_hierarchy.main([f["refit"], f["half"]]) == 0
    half, want = load(f["half"]), cc.half_round_trip(refit)
    for k in ARRAYS:
        assert torch.equal(bits(getattr(half, k)), bits(getattr(want, k))), ("compress", k)
    capsys.readouterr()
    # the specs chained from the first files' arrays
    s = hierarchy.align_hierarchy(hierarchy.merge_hierarchies(chunks))
    s = hierarchy.transform_hierarchy(s, typed)
    sp = hierarchy.prune_hierarchy(s, remove=cc.tool_args("prune", s)[1]["remove"])
    assert torch.equal(sp.hierarchy.nodes, pruned.nodes) and torch.equal(bits(sp.hierarchy.boxes), bits(pruned.boxes))
    st = hierarchy.trim_hierarchy(sp.hierarchy, cc.median_extent(sp.hierarchy))
    end = hierarchy.refit_boxes(st.hierarchy, "cube")
    assert torch.equal(end.nodes, refit.nodes) and torch.equal(end.nodes, half.nodes)
    remerged = remerged[st.old_of_new.numpy()]                 # the rows the prune computed that the trim kept
    assert 0 < int(remerged.sum()) < end.num_nodes
    assert_within_builders_bounds("the re-merged rows of the last float file against the spec chain", refit, end, remerged)
    stats = {k: pa.err_stats(getattr(refit, k), getattr(end, k)) for k in ("xyz", "shs", "alpha")}       # every row: the
    pa.assert_stats("the last float file against the spec chain", stats, rel_tol=1e-5)                     # same Gaussians
    cg, cw = cov_rows(refit.log_scales, refit.rots), cov_rows(end.log_scales, end.rots)
    rel = np.linalg.norm(cg - cw, axis=(1, 2)) / np.linalg.norm(cw, axis=(1, 2))
    assert float(rel.max()) <= 1e-5, (float(rel.max()), int(rel.argmax()))
    tol = 1e-4 * float(end.boxes[0, 0, 3])
    for got in (refit, half):
        assert float((got.boxes - end.boxes).abs().max()) <= tol, float((got.boxes - end.boxes).abs().max())
