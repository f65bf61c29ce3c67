"""GPU parity of the frustum-culled hierarchy cut (csrc/lod_frustum.hip, hgs/frustum.py) against tests/frustum_spec.py:
bounds, the cut on both routes, the contract that a culled cut is the unculled cut minus entries the rasterizer would
not have drawn (bit-identical renders), buffer discipline, and the budgeted viewer path with a frustum."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import frustum_cases as fc
import frustum_spec as fs
import parity as pa
import ws_guard as wg
from hgs import _lib, hierarchy, synth
from oracle import lod_oracle as lo

pytestmark = pytest.mark.gpu

LEAVES = (1, 2, 3, 33, 128, 129, 1000, 20000)       # N = 2 P - 1 nodes: 1, 3, 5, 65, 255, 257, 1999, 39999
ALL_INSIDE = torch.tensor([[0.0, 0.0, 1.0, 1e30]] * 5)


@functools.lru_cache(maxsize=None)
def _case(P):
    """(Hierarchy on the CPU, nodes, boxes, means, activated scales on the GPU, bounds made on the GPU)."""
    from hgs.frustum import cull_bounds
    h = fc.hier20k()[0] if P == 20000 else hierarchy.build_hierarchy(synth.make_scene(P, synth.make_camera(fc.W, fc.H), seed=2))
    dev = torch.device("cuda:0")
    nodes, boxes = h.nodes.to(dev), h.boxes.to(dev)
    means, scales = h.xyz.to(dev).contiguous(), torch.exp(h.log_scales).to(dev).contiguous()
    return h, nodes, boxes, means, scales, cull_bounds(nodes, means, scales)


def _planes(cam, **kw):
    from hgs.frustum import frustum_planes
    return frustum_planes(cam.world_view_transform, cam.tanfovx, cam.tanfovy, fc.W, fc.H, **kw)


def _views():
    return [(name, tau_px) for name in "ABC" for tau_px in fc.TAUS_PX]


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return _np(t).view(np.uint32)


def _assert_cut_equals_spec(cv, spec):
    assert (cv.n, cv.n_unculled) == (spec["n"], spec["n_unculled"])
    assert np.array_equal(_np(cv.render_indices), spec["render_indices"])
    assert np.array_equal(_np(cv.parent_indices), spec["parent_indices"])
    assert np.array_equal(_np(cv.node_indices), spec["node_indices"])
    assert np.array_equal(_np(cv.kids), spec["kids"])
    assert np.array_equal(_bits(cv.weights), spec["weights"].view(np.uint32))


def _within_4_ulp_of_R(got, ref):
    tol = 4 * np.spacing(np.where(np.isfinite(ref[:, 3]), ref[:, 3], np.float32(1.0)))
    assert np.array_equal(np.isinf(got[:, 3]), np.isinf(ref[:, 3]))
    fin = np.isfinite(ref[:, 3])
    err = np.abs(got[fin].astype(np.float64) - ref[fin].astype(np.float64)).max(axis=1)
    assert np.all(err <= tol[fin]), (float(err.max()), int(np.argmax(err - tol[fin])))


@pytest.mark.parametrize("P", LEAVES)
def test_bounds_match_the_spec(gpu, P):
    h, nodes, boxes, means, scales, bounds = _case(P)
    ref = fs.bounds_spec(h.nodes.numpy(), _np(means), _np(scales))
    got = _np(bounds)
    assert got.shape == (2 * P - 1, 4)
    _within_4_ulp_of_R(got, ref)


def test_bounds_of_nodes_with_several_rows_and_rows_outside_the_arrays(gpu):
    from hgs.frustum import cull_bounds
    nodes, means, scales = fc.multi_row_case()
    d = lambda a: torch.from_numpy(a).to(gpu)
    got = _np(cull_bounds(d(nodes), d(means), d(scales)))
    _within_4_ulp_of_R(got, fs.bounds_spec(nodes, means, scales))
    assert np.isinf(got[4, 3]) and np.all(got[4, :3] == 0)          # the node without rows
    for col, val, who in ((2, 9, 3), (3, 10, 1), (2, -1, 2)):         # rows [9, 13), [3, 13) and [-1, 0) of 12
        bad = nodes.copy()
        bad[who, col] = val
        with pytest.raises(_lib.HgsError, match=rf"node {who} lie outside \[0, 12\)"):
            cull_bounds(d(bad), d(means), d(scales))
    assert np.array_equal(_np(cull_bounds(d(nodes), d(means), d(scales))), got)     # and the next call is fine


@pytest.mark.parametrize("P", LEAVES)
def test_cut_matches_the_spec_on_both_routes(gpu, P):
    """GPU-made bounds fed to the spec: counts, the three index arrays and the sibling counts exactly; the weights bit for
    bit against the spec AND against hgs_interp_weights on the same node list; single-pass and level routes agree."""
    from gaussian_hierarchy._C import get_interpolation_weights
    from hgs.frustum import cut_view
    h, nodes, boxes, means, scales, bounds = _case(P)
    nodes_h, boxes_h, bounds_h = h.nodes.numpy(), h.boxes.numpy(), _np(bounds)
    N = nodes_h.shape[0]
    w_ref = torch.zeros(N, device=gpu); k_ref = torch.zeros(N, dtype=torch.int32, device=gpu)
    culled_something = False
    for name, tau_px in _views() + [("B", -0.5), ("C", 1e6)]:         # tau = 0: every leaf; huge: the root alone
        cam = fc.camera(name)
        tau = fc.tau_of(cam, tau_px)
        planes, rs = _planes(cam)
        vp = cam.camera_center
        if P == 20000 and tau_px in fc.TAUS_PX:                       # the unculled cut is shared with the CPU tests
            u = fc.unculled(name, tau_px)
            keep = ~fs.culled_spec(nodes_h, bounds_h, u["ni"], planes.numpy(), rs)
            spec = dict(n=int(keep.sum()), n_unculled=len(u["r"]), render_indices=u["r"][keep],
                        parent_indices=u["p"][keep], node_indices=u["ni"][keep], weights=u["w"][keep], kids=u["kids"][keep])
        else:
            spec = fs.cut_view_spec(nodes_h, boxes_h, bounds_h, tau, vp.numpy(), planes.numpy(), rs)
        culled_something |= spec["n"] < spec["n_unculled"]
        cuts = [cut_view(nodes, boxes, bounds, tau, vp, planes, rs, nested=route) for route in (True, False, None)]
        for cv in cuts:
            _assert_cut_equals_spec(cv, spec)
        if spec["n"]:
            get_interpolation_weights(cuts[0].node_indices, tau, nodes, boxes, vp, torch.zeros(3), w_ref, k_ref)
            assert np.array_equal(_bits(cuts[0].weights), _bits(w_ref[:spec["n"]]))
            assert torch.equal(cuts[0].kids, k_ref[:spec["n"]])
    assert culled_something or P < 1000


def test_non_nested_hierarchy_takes_the_level_route(gpu):
    """A deep interior node with an extent larger than its parent's: its size is above every granularity, so the
    single-pass rule ("my parent is too coarse") reaches its children even where an ancestor further up was fine enough
    and drawn whole.  The nesting check says so, the default route is the level-by-level one and gives the spec's cut;
    the single-pass route, forced, does not at 40 px -- the two routes are really different code."""
    from gaussian_hierarchy import _C as gh
    from hgs.frustum import cut_view
    h, nodes, boxes, means, scales, bounds = _case(1000)
    boxes = boxes.clone()
    x = int(h.nodes[-1, 1])                               # the last leaf's parent: far away, below every coarse cut
    boxes[x, 0, 3] = 1e6
    hb = h.boxes.clone(); hb[x, 0, 3] = 1e6
    assert gh._boxes_nested(nodes, _case(1000)[2]) and not gh._boxes_nested(nodes, boxes)
    differs = {}
    for name, tau_px in _views():
        cam = fc.camera(name)
        tau = fc.tau_of(cam, tau_px)
        planes, rs = _planes(cam)
        spec = fs.cut_view_spec(h.nodes.numpy(), hb.numpy(), _np(bounds), tau, cam.camera_center.numpy(), planes.numpy(), rs)
        _assert_cut_equals_spec(cut_view(nodes, boxes, bounds, tau, cam.camera_center, planes, rs), spec)
        _assert_cut_equals_spec(cut_view(nodes, boxes, bounds, tau, cam.camera_center, planes, rs, nested=False), spec)
        single = cut_view(nodes, boxes, bounds, tau, cam.camera_center, planes, rs, nested=True)
        differs[name, tau_px] = single.n_unculled - spec["n_unculled"]
    print("single-pass minus level route, unculled entries:", differs)
    assert all(differs[name, 40.0] > 0 for name in "ABC"), differs


@pytest.mark.parametrize("P", [3, 129, 20000])
def test_planes_that_contain_everything_give_expand_to_size(gpu, P):
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    from hgs.frustum import cut_view
    h, nodes, boxes, means, scales, bounds = _case(P)
    N = nodes.shape[0]
    ri = torch.zeros(N, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(N, device=gpu); ns = torch.zeros(N, dtype=torch.int32, device=gpu)
    for name, tau_px in _views():
        cam = fc.camera(name)
        tau = fc.tau_of(cam, tau_px)
        n = expand_to_size(nodes, boxes, tau, cam.camera_center.to(gpu), torch.zeros(3), ri, pi, ni)
        get_interpolation_weights(ni[:n], tau, nodes, boxes, cam.camera_center, torch.zeros(3), w, ns)
        for route in (True, False):
            cv = cut_view(nodes, boxes, bounds, tau, cam.camera_center, ALL_INSIDE, 1.4, nested=route)
            assert cv.n == cv.n_unculled == n
            assert torch.equal(cv.render_indices, ri[:n]) and torch.equal(cv.parent_indices, pi[:n])
            assert torch.equal(cv.node_indices, ni[:n]) and torch.equal(cv.kids, ns[:n])
            assert np.array_equal(_bits(cv.weights), _bits(w[:n]))


@pytest.mark.parametrize("P", [1, 129, 20000])
def test_camera_facing_away_gets_an_empty_cut(gpu, P):
    """Every ball is behind the near plane: n = 0 with n_unculled > 0, no error from an empty launch, outputs untouched,
    and the next call works."""
    from hgs.frustum import CutBuffers, cut_view
    h, nodes, boxes, means, scales, bounds = _case(P)
    cam = fc.yaw_camera((0.0, 0.0, -50.0), 180.0)
    planes, rs = _planes(cam)
    out = CutBuffers(nodes.shape[0], gpu)
    for t in (out.ri, out.pi, out.ni, out.ns):
        t.fill_(-7)
    out.w.fill_(-7.0)
    for route in (True, False):
        cv = cut_view(nodes, boxes, bounds, fc.tau_of(cam, 3.0), cam.camera_center, planes, rs, out=out, nested=route)
        assert cv.n == 0 and cv.n_unculled > 0 and cv.render_indices.numel() == 0 and cv.weights.numel() == 0
        torch.cuda.synchronize()
        assert bool((out.ri == -7).all()) and bool((out.ns == -7).all()) and bool((out.w == -7.0).all())
    assert cut_view(nodes, boxes, bounds, fc.tau_of(cam, 3.0), cam.camera_center, ALL_INSIDE, rs, out=out).n == cv.n_unculled


def test_capacity_overflow_names_the_count_and_bad_arguments_are_refused(gpu):
    from hgs.frustum import CutBuffers, cut_view
    h, nodes, boxes, means, scales, bounds = _case(1000)
    cam = fc.camera("A")
    tau = fc.tau_of(cam, 3.0)
    planes, rs = _planes(cam)
    full = cut_view(nodes, boxes, bounds, tau, cam.camera_center, planes, rs)
    assert full.n > 10
    for route in (True, False):
        small = CutBuffers(10, gpu)
        small.ri.fill_(-7)
        with pytest.raises(_lib.HgsError, match=rf"{full.n} entries exceed the output capacity 10"):
            cut_view(nodes, boxes, bounds, tau, cam.camera_center, planes, rs, out=small, nested=route)
    exact = CutBuffers(full.n, gpu)
    assert cut_view(nodes, boxes, bounds, tau, cam.camera_center, planes, rs, out=exact).n == full.n
    assert torch.equal(exact.ri, full.render_indices)
    args = dict(nodes=nodes, boxes=boxes, bounds=bounds, tau=tau, viewpoint=cam.camera_center, planes=planes, radius_scale=rs)
    for key, bad in (("nodes", nodes.cpu()), ("boxes", boxes.cpu()), ("bounds", bounds.cpu()), ("nodes", nodes.long()),
                     ("boxes", boxes.double()), ("bounds", bounds.half()), ("nodes", nodes[:, :6]), ("boxes", boxes[:-1]),
                     ("bounds", bounds[:, :3]), ("bounds", bounds[:-1]), ("nodes", nodes.t().contiguous().t()),
                     ("bounds", bounds.t().contiguous().t()), ("planes", planes[:4]), ("viewpoint", torch.zeros(4))):
        with pytest.raises(ValueError):
            cut_view(**dict(args, **{key: bad}))
    odd = CutBuffers(full.n, gpu)
    odd.w = odd.w.double()
    with pytest.raises(ValueError):
        cut_view(**args, out=odd)
    # the C ABI checks its arguments before any HIP call
    lib = _lib.lib()
    n, n_all = C.c_int32(5), C.c_int32(5)
    assert lib.hgs_lod_cut_view(None, None, None, 0, 0.1, None, None, 1.0, 1, None, None, None, None, None, 0, None,
                                C.byref(n), C.byref(n_all), None, 0) == 0 and (n.value, n_all.value) == (0, 0)
    assert lib.hgs_lod_cut_view(None, None, None, 7, 0.1, None, None, 1.0, 1, None, None, None, None, None, 0, None,
                                C.byref(n), C.byref(n_all), None, 0) != 0
    assert b"null" in lib.hgs_last_error()
    assert lib.hgs_hier_cull_bounds(None, 7, None, None, 7, None, None, 0) != 0 and b"null" in lib.hgs_last_error()
    assert lib.hgs_hier_cull_bounds(None, 0, None, None, 0, None, None, 0) == 0


@pytest.mark.parametrize("P,route", [(129, True), (129, False), (1000, True), (1000, False)])
def test_outputs_and_workspace_stay_inside_their_bytes(gpu, P, route):
    """Every output at exactly the cut's size and the workspace at exactly hgs_lod_cut_view_tmp_bytes, each between two
    guards, free bytes filled once with 0x00 and once with 0xFF: intact guards, bit-equal results."""
    from hgs.frustum import cut_view
    h, nodes, boxes, means, scales, bounds = _case(P)
    cam = fc.camera("C")
    tau = fc.tau_of(cam, 3.0)
    planes, rs = _planes(cam)
    ref = cut_view(nodes, boxes, bounds, tau, cam.camera_center, planes, rs)
    assert 0 < ref.n < ref.n_unculled
    lib, N, p = _lib.lib(), int(nodes.shape[0]), _lib.ptr
    vp = (C.c_float * 3)(*[float(x) for x in cam.camera_center])
    pl = (C.c_float * 20)(*[float(x) for x in planes.reshape(-1)])
    results = []
    for fill in (0x00, 0xFF):
        gs = {k: wg.guarded(4 * ref.n, gpu, fill, k) for k in ("ri", "pi", "ni", "w", "ns")}
        gs["tmp"] = wg.guarded(lib.hgs_lod_cut_view_tmp_bytes(N), gpu, fill, "tmp")
        gs["bounds"] = wg.guarded(16 * N, gpu, fill, "bounds")
        b = gs["bounds"].view(torch.float32, N, 4)
        _lib.check(lib.hgs_hier_cull_bounds(p(nodes), N, p(means), p(scales), int(means.shape[0]), p(b),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream), 0), "bounds")
        n, n_all = C.c_int32(0), C.c_int32(0)
        a = lambda k: C.c_void_p(gs[k].addr)
        _lib.check(lib.hgs_lod_cut_view(p(nodes), p(boxes), p(b), N, float(tau), vp, pl, float(rs), int(route), a("ri"),
                                        a("pi"), a("ni"), a("w"), a("ns"), ref.n, a("tmp"), C.byref(n), C.byref(n_all),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream), 0), "cut_view")
        wg.check(*gs.values())
        assert (n.value, n_all.value) == (ref.n, ref.n_unculled)
        results.append({k: gs[k].body.clone() for k in ("ri", "pi", "ni", "w", "ns", "bounds")})
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k
    for k, t in (("ri", ref.render_indices), ("pi", ref.parent_indices), ("ni", ref.node_indices), ("w", ref.weights),
                 ("ns", ref.kids), ("bounds", bounds)):
        assert torch.equal(results[0][k], t.contiguous().view(-1).view(torch.uint8)), k


def test_two_calls_and_two_streams_give_the_same_bits(gpu):
    from hgs.frustum import cull_bounds, cut_view
    h, nodes, boxes, means, scales, bounds = _case(20000)
    assert torch.equal(cull_bounds(nodes, means, scales), bounds)
    cam = fc.camera("B")
    tau = fc.tau_of(cam, 3.0)
    planes, rs = _planes(cam)
    ref = cut_view(nodes, boxes, bounds, tau, cam.camera_center, planes, rs)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=gpu) for _ in range(2)]
    cuts = []
    for rep in range(2):
        for s in streams:
            with torch.cuda.stream(s):
                cuts.append(cut_view(nodes, boxes, bounds, tau, cam.camera_center, planes, rs, nested=bool(rep)))
    torch.cuda.synchronize()
    for cv in cuts:
        assert (cv.n, cv.n_unculled) == (ref.n, ref.n_unculled)
        for a, b in ((cv.render_indices, ref.render_indices), (cv.parent_indices, ref.parent_indices),
                     (cv.node_indices, ref.node_indices), (cv.kids, ref.kids)):
            assert torch.equal(a, b)
        assert np.array_equal(_bits(cv.weights), _bits(ref.weights))


# ---- rendering ---------------------------------------------------------------------------------------------------------
def _attrs(gpu=None):
    h, full, _ = fc.hier20k()
    a = dict(means3D=full["xyz"], shs=full["features"], opacities=full["opacity"].reshape(-1, 1), scales=full["scaling"],
             rotations=full["rotation"])
    return a if gpu is None else {k: v.to(gpu).contiguous() for k, v in a.items()}


def _render(gpu, cam, arrays, ri, pi, w, ns):
    """The in-op LOD path: full (or slot) arrays plus the cut's index tensors (tests/test_lod_gpu.py shows the call)."""
    import diff_gaussian_rasterization as dgr
    kw = pa.settings_kwargs(cam, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=w, num_node_kids=ns)
    kw.update(render_indices=ri.contiguous(), parent_indices=pi.contiguous())
    G = arrays["means3D"].shape[0]
    with torch.no_grad():
        color, radii, _ = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw))(
            means3D=arrays["means3D"], means2D=torch.zeros(G, 3, device=gpu), shs=arrays["shs"],
            opacities=arrays["opacities"], scales=arrays["scales"], rotations=arrays["rotations"])
    return color, radii


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("tau_px", fc.TAUS_PX)
def test_culled_render_is_the_unculled_render(gpu, name, tau_px):
    """Every entry the cull dropped has radii == 0 in the unculled render; the two images and the kept entries' radii are
    bit-identical."""
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    from hgs.frustum import cut_view
    h, nodes, boxes, means, scales, bounds = _case(20000)
    full = _attrs(gpu)
    N = nodes.shape[0]
    cam = fc.camera(name)
    tau = fc.tau_of(cam, tau_px)
    ri = torch.zeros(N, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(N, device=gpu); ns = torch.zeros(N, dtype=torch.int32, device=gpu)
    n = expand_to_size(nodes, boxes, tau, cam.camera_center.to(gpu), torch.zeros(3), ri, pi, ni)
    get_interpolation_weights(ni[:n], tau, nodes, boxes, cam.camera_center, torch.zeros(3), w, ns)
    color_u, radii_u = _render(gpu, cam, full, ri[:n], pi[:n], w[:n], ns[:n])
    planes, rs = _planes(cam)
    cv = cut_view(nodes, boxes, bounds, tau, cam.camera_center, planes, rs)
    assert cv.n_unculled == n and 0 < cv.n < n
    kept = torch.isin(ri[:n], cv.render_indices)
    assert int(kept.sum()) == cv.n and torch.equal(ri[:n][kept], cv.render_indices)
    assert int((radii_u[~kept] > 0).sum()) == 0, "the cull dropped an entry that the rasterizer draws"
    assert int((radii_u > 0).sum()) > 0
    color_c, radii_c = _render(gpu, cam, full, cv.render_indices, cv.parent_indices, cv.weights, cv.kids)
    assert torch.equal(radii_c, radii_u[kept])
    assert torch.equal(color_c, color_u)
    print(f"{name} tau {tau_px}: kept {cv.n} of {n}, drawn {int((radii_u > 0).sum())}")


# ---- the budgeted viewer path ------------------------------------------------------------------------------------------
def _budgeted(gpu, budget_rows):
    from hgs.residency import BudgetedHierarchy
    a = _attrs()
    return BudgetedHierarchy(a["means3D"], a["shs"], a["opacities"], a["scales"], a["rotations"], gpu, budget_rows=budget_rows)


def _slot_arrays(bh):
    return dict(means3D=bh.means3D, shs=bh.shs, opacities=bh.opacities, scales=bh.scales, rotations=bh.rotations)


def _select(bh, nodes, boxes, tau, cam, frustum):
    kw = {} if frustum is None else dict(frustum=frustum)
    return bh.select(nodes, boxes, tau, cam.camera_center.to(bh.dev), cam.camera_center.cpu(), **kw)


def test_frustum_select_renders_like_the_plain_select(gpu):
    """A budget that holds everything: nothing is regulated, and the frustum path's image equals the plain path's, bit
    for bit, from fewer entries; stats count what was culled; without the argument nothing changes."""
    h, nodes, boxes, means, scales, bounds = _case(20000)
    G = nodes.shape[0]
    plain, frus = _budgeted(gpu, G), _budgeted(gpu, G)
    culled = 0
    for name in "ABC":
        cam = fc.camera(name)
        tau = fc.tau_of(cam, 3.0)
        sp = _select(plain, nodes, boxes, tau, cam, None)
        sf = _select(frus, nodes, boxes, tau, cam, _planes(cam))
        assert sp.attempts == sf.attempts == 1 and sp.tau == sf.tau == tau and 0 < sf.n < sp.n
        culled += sp.n - sf.n
        cp, _ = _render(gpu, cam, _slot_arrays(plain), sp.render_indices, sp.parent_indices, sp.weights, sp.kids)
        cf, _ = _render(gpu, cam, _slot_arrays(frus), sf.render_indices, sf.parent_indices, sf.weights, sf.kids)
        assert torch.equal(cp, cf)
        # the kept entries are the plain cut's: same rows, parents, weights
        rows_p, rows_f = plain.id_of_slot[sp.render_indices.long()], frus.id_of_slot[sf.render_indices.long()]
        keep = torch.isin(rows_p, rows_f)
        assert torch.equal(rows_p[keep], rows_f)
        assert np.array_equal(_bits(sp.weights[:sp.n][keep]), _bits(sf.weights[:sf.n]))
    assert frus.stats["entries_culled"] == culled and plain.stats["entries_culled"] == 0
    assert frus.stats["rows_fetched"] < plain.stats["rows_fetched"]
    assert frus._bounds is not None and torch.equal(frus._bounds[1], bounds) and plain._bounds is None


def test_at_a_quarter_budget_the_frustum_path_renders_finer_and_fetches_less(gpu):
    """Budget = a quarter of the unculled cut at the requested granularity; both paths start cold.

    (a) Six views of a camera flying a circle in the middle of the scene (frustum_cases.flight_camera): the kept cut is a
    third of the plain one, more than the budget, so BOTH paths regulate.  The culled cut at any granularity is a subset
    of the plain cut there, so what fits the plain path fits the frustum path: its regulated tau is <= the plain one's at
    every view.  (Both then FILL the budget, the frustum path with a finer cut -- which is the point of culling under a
    budget -- so its fetches there are not fewer and nothing is asserted about them; the figures are printed.  Measured:
    tau 0.98 .. 1.08 against 1.89 .. 1.99, rows fetched 13 966 against 12 393.)

    (b) Six views on a small orbit deep inside the scene (frustum_cases.inside_orbit_camera): a tenth of the cut is in
    view (tests/test_frustum_cpu.py measures the share for such cameras), well under the budget, so the frustum path
    renders the REQUESTED granularity and fetches at most the rows of the union of six overlapping views, while the plain
    path must regulate and fills the budget on its first view alone (the regulator stops at the first granularity that
    fits, a 5 % step after one that did not): rows_fetched over the orbit is smaller, tau <= again.  Measured: 2 402 rows
    at the requested tau against 5 734 at 34 times that."""
    h, nodes, boxes, means, scales, bounds = _case(20000)
    for label, cams in (("flight", [fc.flight_camera(k) for k in range(6)]),
                        ("inside orbit", [fc.inside_orbit_camera(k) for k in range(6)])):
        tau = fc.tau_of(cams[0], 3.0)
        n_unculled = len(lo.expand_to_size(h.nodes.numpy(), h.boxes.numpy(), tau, cams[0].camera_center.numpy())[0])
        B = n_unculled // 4
        plain, frus = _budgeted(gpu, B), _budgeted(gpu, B)
        assert plain.B == frus.B == B
        for cam in cams:
            sp = _select(plain, nodes, boxes, tau, cam, None)
            sf = _select(frus, nodes, boxes, tau, cam, _planes(cam))
            print(f"{label}: plain tau {sp.tau:.4f} n {sp.n} misses {sp.misses} attempts {sp.attempts} | "
                  f"frustum tau {sf.tau:.4f} n {sf.n} misses {sf.misses} attempts {sf.attempts}")
            assert sp.attempts > 1 or sp.tau > tau                    # the plain path is regulated at every view
            assert sf.tau <= sp.tau
            assert sf.n <= B and sp.n <= B
        print(f"{label}: rows fetched plain {plain.stats['rows_fetched']} frustum {frus.stats['rows_fetched']}, "
              f"entries culled {frus.stats['entries_culled']}")
        if label == "flight":
            assert frus.stats["retries"] > 0                          # (a): the frustum path regulates too
        else:
            assert frus.stats["retries"] == 0                         # (b): it renders what was asked for
            assert frus.stats["rows_fetched"] < plain.stats["rows_fetched"]
        # what the frustum path rendered last is the resident render at ITS granularity, culled
        cam = cams[-1]
        color, _ = _render(gpu, cam, _slot_arrays(frus), sf.render_indices, sf.parent_indices, sf.weights, sf.kids)
        from hgs.frustum import cut_view
        planes, rs = _planes(cam)
        cv = cut_view(nodes, boxes, bounds, sf.tau, cam.camera_center, planes, rs)
        ref, _ = _render(gpu, cam, _attrs(gpu), cv.render_indices, cv.parent_indices, cv.weights, cv.kids)
        assert cv.n == sf.n and torch.equal(color, ref)


def test_prefetch_with_a_frustum_gives_the_selection_of_select_alone(gpu):
    h, nodes, boxes, means, scales, bounds = _case(20000)
    G = nodes.shape[0]
    cams = [fc.camera("B"), fc.camera("C")]
    tau = fc.tau_of(cams[0], 3.0)
    fr = [_planes(c) for c in cams]
    alone, pre = _budgeted(gpu, G), _budgeted(gpu, G)
    _select(alone, nodes, boxes, tau, cams[0], fr[0])
    want = _select(alone, nodes, boxes, tau, cams[1], fr[1])
    _select(pre, nodes, boxes, tau, cams[0], fr[0])
    fetched = pre.prefetch(nodes, boxes, tau, cams[1].camera_center.to(gpu), cams[1].camera_center.cpu(), frustum=fr[1])
    got = _select(pre, nodes, boxes, tau, cams[1], fr[1])
    assert fetched == want.misses > 0 and got.misses == 0             # the rows crossed the bus in the prefetch
    assert (got.n, got.tau, got.attempts) == (want.n, want.tau, want.attempts)
    rows = lambda bh, s, idx: bh.id_of_slot[idx.long()]
    assert torch.equal(rows(pre, got, got.render_indices), rows(alone, want, want.render_indices))
    assert torch.equal(rows(pre, got, got.parent_indices), rows(alone, want, want.parent_indices))
    assert np.array_equal(_bits(got.weights[:got.n]), _bits(want.weights[:want.n]))
    assert torch.equal(got.kids[:got.n], want.kids[:want.n])
    assert pre.stats["entries_culled"] == alone.stats["entries_culled"]
    # a prefetch under another frustum is not reused as this view's cut
    pre.prefetch(nodes, boxes, tau, cams[0].camera_center.to(gpu), cams[0].camera_center.cpu(), frustum=fr[1])
    again = _select(pre, nodes, boxes, tau, cams[0], fr[0])
    first = _select(alone, nodes, boxes, tau, cams[0], fr[0])
    assert again.n == first.n and torch.equal(rows(pre, again, again.render_indices), rows(alone, first, first.render_indices))
