"""GPU parity of the budget-exact hierarchy cut (csrc/lod_budget.hip, hgs.frustum.cut_to_budget) against
tests/budget_cut_spec.py: tau* and the cost bit for bit, the cut equal to cut_view at tau*, the regulator's bound,
refusals, buffer discipline, determinism, and BudgetedHierarchy.select / prefetch with fit="budget"."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import budget_cut_cases as bc
import budget_cut_spec as bs
import frustum_cases as fc
import ws_guard as wg
from hgs import _lib
from oracle import lod_oracle as lo
from test_frustum_gpu import ALL_INSIDE, _attrs, _bits, _budgeted, _np, _planes, _render, _slot_arrays

pytestmark = pytest.mark.gpu

LEAVES = (1, 2, 3, 33, 128, 129, 1000, 20000)       # N = 2 P - 1 nodes: 1, 3, 5, 65, 255, 257, 1999, 39999
FIELDS = ("render_indices", "parent_indices", "node_indices", "kids")


@functools.lru_cache(maxsize=None)
def _case(P):
    """(nodes, boxes CPU arrays; nodes, boxes, means, scales, bounds on the GPU -- the bounds made there)."""
    from hgs.frustum import cull_bounds
    nodes, boxes, _, means, scales = bc.multi_row() if P == "multi" else bc.built(P)
    dev = torch.device("cuda:0")
    g = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (nodes, boxes, means, scales)]
    return nodes, boxes, g[0], g[1], g[2], g[3], cull_bounds(g[0], g[2], g[3])


def _same_cut(a, b):
    assert (a.n, a.n_unculled) == (b.n, b.n_unculled)
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(_bits(a.weights), _bits(b.weights))


def _cut_view_at(g_nodes, g_boxes, g_bounds, tau, cam, planes, rs):
    from hgs.frustum import cut_view
    if planes is None:          # (planes that contain everything: expand_to_size + get_interpolation_weights, as
        planes, rs = ALL_INSIDE, 1.0    # tests/test_frustum_gpu.py checks)
    return cut_view(g_nodes, g_boxes, g_bounds, tau, cam.camera_center, planes, rs)


def _check(case, cam, frustum, view, ev, cost, tau_min, budget, seen):
    """One cut_to_budget call against the spec's descent; the cut against cut_view at tau* (once per tau*)."""
    from hgs.frustum import cut_to_budget
    nodes, boxes, g_nodes, g_boxes, _, _, g_bounds = case
    planes, rs = frustum if frustum is not None else (None, 1.0)
    c_inf = ev.cost(bs.INF_BITS)
    kw = dict(planes=planes, radius_scale=rs, tau_min=tau_min, cost=cost)
    if budget < c_inf:
        with pytest.raises(_lib.HgsError, match=rf"coarsest cut costs {c_inf},") as e:
            cut_to_budget(g_nodes, g_boxes, g_bounds if planes is not None else None, budget, cam.camera_center, **kw)
        assert e.value.code == _lib.ERR_CAPACITY
        return None
    t, c = bs.descent(ev, tau_min, budget)
    got = cut_to_budget(g_nodes, g_boxes, g_bounds if planes is not None else None, budget, cam.camera_center, **kw)
    assert (bs.bits(got.tau), got.cost) == (t, c), (float(tau_min), budget, got.tau, float(bs.value(t)), got.cost, c)
    assert got.cost <= budget and got.n <= got.cost
    key = (t, planes is not None)
    if key not in seen:
        seen[key] = _cut_view_at(g_nodes, g_boxes, g_bounds, got.tau, cam, planes, rs)
    _same_cut(got, seen[key])
    return t


@pytest.mark.parametrize("cost", ["entries", "rows"])
@pytest.mark.parametrize("P", LEAVES + ("multi",))
def test_tau_and_cut_match_the_spec(gpu, P, cost):
    """Both cost modes, with and without planes, cameras A, B, C, the budgets and requests of the issue, and a budget of
    exactly cost(t) and cost(t) - 1 at three interior keys: tau* and the cost are the spec's, the five outputs are
    cut_view's at tau*."""
    case = _case(P)
    nodes, boxes, g_nodes, g_boxes, _, _, g_bounds = case
    N = len(nodes)
    bounds = _np(g_bounds)
    ran = refused = 0
    for name in "ABC":
        cam = fc.camera(name)
        vp = cam.camera_center.numpy()
        frustum = _planes(cam)
        for fr in (None, frustum):
            view = bs.View(nodes, boxes, vp) if fr is None else bs.View(nodes, boxes, vp, bounds, fr[0].numpy(), fr[1])
            ev = bs.Events(view, cost)
            c_inf = ev.cost(bs.INF_BITS)
            seen = {}
            jobs = [(bc.tau_min_of(cam, px), b) for px in bc.TAU_MINS_PX for b in bc.budgets(N, c_inf)]
            keys = np.unique(ev.keys[ev.keys < bs.INF_BITS])
            if len(keys) >= 4:
                for t in keys[[len(keys) // 4, len(keys) // 2, 3 * len(keys) // 4]]:
                    jobs += [(0.0, ev.cost(int(t)) - d) for d in (0, 1) if ev.cost(int(t)) - d >= 0]
            for tau_min, budget in jobs:
                r = _check(case, cam, fr, view, ev, cost, tau_min, budget, seen)
                ran += r is not None
                refused += r is None
    print(f"P {P} cost {cost}: {ran} cuts, {refused} refused for capacity")
    assert ran > 0


@pytest.mark.parametrize("P", [129, 1000, 20000])
def test_entries_budget_is_at_least_as_fine_as_the_regulator(gpu, P):
    """cost = entries without planes is monotone, so tau* is the smallest fitting granularity: at or below the first of
    tau 1.2^k (from 1e-4 for a request of 0, as the regulator starts) whose expand_to_size count fits, with at least
    that count."""
    from gaussian_hierarchy._C import expand_to_size
    from hgs.frustum import cut_to_budget
    nodes, boxes, g_nodes, g_boxes, _, _, _ = _case(P)
    N = len(nodes)
    ri = torch.zeros(N, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    for name in "AB":
        cam = fc.camera(name)
        for px in (None, 3.0):
            tau_min = bc.tau_min_of(cam, px)
            for budget in (N // 8, N // 4, N // 2):
                t, n_reg = tau_min, None
                for k in range(97):
                    n = expand_to_size(g_nodes, g_boxes, t, cam.camera_center.to(gpu), torch.zeros(3), ri, pi, ni)
                    if n <= budget:
                        n_reg = n
                        break
                    t = t * 1.2 if t > 0 else 1e-4
                assert n_reg is not None
                got = cut_to_budget(g_nodes, g_boxes, None, budget, cam.camera_center, tau_min=tau_min, cost="entries")
                print(f"P {P} {name} request {tau_min:.5f} budget {budget}: regulator tau {t:.5f} n {n_reg} after {k + 1} "
                      f"cuts | budget cut tau {got.tau:.5f} n {got.n}")
                assert np.float32(got.tau) <= np.float32(t) and n_reg <= got.n <= budget and got.cost == got.n


def _non_nested(P=1000):
    nodes, boxes, g_nodes, g_boxes, _, _, g_bounds = _case(P)
    x = int(nodes[-1, 1])                                 # the last leaf's parent with an extent above its parent's
    bad = g_boxes.clone()
    bad[x, 0, 3] = 1e6
    return g_nodes, bad, g_bounds


def test_a_non_nested_hierarchy_is_refused(gpu):
    from gaussian_hierarchy import _C as gh
    from hgs.frustum import cut_to_budget
    g_nodes, bad, g_bounds = _non_nested()
    assert not gh._boxes_nested(g_nodes, bad)
    cam = fc.camera("A")
    for cost in ("entries", "rows"):
        with pytest.raises(ValueError, match="do not"):
            cut_to_budget(g_nodes, bad, None, 100, cam.camera_center, cost=cost)
    # the C call finds it from this viewpoint when it counts rows (a child larger than its parent), and writes no output
    lib, N, p = _lib.lib(), int(g_nodes.shape[0]), _lib.ptr
    out = [torch.full((N,), -7, dtype=torch.int32, device=gpu) for _ in range(5)]
    tmp = torch.empty(lib.hgs_lod_cut_budget_tmp_bytes(N), dtype=torch.uint8, device=gpu)
    vp = (C.c_float * 3)(*[float(x) for x in cam.camera_center])
    n, na, tau, cst = C.c_int32(0), C.c_int32(0), C.c_float(0), C.c_int32(0)
    rc = lib.hgs_lod_cut_budget(p(g_nodes), p(bad), None, N, 0.01, N, _lib.CUT_COST_ROWS, vp, None, 1.0,
                                *[p(t) for t in out], N, p(tmp), C.byref(n), C.byref(na), C.byref(tau), C.byref(cst),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream), 0)
    assert rc == 1 and b"do not nest" in lib.hgs_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out)


@pytest.mark.parametrize("P", [129, "multi"])
def test_a_budget_below_the_roots_rows_names_the_count_and_writes_no_output(gpu, P):
    """The outputs keep their bytes and every guard -- the workspace's too -- is intact.  (The workspace itself holds the
    sizes and the descent's state by then: the count comes from the device.)"""
    nodes, boxes, g_nodes, g_boxes, _, _, g_bounds = _case(P)
    N, root = len(nodes), int(nodes[0, 3] + nodes[0, 4])
    assert root >= 1
    lib, p = _lib.lib(), _lib.ptr
    cam = fc.camera("A")
    vp = (C.c_float * 3)(*[float(x) for x in cam.camera_center])
    for mode in (_lib.CUT_COST_ENTRIES, _lib.CUT_COST_ROWS):
        for fill in (0x00, 0xFF):
            gs = {k: wg.guarded(4 * N, gpu, fill, k) for k in ("ri", "pi", "ni", "w", "ns")}
            gs["tmp"] = wg.guarded(lib.hgs_lod_cut_budget_tmp_bytes(N), gpu, fill, "tmp")
            before = {k: gs[k].body.clone() for k in ("ri", "pi", "ni", "w", "ns")}
            a = lambda k: C.c_void_p(gs[k].addr)
            n, na, tau, cst = C.c_int32(5), C.c_int32(5), C.c_float(5), C.c_int32(5)
            rc = lib.hgs_lod_cut_budget(p(g_nodes), p(g_boxes), None, N, 0.0, root - 1, mode, vp, None, 1.0, a("ri"),
                                        a("pi"), a("ni"), a("w"), a("ns"), N, a("tmp"), C.byref(n), C.byref(na),
                                        C.byref(tau), C.byref(cst), C.c_void_p(torch.cuda.current_stream().cuda_stream), 0)
            assert rc == _lib.ERR_CAPACITY and (n.value, na.value, cst.value) == (0, 0, root)
            assert f"coarsest cut costs {root}, more than the budget of {root - 1}".encode() in lib.hgs_last_error()
            wg.check(*gs.values())
            for k, t in before.items():
                assert torch.equal(gs[k].body, t), k


@pytest.mark.parametrize("P", [1, 129, 20000])
def test_camera_facing_away_gets_the_request_and_an_empty_cut(gpu, P):
    """Every ball is behind the near plane: the kept cost is 0 at every tau, so tau* = tau_min and n = 0 whatever the
    budget; no error from an empty launch, outputs untouched."""
    from hgs.frustum import CutBuffers, cut_to_budget
    nodes, boxes, g_nodes, g_boxes, _, _, g_bounds = _case(P)
    cam = fc.yaw_camera((0.0, 0.0, -50.0), 180.0)
    planes, rs = _planes(cam)
    out = CutBuffers(max(len(nodes), 3), gpu)
    for t in (out.ri, out.pi, out.ni, out.ns):
        t.fill_(-7)
    out.w.fill_(-7.0)
    for cost in ("entries", "rows"):
        for tau_min in (0.0, fc.tau_of(cam, 3.0), fc.tau_of(cam, 40.0)):
            for budget in (0, 1, 3):
                cut = cut_to_budget(g_nodes, g_boxes, g_bounds, budget, cam.camera_center, planes, rs, tau_min=tau_min,
                                    cost=cost, out=out)
                assert (cut.n, cut.cost, bs.bits(cut.tau)) == (0, 0, bs.bits(tau_min)) and cut.n_unculled > 0
                assert cut.render_indices.numel() == 0
    torch.cuda.synchronize()
    assert bool((out.ri == -7).all()) and bool((out.ns == -7).all()) and bool((out.w == -7.0).all())


@pytest.mark.parametrize("cost", ["entries", "rows"])
@pytest.mark.parametrize("P,culled", [(129, True), (129, False), (1000, True), ("multi", False)])
def test_outputs_and_workspace_stay_inside_their_bytes(gpu, P, culled, cost):
    """Every output at exactly ``budget`` entries and the workspace at exactly hgs_lod_cut_budget_tmp_bytes, each between
    two guards, free bytes filled once with 0x00 and once with 0xFF: intact guards, bit-equal results."""
    from hgs.frustum import cut_to_budget
    nodes, boxes, g_nodes, g_boxes, _, _, g_bounds = _case(P)
    N = len(nodes)
    cam = fc.camera("B")
    planes, rs = _planes(cam) if culled else (None, 1.0)
    budget = max(N // 8, 4)
    tau_min = fc.tau_of(cam, 3.0)
    ref = cut_to_budget(g_nodes, g_boxes, g_bounds if culled else None, budget, cam.camera_center, planes, rs,
                        tau_min=tau_min, cost=cost)
    print(f"P {P} culled {culled} cost {cost}: request {tau_min:.5f} tau* {ref.tau:.5f} n {ref.n} cost {ref.cost} of {budget}")
    assert 0 < ref.n <= ref.cost <= budget
    lib, p = _lib.lib(), _lib.ptr
    vp = (C.c_float * 3)(*[float(x) for x in cam.camera_center])
    pl = (C.c_float * 20)(*[float(x) for x in planes.reshape(-1)]) if culled else None
    results = []
    for fill in (0x00, 0xFF):
        gs = {k: wg.guarded(4 * budget, gpu, fill, k) for k in ("ri", "pi", "ni", "w", "ns")}
        gs["tmp"] = wg.guarded(lib.hgs_lod_cut_budget_tmp_bytes(N), gpu, fill, "tmp")
        a = lambda k: C.c_void_p(gs[k].addr)
        n, na, tau, cst = C.c_int32(0), C.c_int32(0), C.c_float(0), C.c_int32(0)
        _lib.check(lib.hgs_lod_cut_budget(p(g_nodes), p(g_boxes), p(g_bounds) if culled else None, N, float(tau_min), budget,
                                          bs_mode(cost), vp, pl, float(rs), a("ri"), a("pi"), a("ni"), a("w"), a("ns"),
                                          budget, a("tmp"), C.byref(n), C.byref(na), C.byref(tau), C.byref(cst),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream), 0), "cut_budget")
        wg.check(*gs.values())
        assert (n.value, na.value, tau.value, cst.value) == (ref.n, ref.n_unculled, ref.tau, ref.cost)
        results.append({k: gs[k].body[:4 * ref.n].clone() for k in ("ri", "pi", "ni", "w", "ns")})
    for k, t in (("ri", ref.render_indices), ("pi", ref.parent_indices), ("ni", ref.node_indices), ("w", ref.weights),
                 ("ns", ref.kids)):
        assert torch.equal(results[0][k], results[1][k]), k
        assert torch.equal(results[0][k], t.contiguous().view(-1).view(torch.uint8)), k


def bs_mode(cost):
    return {"entries": _lib.CUT_COST_ENTRIES, "rows": _lib.CUT_COST_ROWS}[cost]


def test_two_calls_and_two_streams_give_the_same_bits(gpu):
    from hgs.frustum import cut_to_budget
    nodes, boxes, g_nodes, g_boxes, _, _, g_bounds = _case(20000)
    cam = fc.camera("B")
    planes, rs = _planes(cam)
    args = (g_nodes, g_boxes, g_bounds, len(nodes) // 8, cam.camera_center, planes, rs)
    ref = cut_to_budget(*args, tau_min=fc.tau_of(cam, 3.0))
    assert ref.tau > fc.tau_of(cam, 3.0) and ref.n > 100
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=gpu) for _ in range(2)]
    cuts = []
    for rep in range(2):
        for s in streams:
            with torch.cuda.stream(s):
                cuts.append(cut_to_budget(*args, tau_min=fc.tau_of(cam, 3.0)))
    torch.cuda.synchronize()
    for cut in cuts:
        assert (bs.bits(cut.tau), cut.cost) == (bs.bits(ref.tau), ref.cost)
        _same_cut(cut, ref)


def test_bad_arguments_are_refused(gpu):
    from hgs.frustum import CutBuffers, cut_to_budget
    nodes, boxes, g_nodes, g_boxes, _, _, g_bounds = _case(1000)
    cam = fc.camera("A")
    planes, rs = _planes(cam)
    args = dict(nodes=g_nodes, boxes=g_boxes, bounds=g_bounds, budget=100, viewpoint=cam.camera_center, planes=planes,
                radius_scale=rs)
    assert cut_to_budget(**args).cost <= 100
    for key, bad in (("nodes", g_nodes.cpu()), ("boxes", g_boxes.cpu()), ("bounds", g_bounds.cpu()), ("nodes", g_nodes.long()),
                     ("boxes", g_boxes.double()), ("bounds", g_bounds.half()), ("nodes", g_nodes[:, :6]),
                     ("boxes", g_boxes[:-1]), ("bounds", g_bounds[:, :3]), ("bounds", g_bounds[:-1]),
                     ("nodes", g_nodes.t().contiguous().t()), ("planes", planes[:4]), ("viewpoint", torch.zeros(4)),
                     ("bounds", None), ("planes", None), ("budget", -1), ("budget", 2 ** 31), ("tau_min", -0.5),
                     ("tau_min", float("nan")), ("cost", "bytes")):
        with pytest.raises(ValueError):
            cut_to_budget(**dict(args, **{key: bad}))
    odd = CutBuffers(100, gpu)
    odd.w = odd.w.double()
    with pytest.raises(ValueError):
        cut_to_budget(**args, out=odd)
    with pytest.raises(_lib.HgsError, match="outputs hold 99 entries"):     # fewer entries than the budget may need
        cut_to_budget(**args, out=CutBuffers(99, gpu))


# ---- the budgeted viewer path ------------------------------------------------------------------------------------------
def _select(bh, nodes, boxes, tau, cam, frustum, fit):
    kw = {} if frustum is None else dict(frustum=frustum)
    return bh.select(nodes, boxes, tau, cam.camera_center.to(bh.dev), cam.camera_center.cpu(), fit=fit, **kw)


def _needed_rows(g_nodes, g_boxes, g_bounds, tau, cam, frustum):
    """Distinct rows the cut at ``tau`` reads: every entry's row and the parent row of the entries of weight < 1."""
    cv = _cut_view_at(g_nodes, g_boxes, g_bounds, tau, cam, *(frustum if frustum is not None else (None, 1.0)))
    return torch.unique(torch.cat([cv.render_indices, cv.parent_indices[cv.weights < 1.0]])).long(), cv


@pytest.mark.parametrize("culled", [False, True])
@pytest.mark.parametrize("path", ["flight", "inside orbit"])
def test_budget_fit_selects_once_and_renders_the_cut_at_its_tau(gpu, path, culled):
    """20 000 leaves, a budget of a quarter of the unculled cut at the request, cold start, six views: one cut and no
    retry per view, the resident rows within the budget, the fetched plus the already resident rows equal to the cost
    the cut was selected at, and the image that of a generous-budget plain select at Selection.tau, bit for bit.  The
    regulator's tau is printed beside tau*; no order is asserted (rows(tau) is not monotone: the regulator may land in a
    fitting pocket below tau*)."""
    nodes, boxes, g_nodes, g_boxes, _, _, g_bounds = _case(20000)
    cams = [(fc.flight_camera if path == "flight" else fc.inside_orbit_camera)(k) for k in range(6)]
    tau = fc.tau_of(cams[0], 3.0)
    B = len(lo.expand_to_size(nodes, boxes, tau, cams[0].camera_center.numpy())[0]) // 4
    exact, reg, gen = _budgeted(gpu, B), _budgeted(gpu, B), _budgeted(gpu, len(nodes))
    for i, cam in enumerate(cams):
        fr = _planes(cam) if culled else None
        resident = exact.slot_of >= 0
        s = _select(exact, g_nodes, g_boxes, tau, cam, fr, "budget")
        r = _select(reg, g_nodes, g_boxes, tau, cam, fr, "regulate")
        need, cv = _needed_rows(g_nodes, g_boxes, g_bounds, s.tau, cam, fr)
        hits = int(resident[need].sum())
        print(f"{path} culled {culled} view {i}: budget tau {s.tau:.5f} n {s.n} cost {s.cost} misses {s.misses} hits {hits} "
              f"| regulate tau {r.tau:.5f} n {r.n} attempts {r.attempts}")
        assert s.attempts == 1 and exact.stats["retries"] == 0
        assert s.tau >= np.float32(tau) and s.n == cv.n and s.cost <= B
        assert exact.resident_rows <= B
        assert s.misses + hits == s.cost == need.numel()
        g = _select(gen, g_nodes, g_boxes, s.tau, cam, fr, "regulate")
        assert g.attempts == 1 and g.tau == s.tau and g.n == s.n
        got, _ = _render(gpu, cam, _slot_arrays(exact), s.render_indices, s.parent_indices, s.weights, s.kids)
        want, _ = _render(gpu, cam, _slot_arrays(gen), g.render_indices, g.parent_indices, g.weights, g.kids)
        assert torch.equal(got, want)
    assert exact._regulated is None and exact.stats["views"] == 6


@pytest.mark.parametrize("culled", [False, True])
def test_budget_fit_with_a_generous_budget_is_the_request(gpu, culled):
    nodes, boxes, g_nodes, g_boxes, _, _, g_bounds = _case(20000)
    a, b = _budgeted(gpu, len(nodes)), _budgeted(gpu, len(nodes))
    for name in "ABC":
        cam = fc.camera(name)
        tau = fc.tau_of(cam, 3.0)
        fr = _planes(cam) if culled else None
        sa = _select(a, g_nodes, g_boxes, tau, cam, fr, "budget")
        sb = _select(b, g_nodes, g_boxes, tau, cam, fr, "regulate")
        assert sa.tau == float(np.float32(tau)) and sb.tau == tau and (sa.n, sa.attempts) == (sb.n, 1) and sa.misses == sb.misses
        ca, _ = _render(gpu, cam, _slot_arrays(a), sa.render_indices, sa.parent_indices, sa.weights, sa.kids)
        cb, _ = _render(gpu, cam, _slot_arrays(b), sb.render_indices, sb.parent_indices, sb.weights, sb.kids)
        assert torch.equal(ca, cb)
    assert a.stats["entries_culled"] == b.stats["entries_culled"]
    with pytest.raises(ValueError, match="fit"):
        _select(a, g_nodes, g_boxes, tau, cam, fr, "exact")


@pytest.mark.parametrize("generous", [True, False])
@pytest.mark.parametrize("culled", [False, True])
def test_prefetch_then_select_is_select_alone(gpu, culled, generous):
    nodes, boxes, g_nodes, g_boxes, _, _, g_bounds = _case(20000)
    cams = [fc.flight_camera(0), fc.flight_camera(1)]
    tau = fc.tau_of(cams[0], 3.0)
    B = len(nodes) if generous else len(lo.expand_to_size(nodes, boxes, tau, cams[0].camera_center.numpy())[0]) // 4
    fr = [_planes(c) if culled else None for c in cams]
    alone, pre = _budgeted(gpu, B), _budgeted(gpu, B)
    _select(alone, g_nodes, g_boxes, tau, cams[0], fr[0], "budget")
    want = _select(alone, g_nodes, g_boxes, tau, cams[1], fr[1], "budget")
    _select(pre, g_nodes, g_boxes, tau, cams[0], fr[0], "budget")
    kw = {} if fr[1] is None else dict(frustum=fr[1])
    fetched = pre.prefetch(g_nodes, g_boxes, tau, cams[1].camera_center.to(gpu), cams[1].camera_center.cpu(), fit="budget", **kw)
    reused = pre._prefetched is not None
    got = _select(pre, g_nodes, g_boxes, tau, cams[1], fr[1], "budget")
    print(f"culled {culled} generous {generous}: prefetched {fetched} rows, cut reused {reused}, select fetched {got.misses} "
          f"(alone: {want.misses})")
    if generous:
        assert reused and fetched == want.misses > 0 and got.misses == 0    # the rows crossed the bus in the prefetch
    assert fetched + got.misses == want.misses
    assert (got.n, got.tau, got.cost, got.attempts) == (want.n, want.tau, want.cost, 1)
    rows = lambda bh, idx: bh.id_of_slot[idx.long()]
    assert torch.equal(rows(pre, got.render_indices), rows(alone, want.render_indices))
    assert torch.equal(rows(pre, got.parent_indices), rows(alone, want.parent_indices))
    assert np.array_equal(_bits(got.weights[:got.n]), _bits(want.weights[:want.n]))
    assert torch.equal(got.kids[:got.n], want.kids[:want.n])
    assert pre.stats["retries"] == alone.stats["retries"] == 0
    # a budget prefetch is not taken for the regulator's cut, nor the other way round
    pre.prefetch(g_nodes, g_boxes, tau, cams[0].camera_center.to(gpu), cams[0].camera_center.cpu(), fit="budget",
                 **({} if fr[0] is None else dict(frustum=fr[0])))
    if generous:
        again = _select(pre, g_nodes, g_boxes, tau, cams[0], fr[0], "regulate")
        first = _select(alone, g_nodes, g_boxes, tau, cams[0], fr[0], "regulate")
        assert (again.n, again.tau) == (first.n, first.tau)
        assert torch.equal(rows(pre, again.render_indices), rows(alone, first.render_indices))
