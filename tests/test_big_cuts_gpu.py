"""The four hierarchy cuts where their scan takes a second chunk: expand_to_size (csrc/lod.hip), cut_view
(lod_frustum.hip), cut_to_budget (lod_budget.hip) and cut_views (lod_views.hip) on the 2 099 999-node hierarchy of
tests/big_cut_cases.py -- 8 204 workgroup sums, 12 of them behind the 8 192 one scan workgroup covers -- against
tests/big_cut_spec.py and against each other.  Below 2 097 153 nodes the published chunk totals, the look-back over them,
clear_scan_chain(), the second chunk's add into the unculled total, cut_views' per-view strides into ``chain`` and the
tail write behind a prefix never run or never matter; the budget histogram's grid-stride loop takes its second step from
524 289 nodes.  Every comparison is exact: integers equal, weights and tau* as bit patterns.

Each view's expected cut comes through big_cut_cases.spec(), which asserts that nodes behind the seam emit (and, under a
cull, that some are kept): a test cannot pass on a view that leaves the second chunk empty."""
import ctypes as C

import numpy as np
import pytest
import torch

import big_cut_cases as bcs
import budget_cut_spec as bs
from hgs import _lib
from test_frustum_gpu import ALL_INSIDE, _assert_cut_equals_spec

pytestmark = pytest.mark.gpu

FIELDS = ("render_indices", "parent_indices", "node_indices", "weights", "kids")
VIEWS = [(name, px) for name in bcs.CAMERAS for px in bcs.TAUS_PX]
SENTINEL = -7


def _np(t):
    return t.cpu().numpy()


def _assert_same_cut(a, b, what=""):
    assert (a.n, a.n_unculled) == (b.n, b.n_unculled), (what, a.n, a.n_unculled, b.n, b.n_unculled)
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, f)


def _cycled(V):
    """V views with a camera and a granularity each: both cycled, the granularities one further every three views, so
    that neighbours differ in both and the first nine are all the pairs."""
    return [(bcs.CAMERAS[k % 3], bcs.TAUS_PX[(k + k // 3) % 3]) for k in range(V)]


def test_the_fixture_crosses_the_seam(gpu):
    """The conditions the other tests lean on, from the spec on the GPU-built hierarchy (printed: profiles/
    big_cuts_tests.md records them)."""
    from gaussian_hierarchy import _C as gh
    f = bcs.big()
    nblk = (f.N + 255) // 256
    assert f.N == 2_099_999 and nblk == 8204 and nblk - bcs.SCAN_CHUNK == 12 and f.N - bcs.SEAM == 2847
    assert f.N > bcs.HIST_SEAM
    depth = f.nodes_h[:, 0]
    assert np.all(np.diff(depth) >= 0)                                   # numbered level by level ...
    tail = f.nodes_h[bcs.SEAM:]
    assert np.all(tail[:, 0] == depth.max()) and np.all(tail[:, 3] == 1) and np.all(tail[:, 6] == 0)     # ... deepest leaves
    assert gh._boxes_nested(f.nodes, f.boxes)
    for name, px in VIEWS:
        c = bcs.seam_counts(name, px)
        print(f"camera {name} at {px} px: {c}")
        for culled in (False, True):
            assert bcs.host_view(name, culled).nested()
            bcs.spec(name, px, culled)                                  # asserts the seam conditions of this view
        assert c["culled_hi"] >= 1 and c["kept_lo"] < c["emit_lo"]       # kept and culled on both sides
        if px == -0.5:
            assert c["emit_hi"] == 2847 and c["entries"] == bcs.LEAVES   # tau = 0: every leaf
    b3 = bcs.seam_counts("B", 3.0)
    assert b3["emit_hi"] >= 500 and b3["kept_hi"] >= 100 and b3["culled_hi"] >= 100


@pytest.mark.parametrize("name,px", VIEWS)
def test_expand_to_size_and_weights(gpu, name, px):
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    f, v, spec = bcs.big(), bcs.view(name, px), bcs.spec(name, px, False)
    ri = torch.full((f.N,), SENTINEL, dtype=torch.int32, device=gpu); pi = ri.clone(); ni = ri.clone()
    n = expand_to_size(f.nodes, f.boxes, v["tau"], v["vp"], torch.zeros(3), ri, pi, ni)
    assert n == spec["n"] == spec["n_unculled"]
    assert np.array_equal(_np(ri[:n]), spec["render_indices"]) and np.array_equal(_np(pi[:n]), spec["parent_indices"])
    assert np.array_equal(_np(ni[:n]), spec["node_indices"])
    assert bool((ri[n:] == SENTINEL).all()) and bool((ni[n:] == SENTINEL).all())
    w = torch.zeros(n, device=gpu); ns = torch.zeros(n, dtype=torch.int32, device=gpu)
    get_interpolation_weights(ni[:n], v["tau"], f.nodes, f.boxes, v["vp"], torch.zeros(3), w, ns)
    assert np.array_equal(_np(w).view(np.uint32), spec["weights"].view(np.uint32))
    assert np.array_equal(_np(ns), spec["kids"])


@pytest.mark.parametrize("name,px", VIEWS)
def test_cut_view_on_both_routes(gpu, name, px):
    """n_unculled is the word only the add from more than one chunk produces.  With planes that contain everything the
    cut is expand_to_size's."""
    from gaussian_hierarchy._C import expand_to_size
    from hgs.frustum import cut_view
    f, v = bcs.big(), bcs.view(name, px)
    spec, plain = bcs.spec(name, px, True), bcs.spec(name, px, False)
    assert 0 < spec["n"] < spec["n_unculled"] == plain["n"]
    for route in (True, False, None):
        _assert_cut_equals_spec(cut_view(f.nodes, f.boxes, f.bounds, v["tau"], v["vp"], v["planes"], v["rs"], nested=route), spec)
    ri = torch.zeros(f.N, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    n = expand_to_size(f.nodes, f.boxes, v["tau"], v["vp"], torch.zeros(3), ri, pi, ni)
    for route in (True, False):
        cv = cut_view(f.nodes, f.boxes, f.bounds, v["tau"], v["vp"], ALL_INSIDE, 1.4, nested=route)
        _assert_cut_equals_spec(cv, plain)
        assert cv.n == cv.n_unculled == n and torch.equal(cv.render_indices, ri[:n])
        assert torch.equal(cv.parent_indices, pi[:n]) and torch.equal(cv.node_indices, ni[:n])


def _budget_jobs(name, culled, cost):
    """(tau_min, budget) of the budget test, all from a request of 3 px: an eighth of the request's cost; then exactly
    the cost at an interior event key t -- the largest at or below the 15 px granularity -- and one less.  (Rows, and any
    cost under a cull, may cost MORE at 15 px than at 3 px: then the request fits and tau* is the request, rule 3.)"""
    ev = bcs.events(name, culled, cost)
    tau3, tau15 = bcs.view(name, 3.0)["tau"], bcs.view(name, 15.0)["tau"]
    keys = ev.keys[(ev.keys > bs.bits(tau3)) & (ev.keys <= bs.bits(tau15))]
    assert keys.size and ev.keys[0] < keys[-1] < ev.keys[-1]
    t = int(keys[-1])
    return [(tau3, ev.cost(bs.bits(tau3)) // 8), (tau3, ev.cost(t)), (tau3, ev.cost(t) - 1)]


@pytest.mark.parametrize("culled", [False, True])
@pytest.mark.parametrize("cost", ["entries", "rows"])
@pytest.mark.parametrize("name", bcs.CAMERAS)
def test_cut_to_budget(gpu, name, cost, culled):
    """tau* as a bit pattern and the cost are the spec's descent (and, where the cost is monotone, the smallest fit); the
    cut is cut_view's at tau*, bit for bit.  The first size at which budget_hist_kernel's grid-stride loop takes more
    than one step: nodes from 524 288 on reach the histogram in a later step of a workgroup that has already added."""
    from hgs.frustum import cut_to_budget, cut_view
    f, v = bcs.big(), bcs.view(name, 3.0)
    hv, ev = bcs.host_view(name, culled), bcs.events(name, culled, cost)
    planes, rs, bounds = (v["planes"], v["rs"], f.bounds) if culled else (None, 1.0, None)
    behind_hist_seam = int(((hv.s_par >= np.float32(v["tau"])) & hv.kept)[bcs.HIST_SEAM:].sum())
    assert behind_hist_seam > 1000                        # events of the later grid-stride steps decide the costs
    descents = 0
    for k, (tau_min, budget) in enumerate(_budget_jobs(name, culled, cost)):
        t, c = bs.descent(ev, tau_min, budget)
        descents += t != bs.bits(tau_min)
        if cost == "entries" and not culled:                # monotone (tests/test_budget_cut_cpu.py): the smallest fit
            assert t == ev.smallest_fit(tau_min, budget)
        got = cut_to_budget(f.nodes, f.boxes, bounds, budget, v["vp"], planes, rs, tau_min=tau_min, cost=cost)
        print(f"{name} {cost} culled {culled}: request {tau_min:.6f} budget {budget} -> tau* {got.tau:.6f} cost {got.cost} n {got.n}")
        assert (bs.bits(got.tau), got.cost) == (t, c), (tau_min, budget, got.tau, float(bs.value(t)), got.cost, c)
        assert got.n <= got.cost <= budget
        if k > 0:                                           # at most 15 px: the cut at tau* has entries behind the seam
            assert int(((hv.s_par >= bs.value(t)) & hv.kept)[bcs.SEAM:].sum()) >= 1
        ref = (cut_view(f.nodes, f.boxes, f.bounds, got.tau, v["vp"], planes, rs) if culled
               else cut_view(f.nodes, f.boxes, f.bounds, got.tau, v["vp"], ALL_INSIDE, 1.0))
        _assert_same_cut(got, ref, (tau_min, budget))
    assert descents >= 1                                    # the eighth never fits: all three digits ran


def _views_call(views, culled, **kw):
    from hgs.frustum import cut_views
    f = bcs.big()
    vs = [bcs.view(*x) for x in views]
    if not culled:
        return cut_views(f.nodes, f.boxes, None, [v["tau"] for v in vs], torch.stack([v["vp"] for v in vs]), **kw)
    return cut_views(f.nodes, f.boxes, f.bounds, [v["tau"] for v in vs], torch.stack([v["vp"] for v in vs]),
                     torch.stack([v["planes"] for v in vs]), [v["rs"] for v in vs], **kw)


def _sentinel_buffers(cap, gpu):
    from hgs.frustum import CutBuffers
    out = CutBuffers(cap, gpu)
    for t in (out.ri, out.pi, out.ni, out.ns):
        t.fill_(SENTINEL)
    out.w.fill_(float(SENTINEL))
    return out


def _single(name, px, culled):
    from hgs.frustum import cut_view
    f, v = bcs.big(), bcs.view(name, px)
    planes, rs = (v["planes"], v["rs"]) if culled else (ALL_INSIDE, 1.0)
    return cut_view(f.nodes, f.boxes, f.bounds, v["tau"], v["vp"], planes, rs, nested=True)


def _check_packed_views(gpu, views, culled, specs):
    """One cut_views call into sentinel-filled buffers: every view is cut_view's and the spec's, starts on 16 bytes
    behind the views before it, and nothing else is written."""
    refs = {x: _single(*x, culled) for x in dict.fromkeys(views)}
    cap = sum((refs[x].n + 3) // 4 * 4 for x in views) + 37
    out = _sentinel_buffers(cap, gpu)
    cuts = _views_call(views, culled, out=out)
    torch.cuda.synchronize()
    assert len(cuts) == len(views)
    written = torch.zeros(cap, dtype=torch.bool, device=gpu)
    at = 0
    for k, (x, cv) in enumerate(zip(views, cuts)):
        _assert_same_cut(cv, refs[x], f"view {k} {x}")
        if k < 9:                                           # (the cycle repeats from the tenth view on)
            _assert_cut_equals_spec(cv, specs[k])
        for fld in FIELDS:
            assert getattr(cv, fld).storage_offset() == at
        assert at % 4 == 0 and (cv.n == 0 or cv.render_indices.data_ptr() % 16 == 0)
        written[at:at + cv.n] = True
        at += (cv.n + 3) // 4 * 4
    for buf in (out.ri, out.pi, out.ni, out.ns):
        assert bool((buf[~written] == SENTINEL).all())
    assert bool((out.w[~written] == float(SENTINEL)).all())
    assert int((~written).sum()) >= 37
    return cuts


@pytest.mark.parametrize("culled", [True, False])
@pytest.mark.parametrize("V", [1, 3, 16])
def test_cut_views(gpu, V, culled):
    """A camera and a granularity per view: a swapped or dropped stride into the per-view sums and chains gives a view
    another view's prefix."""
    views = _cycled(V)
    assert len(set(views)) == min(V, 9)
    cuts = _check_packed_views(gpu, views, culled, [bcs.spec(*x, culled) for x in views[:9]])
    # no view could be taken for its neighbour (without a cull B and C, at one viewpoint, share their counts; with one
    # all nine pairs differ)
    assert all(a.n != b.n for a, b in zip(cuts, cuts[1:]))
    assert not culled or len({cv.n for cv in cuts[:9]}) == min(V, 9)
    if V == 16 and culled:
        assert any(cv.n % 4 for cv in cuts[:-1])                # and some offset needed rounding


def test_cut_views_behind_an_empty_view(gpu):
    """The first view faces away and keeps nothing: the later views' bases are sums that include a zero."""
    views = [("away", 3.0), ("B", 3.0), ("O", 15.0)]
    empty = bcs.raw_spec("away", 3.0, True)
    assert empty["n"] == 0 and empty["n_unculled"] > 0
    cuts = _check_packed_views(gpu, views, True, [empty, bcs.spec("B", 3.0, True), bcs.spec("O", 15.0, True)])
    assert cuts[0].n == 0 and cuts[0].n_unculled == empty["n_unculled"] and cuts[1].render_indices.storage_offset() == 0


# ---- the C ABI: what the workspace holds when a call starts ----------------------------------------------------------
def _floats(xs):
    return (C.c_float * len(xs))(*[float(x) for x in xs])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _budget_of(name, px, cost):
    """(tau_min, budget): a request of ``px`` pixels and 7/8 of its culled cost -- it never fits, so the descent runs all
    three digits, and tau* lies close enough above the request that nodes behind the seam are in the cut."""
    tau = bcs.view(name, px)["tau"]
    return tau, bcs.events(name, True, cost).cost(bs.bits(tau)) * 7 // 8


KINDS = ("expand_nested", "expand_levels", "cut_view_nested", "cut_view_levels", "budget_entries", "budget_rows",
         "views_culled", "views_plain")


def _tmp_bytes(kind, V=1):
    lib, N = _lib.lib(), bcs.big().N
    if kind.startswith("expand"):
        return lib.hgs_expand_tmp_bytes(N)
    if kind.startswith("cut_view"):
        return lib.hgs_lod_cut_view_tmp_bytes(N)
    if kind.startswith("budget"):
        return lib.hgs_lod_cut_budget_tmp_bytes(N)
    return lib.hgs_lod_cut_views_tmp_bytes(N, V)


def _python_call(kind, views):
    """The same call through the Python layer -> one CutView-like result per view (expand: the three index arrays)."""
    from gaussian_hierarchy._C import expand_to_size
    from hgs.frustum import CutView, cut_to_budget, cut_view
    f = bcs.big()
    if kind.startswith("views"):
        return _views_call(views, kind == "views_culled")
    (name, px), = views
    v = bcs.view(name, px)
    if kind.startswith("expand"):                           # (the Python layer takes the single-pass route: boxes nest)
        ri = torch.zeros(f.N, dtype=torch.int32, device=f.nodes.device); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
        n = expand_to_size(f.nodes, f.boxes, v["tau"], v["vp"], torch.zeros(3), ri, pi, ni)
        return [CutView(n, n, ri[:n], pi[:n], ni[:n], None, None)]
    if kind.startswith("cut_view"):
        return [cut_view(f.nodes, f.boxes, f.bounds, v["tau"], v["vp"], v["planes"], v["rs"], nested=kind == "cut_view_nested")]
    cost = kind.split("_")[1]
    tau_min, budget = _budget_of(name, px, cost)
    got = cut_to_budget(f.nodes, f.boxes, f.bounds, budget, v["vp"], v["planes"], v["rs"], tau_min=tau_min, cost=cost)
    hv = bcs.host_view(name, True)
    assert got.tau > tau_min and int(((hv.s_par >= np.float32(got.tau)) & hv.kept)[bcs.SEAM:].sum()) >= 1
    return [got]


def _abi_call(kind, views, outs, cap, tmp):
    """The call on raw addresses: ``outs`` five (expand: three used) output addresses of ``cap`` entries, ``tmp`` the
    workspace.  -> (the host words the call returns, [(offset, n) of every view's entries])."""
    lib, p, f = _lib.lib(), _lib.ptr, bcs.big()
    o = [C.c_void_p(a) for a in outs]
    vs = [bcs.view(*x) for x in views]
    v = vs[0]
    if kind.startswith("expand"):
        fn = lib.hgs_expand_to_size_nested if kind == "expand_nested" else lib.hgs_expand_to_size
        n = C.c_int32(0)
        _lib.check(fn(p(f.nodes), p(f.boxes), f.N, float(v["tau"]), _floats(v["vp"]), _floats([0, 0, 0]), o[0], o[1], o[2],
                      cap, C.c_void_p(tmp), C.byref(n), _stream(), 0), kind)
        return (n.value,), [(0, n.value)]
    if kind.startswith("cut_view"):
        n, n_all = C.c_int32(0), C.c_int32(0)
        _lib.check(lib.hgs_lod_cut_view(p(f.nodes), p(f.boxes), p(f.bounds), f.N, float(v["tau"]), _floats(v["vp"]),
                                        _floats(v["planes"].reshape(-1)), float(v["rs"]), int(kind == "cut_view_nested"),
                                        *o, cap, C.c_void_p(tmp), C.byref(n), C.byref(n_all), _stream(), 0), kind)
        return (n.value, n_all.value), [(0, n.value)]
    if kind.startswith("budget"):
        cost = kind.split("_")[1]
        mode = {"entries": _lib.CUT_COST_ENTRIES, "rows": _lib.CUT_COST_ROWS}[cost]
        n, n_all, tau, cst = C.c_int32(0), C.c_int32(0), C.c_float(0), C.c_int32(0)
        tau_min, budget = _budget_of(*views[0], cost)
        _lib.check(lib.hgs_lod_cut_budget(p(f.nodes), p(f.boxes), p(f.bounds), f.N, float(tau_min), budget, mode,
                                          _floats(v["vp"]), _floats(v["planes"].reshape(-1)), float(v["rs"]), *o, cap,
                                          C.c_void_p(tmp), C.byref(n), C.byref(n_all), C.byref(tau), C.byref(cst),
                                          _stream(), 0), kind)
        return (n.value, n_all.value, bs.bits(tau.value), cst.value), [(0, n.value)]
    V, culled = len(vs), kind == "views_culled"
    n, n_all, offs, need = (C.c_int32 * V)(), (C.c_int32 * V)(), (C.c_int32 * V)(), C.c_int64(0)
    _lib.check(lib.hgs_lod_cut_views(p(f.nodes), p(f.boxes), p(f.bounds) if culled else None, f.N, V,
                                     _floats([x["tau"] for x in vs]), _floats([c for x in vs for c in x["vp"]]),
                                     _floats([c for x in vs for c in x["planes"].reshape(-1)]) if culled else None,
                                     _floats([x["rs"] for x in vs]), *o, cap, C.c_void_p(tmp), n, n_all, offs,
                                     C.byref(need), _stream(), 0), kind)
    return (tuple(n), tuple(n_all), tuple(offs), need.value), list(zip(offs, n))


def _capacity(kind, refs, views):
    """Entries the outputs must hold, exactly: the cut (views: up to the last view's end); a budget call's outputs hold
    ``budget`` entries, which its C call insists on."""
    if kind.startswith("budget"):
        return _budget_of(*views[0], kind.split("_")[1])[1]
    return sum((r.n + 3) // 4 * 4 for r in refs[:-1]) + refs[-1].n


def _segments(bufs, segs, nout):
    """The bytes the call wrote, view by view (the padding between two views belongs to nobody)."""
    torch.cuda.synchronize()
    return [bufs[k][4 * o:4 * (o + n)].clone() for o, n in segs for k in range(nout)]


def _assert_is_python_result(kind, got, refs):
    nout = 3 if kind.startswith("expand") else 5
    assert len(got) == nout * len(refs)
    for k, r in enumerate(refs):
        for j, fld in enumerate(FIELDS[:nout]):
            assert torch.equal(got[nout * k + j], getattr(r, fld).contiguous().view(torch.uint8)), (kind, k, fld)


def _views_of(kind, first=True):
    if kind.startswith("views"):
        return [("B", 3.0), ("O", 15.0), ("C", -0.5)] if first else [("O", 15.0), ("C", 3.0), ("B", 15.0)]
    return [("B", 3.0)] if first else [("O", 15.0)]


@pytest.mark.parametrize("kind", KINDS)
def test_an_uninitialised_workspace_is_enough(gpu, kind):
    """Through the C ABI: outputs of exactly the needed entries and the workspace at exactly its *_tmp_bytes, each between
    two guards, the free bytes filled once with 0x00 and once with 0xFF: intact guards, the two results bit-equal and
    equal to the Python-level call.  This is the first size at which the initial bytes of ``chain`` can matter: with one
    chunk nobody looks back, so nobody reads it; here the second chunk spins on chain[0] until its valid bit is set, and
    0xFF bytes ARE a valid word with a total of 2^32 - 1 unless the kernel in front of the scan cleared them."""
    import ws_guard as wg
    views = _views_of(kind)
    refs = _python_call(kind, views)
    assert all(r.n > 0 for r in refs)
    nout = 3 if kind.startswith("expand") else 5
    cap = _capacity(kind, refs, views)
    results = []
    for fill in (0x00, 0xFF):
        gs = [wg.guarded(4 * cap, gpu, fill, FIELDS[k]) for k in range(5)]
        tmp = wg.guarded(_tmp_bytes(kind, len(views)), gpu, fill, "tmp")
        words, segs = _abi_call(kind, views, [g.addr for g in gs], cap, tmp.addr)
        wg.check(*gs, tmp)
        got = _segments([g.body for g in gs], segs, nout)
        _assert_is_python_result(kind, got, refs)
        assert [n for _, n in segs] == [r.n for r in refs]
        if not kind.startswith("expand"):
            unculled = words[1] if kind.startswith("views") else (words[1],)
            assert list(unculled) == [r.n_unculled for r in refs]
        if kind.startswith("budget"):
            assert words[2:] == (bs.bits(refs[0].tau), refs[0].cost)
        results.append((words, got))
    assert results[0][0] == results[1][0]
    assert all(torch.equal(a, b) for a, b in zip(results[0][1], results[1][1]))


@pytest.mark.parametrize("kind", [k for k in KINDS if not k.startswith("expand")] + ["views_16_then_3"])
def test_one_workspace_call_after_call(gpu, kind):
    """Through the C ABI on ONE workspace: a view, another view, the first again.  The chain then holds the valid totals
    of the call before -- those of another cut -- when a call starts: the third result is the first bit for bit, the
    second is what a fresh workspace gives.  cut_views runs 16 views, then 3 on the workspace sized for 16 (its sums and
    chains then lie elsewhere in the same bytes), then the 16 again."""
    if kind == "views_16_then_3":
        kind, first, second = "views_culled", _cycled(16), _views_of("views_culled", first=False)
    else:
        first, second = _views_of(kind), _views_of(kind, first=False)
    nout = 5
    tmp = torch.full((_tmp_bytes(kind, max(len(first), len(second))),), 0xFF, dtype=torch.uint8, device=gpu)

    def run(views, tmp):
        refs = _python_call(kind, views)
        cap = _capacity(kind, refs, views)
        bufs = [torch.full((4 * cap,), 0xFF, dtype=torch.uint8, device=gpu) for _ in range(nout)]
        words, segs = _abi_call(kind, views, [b.data_ptr() for b in bufs], cap, tmp.data_ptr())
        got = _segments(bufs, segs, nout)
        _assert_is_python_result(kind, got, refs)
        return words, got

    a = run(first, tmp)
    b = run(second, tmp)
    c = run(first, tmp)
    fresh = run(second, torch.full((_tmp_bytes(kind, len(second)),), 0xFF, dtype=torch.uint8, device=gpu))
    for x, y in ((a, c), (b, fresh)):
        assert x[0] == y[0]
        assert len(x[1]) == len(y[1]) and all(torch.equal(s, t) for s, t in zip(x[1], y[1]))
