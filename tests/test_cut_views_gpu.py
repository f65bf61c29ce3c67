"""GPU parity of the cut for several views (csrc/lod_views.hip, hgs.frustum.cut_views): every view of one call against
hgs.frustum.cut_view on its single-pass route, bit for bit, and against tests/frustum_spec.py; the packed layout of the
shared outputs; buffer discipline through the C ABI; refusals; determinism."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import budget_cut_cases as bc
import frustum_cases as fc
import frustum_spec as fs
import ws_guard as wg
from hgs import _lib, hierarchy, synth

pytestmark = pytest.mark.gpu

LEAVES = (1, 2, 3, 33, 128, 129, 1000, 20000)       # N = 2 P - 1 nodes: 1, 3, 5, 65, 255, 257, 1999, 39999
FIELDS = ("render_indices", "parent_indices", "node_indices", "weights", "kids")
AWAY = ((0.0, 0.0, -50.0), 180.0)                    # a camera behind the scene that looks away from it
SENTINEL = -7


@functools.lru_cache(maxsize=None)
def _case(P):
    """(Hierarchy on the CPU, nodes, boxes on the GPU, bounds made on the GPU)."""
    from hgs import frustum
    from hgs.frustum import cull_bounds
    assert hasattr(frustum, "cut_views"), "hgs.frustum has no cut_views"
    h = fc.hier20k()[0] if P == 20000 else hierarchy.build_hierarchy(synth.make_scene(P, synth.make_camera(fc.W, fc.H), seed=2))
    dev = torch.device("cuda:0")
    nodes, boxes = h.nodes.to(dev), h.boxes.to(dev)
    means, scales = h.xyz.to(dev).contiguous(), torch.exp(h.log_scales).to(dev).contiguous()
    return h, nodes, boxes, cull_bounds(nodes, means, scales)


def _view(cam, tau_px):
    """One view's arguments: dict(tau, vp [3], planes [5,4], rs) of a camera (a name of frustum_cases, or a camera)."""
    from hgs.frustum import frustum_planes
    cam = fc.camera(cam) if isinstance(cam, str) else cam
    planes, rs = frustum_planes(cam.world_view_transform, cam.tanfovx, cam.tanfovy, fc.W, fc.H)
    return dict(tau=fc.tau_of(cam, tau_px), vp=cam.camera_center.clone(), planes=planes, rs=rs)


@functools.lru_cache(maxsize=None)
def _eight():
    """The eight views of the equality test: cameras A, B, C at 3 and 40 px, tau = 0 from B, tau at 10^6 px from C."""
    return tuple(_view(n, t) for n in "ABC" for t in fc.TAUS_PX) + (_view("B", -0.5), _view("C", 1e6))


def _call(nodes, boxes, bounds, views, **kw):
    from hgs.frustum import cut_views
    return cut_views(nodes, boxes, bounds, [v["tau"] for v in views], torch.stack([v["vp"] for v in views]),
                     torch.stack([v["planes"] for v in views]), [v["rs"] for v in views], **kw)


def _single(nodes, boxes, bounds, v):
    from hgs.frustum import cut_view
    return cut_view(nodes, boxes, bounds, v["tau"], v["vp"], v["planes"], v["rs"], nested=True)


def _np(t):
    return t.cpu().numpy()


def _bits(cv):
    """Everything of a CutView as comparable host data (weights as uint32)."""
    return (cv.n, cv.n_unculled) + tuple(_np(getattr(cv, f)).view(np.uint32 if f == "weights" else np.int32)
                                         for f in FIELDS)


def _assert_same(a, b, what=""):
    a, b = (x if isinstance(x, tuple) else _bits(x) for x in (a, b))
    assert a[:2] == b[:2], (what, a[:2], b[:2])
    for f, x, y in zip(FIELDS, a[2:], b[2:]):
        assert x.shape == y.shape and np.array_equal(x, y), (what, f)


def _assert_equals_spec(cv, spec, what=""):
    assert (cv.n, cv.n_unculled) == (spec["n"], spec["n_unculled"]), what
    for f in FIELDS[:3] + ("kids",):
        assert np.array_equal(_np(getattr(cv, f)), spec[f]), (what, f)
    assert np.array_equal(_np(cv.weights).view(np.uint32), spec["weights"].view(np.uint32)), what


@pytest.mark.parametrize("P", LEAVES)
def test_every_view_equals_cut_view_and_the_spec(gpu, P):
    h, nodes, boxes, bounds = _case(P)
    views = _eight()
    cuts = _call(nodes, boxes, bounds, views)
    assert len(cuts) == 8
    culled_something = False
    for k, (v, cv) in enumerate(zip(views, cuts)):
        _assert_same(cv, _single(nodes, boxes, bounds, v), f"view {k}")
        culled_something |= cv.n < cv.n_unculled
        if P <= 1000:
            spec = fs.cut_view_spec(h.nodes.numpy(), h.boxes.numpy(), _np(bounds), v["tau"], v["vp"].numpy(),
                                    v["planes"].numpy(), v["rs"])
            _assert_equals_spec(cv, spec, f"view {k}")
    assert cuts[6].n_unculled == P                      # tau = 0: every leaf
    assert cuts[7].n_unculled < cuts[5].n_unculled or P < 3     # 10^6 px: only what the camera is inside of is opened
    assert culled_something or P < 1000


@pytest.mark.parametrize("P", [3, 129, 20000])
def test_without_planes_every_view_is_expand_to_size(gpu, P):
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    from hgs.frustum import cut_views
    h, nodes, boxes, bounds = _case(P)
    views = _eight()
    cuts = cut_views(nodes, boxes, None, [v["tau"] for v in views], torch.stack([v["vp"] for v in views]))
    N = nodes.shape[0]
    ri = torch.zeros(N, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(N, device=gpu); ns = torch.zeros(N, dtype=torch.int32, device=gpu)
    for v, cv in zip(views, cuts):
        n = expand_to_size(nodes, boxes, v["tau"], v["vp"].to(gpu), torch.zeros(3), ri, pi, ni)
        get_interpolation_weights(ni[:n], v["tau"], nodes, boxes, v["vp"], torch.zeros(3), w, ns)
        assert cv.n == cv.n_unculled == n
        assert torch.equal(cv.render_indices, ri[:n]) and torch.equal(cv.parent_indices, pi[:n])
        assert torch.equal(cv.node_indices, ni[:n]) and torch.equal(cv.kids, ns[:n])
        assert np.array_equal(_np(cv.weights).view(np.uint32), _np(w[:n]).view(np.uint32))


@pytest.mark.parametrize("P", [129, 1000])
def test_a_view_does_not_depend_on_its_place_or_its_company(gpu, P):
    """V = 1 per view is the reference; the same views permuted, and 16, 17 and 20 views (the eight cycled: 17 and 20 go
    through the grouping by 16) give every view the same bits."""
    h, nodes, boxes, bounds = _case(P)
    views = _eight()
    alone = [_bits(_call(nodes, boxes, bounds, [v])[0]) for v in views]
    for k, v in enumerate(views):
        _assert_same(alone[k], _single(nodes, boxes, bounds, v), f"alone {k}")
    for order in ([5, 2, 7, 0, 6, 3, 1, 4], [k % 8 for k in range(16)], [k % 8 for k in range(17)],
                  [(3 * k + 1) % 8 for k in range(20)]):
        cuts = _call(nodes, boxes, bounds, [views[k] for k in order])
        assert len(cuts) == len(order)
        at = 0
        for place, (k, cv) in enumerate(zip(order, cuts)):
            _assert_same(cv, alone[k], f"{len(order)} views, place {place}")
            assert cv.render_indices.storage_offset() == at     # the offsets continue across the groups
            at += (cv.n + 3) // 4 * 4


def _sentinel_buffers(cap, gpu):
    from hgs.frustum import CutBuffers
    out = CutBuffers(cap, gpu)
    for t in (out.ri, out.pi, out.ni, out.ns):
        t.fill_(SENTINEL)
    out.w.fill_(float(SENTINEL))
    return out


@pytest.mark.parametrize("P", [129, 1000])
def test_views_are_packed_on_16_bytes_and_nothing_else_is_written(gpu, P):
    h, nodes, boxes, bounds = _case(P)
    eight = _eight()
    views = [eight[0], eight[2], _view(fc.yaw_camera(*AWAY), 3.0), eight[3], eight[6], eight[7], eight[4]]
    refs = [_single(nodes, boxes, bounds, v) for v in views]
    assert refs[2].n == 0 and refs[2].n_unculled > 0          # the middle view faces away: an empty segment
    assert any(r.n % 4 for r in refs[:-1])                    # and some offset needs rounding
    cap = sum((r.n + 3) // 4 * 4 for r in refs) + 37
    out = _sentinel_buffers(cap, gpu)
    cuts = _call(nodes, boxes, bounds, views, out=out)
    torch.cuda.synchronize()
    written = torch.zeros(cap, dtype=torch.bool, device=gpu)
    at = 0
    for k, (cv, ref) in enumerate(zip(cuts, refs)):
        _assert_same(cv, ref, f"view {k}")
        for f, buf in zip(FIELDS, (out.ri, out.pi, out.ni, out.w, out.ns)):
            t = getattr(cv, f)
            assert t.storage_offset() == at and t.numel() == cv.n
            assert cv.n == 0 or t.data_ptr() == buf.data_ptr() + 4 * at                  # a slice of `out`
        assert at % 4 == 0
        written[at:at + cv.n] = True
        at += (cv.n + 3) // 4 * 4
    for buf in (out.ri, out.pi, out.ni, out.ns):
        assert bool((buf[~written] == SENTINEL).all())
    assert bool((out.w[~written] == float(SENTINEL)).all())
    assert int((~written).sum()) >= 37


def test_nodes_of_several_rows(gpu):
    """The hand-built node list of frustum_cases.multi_row_case() inside nested boxes (budget_cut_cases.multi_row):
    counts above 1, a node without rows, offsets that need rounding, a view that keeps nothing."""
    nodes_h, boxes_h, bounds_h, _, _ = bc.multi_row()
    nodes, boxes, bounds = (torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (nodes_h, boxes_h, bounds_h))
    for names in ((("A", 40.0), ("A", 80.0)), (("A", 80.0), ("B", 40.0), ("A", 40.0), ("A", 20.0))):
        views = [_view(n, t) for n, t in names]
        cuts = _call(nodes, boxes, bounds, views)
        at = 0
        for (name, px), v, cv in zip(names, views, cuts):
            spec = fs.cut_view_spec(nodes_h, boxes_h, bounds_h, v["tau"], v["vp"].numpy(), v["planes"].numpy(), v["rs"])
            _assert_equals_spec(cv, spec, f"{name} {px}")
            _assert_same(cv, _single(nodes, boxes, bounds, v), f"{name} {px}")
            assert cv.render_indices.storage_offset() == at
            at += (cv.n + 3) // 4 * 4
        by_name = dict(zip(names, cuts))
        assert by_name["A", 40.0].n == 10 and by_name["A", 80.0].n == 3          # 10 -> 12, 3 -> 4: rounded offsets
        assert int(np.bincount(_np(by_name["A", 40.0].node_indices)).max()) > 1   # several entries of one node
        if ("B", 40.0) in by_name:
            assert by_name["B", 40.0].n == 0 and by_name["B", 40.0].n_unculled == 9


def _abi_call(nodes, boxes, bounds, views, outs, cap, tmp):
    """hgs_lod_cut_views on raw addresses -> (rc, counts, unculled, offsets, needed)."""
    lib, p, V = _lib.lib(), _lib.ptr, len(views)
    fl = lambda xs: (C.c_float * len(xs))(*[float(x) for x in xs])
    n, n_all, offs, need = (C.c_int32 * V)(), (C.c_int32 * V)(), (C.c_int32 * V)(), C.c_int64(0)
    rc = lib.hgs_lod_cut_views(p(nodes), p(boxes), p(bounds), int(nodes.shape[0]), V, fl([v["tau"] for v in views]),
                               fl([x for v in views for x in v["vp"]]),
                               fl([x for v in views for x in v["planes"].reshape(-1)]), fl([v["rs"] for v in views]),
                               *[C.c_void_p(a) for a in outs], cap, C.c_void_p(tmp), n, n_all, offs, C.byref(need),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream), 0)
    return rc, list(n), list(n_all), list(offs), need.value


@pytest.mark.parametrize("V", [1, 3, 16])
@pytest.mark.parametrize("P", [129, 1000])
def test_outputs_and_workspace_stay_inside_their_bytes(gpu, P, V):
    """Every output at exactly the needed entries and the workspace at exactly hgs_lod_cut_views_tmp_bytes, each between
    two guards, free bytes filled once with 0x00 and once with 0xFF: intact guards, the bits of the unguarded run.  Then
    one entry too few: the call fails naming the count, the guards hold, and the next call with room is right."""
    h, nodes, boxes, bounds = _case(P)
    eight = _eight()
    views = [eight[(5 * k + 4) % 8] for k in range(V)]          # C at 3 px first: it culls and keeps something
    refs = [_single(nodes, boxes, bounds, v) for v in views]
    offs_ref = [sum((r.n + 3) // 4 * 4 for r in refs[:k]) for k in range(V)]
    needed = offs_ref[-1] + refs[-1].n
    assert 0 < refs[0].n < refs[0].n_unculled
    N = int(nodes.shape[0])
    tmp_bytes = _lib.lib().hgs_lod_cut_views_tmp_bytes(N, V)
    keys = ("ri", "pi", "ni", "w", "ns")

    def check_results(gs):
        for k, r in enumerate(refs):
            lo, hi = 4 * offs_ref[k], 4 * (offs_ref[k] + r.n)
            for key, f in zip(keys, FIELDS):
                assert torch.equal(gs[key].body[lo:hi], getattr(r, f).contiguous().view(torch.uint8)), (k, key)

    for fill in (0x00, 0xFF):
        gs = {k: wg.guarded(4 * needed, gpu, fill, k) for k in keys}
        gs["tmp"] = wg.guarded(tmp_bytes, gpu, fill, "tmp")
        rc, n, n_all, offs, need = _abi_call(nodes, boxes, bounds, views, [gs[k].addr for k in keys], needed, gs["tmp"].addr)
        wg.check(*gs.values())
        assert rc == 0, _lib.lib().hgs_last_error()
        assert (n, n_all, offs, need) == ([r.n for r in refs], [r.n_unculled for r in refs], offs_ref, needed)
        check_results(gs)
        for k in range(V - 1):                                  # the padding between two views is not written
            lo, hi = 4 * (offs_ref[k] + refs[k].n), 4 * offs_ref[k + 1]
            assert bool((gs["ri"].body[lo:hi] == fill).all())
    # one entry too few
    gs = {k: wg.guarded(4 * (needed - 1), gpu, 0xFF, k) for k in keys}
    gs["tmp"] = wg.guarded(tmp_bytes, gpu, 0xFF, "tmp")
    rc, n, n_all, offs, need = _abi_call(nodes, boxes, bounds, views, [gs[k].addr for k in keys], needed - 1, gs["tmp"].addr)
    wg.check(*gs.values())
    assert rc != 0 and (n, offs, need) == ([r.n for r in refs], offs_ref, needed)
    with pytest.raises(_lib.HgsError, match=rf"{needed} entries exceed the output capacity {needed - 1}\b"):
        _lib.check(rc, "hgs_lod_cut_views")
    gs = {k: wg.guarded(4 * needed, gpu, 0xFF, k) for k in keys}
    gs["tmp"] = wg.guarded(tmp_bytes, gpu, 0xFF, "tmp")
    rc, n, n_all, offs, need = _abi_call(nodes, boxes, bounds, views, [gs[k].addr for k in keys], needed, gs["tmp"].addr)
    wg.check(*gs.values())
    assert rc == 0 and n == [r.n for r in refs]
    check_results(gs)


def test_buffers_that_are_too_small(gpu):
    """Through Python: ``out`` one entry short raises HgsError naming the count and writes nothing behind ``out``'s
    end; without ``out`` the buffers are allocated to fit, also where max(N, 1) entries are not enough."""
    from hgs.frustum import CutBuffers
    h, nodes, boxes, bounds = _case(1000)
    views = [_eight()[k % 8] for k in range(20)]
    cuts = _call(nodes, boxes, bounds, views)                   # 20 views of up to 1000 entries in 1999: the retry
    needed = cuts[-1].render_indices.storage_offset() + cuts[-1].n
    assert needed > nodes.shape[0]
    for k, (v, cv) in enumerate(zip(views, cuts)):
        _assert_same(cv, _single(nodes, boxes, bounds, v), f"view {k}")
    with pytest.raises(_lib.HgsError, match=rf"{needed} entries exceed the output capacity {needed - 1}\b"):
        _call(nodes, boxes, bounds, views, out=CutBuffers(needed - 1, gpu))
    exact = _call(nodes, boxes, bounds, views, out=CutBuffers(needed, gpu))
    for a, b in zip(exact, cuts):
        _assert_same(a, b)


def test_refusals(gpu):
    from hgs.frustum import CutBuffers, cut_views
    h, nodes, boxes, bounds = _case(1000)
    views = _eight()[:3]
    # a hierarchy made non-nested the way test_non_nested_hierarchy_takes_the_level_route does
    bad_boxes = boxes.clone()
    bad_boxes[int(h.nodes[-1, 1]), 0, 3] = 1e6
    with pytest.raises(ValueError, match="boxes nest"):
        _call(nodes, bad_boxes, bounds, views)
    taus = [v["tau"] for v in views]
    vps = torch.stack([v["vp"] for v in views])
    planes = torch.stack([v["planes"] for v in views])
    rss = [v["rs"] for v in views]
    args = dict(nodes=nodes, boxes=boxes, bounds=bounds, taus=taus, viewpoints=vps, planes=planes, radius_scales=rss)
    assert len(cut_views(**args)) == 3
    for key, bad in (("taus", taus[:2]), ("viewpoints", vps[:2]), ("viewpoints", torch.zeros(3, 4)), ("planes", planes[:2]),
                     ("planes", planes[:, :4]), ("planes", [planes[0], planes[1]]), ("planes", [planes[0], planes[1], planes[2][:4]]),
                     ("radius_scales", rss[:2]), ("planes", None), ("bounds", None), ("nodes", nodes.cpu()),
                     ("nodes", nodes.long()), ("boxes", boxes.double()), ("bounds", bounds.half()), ("nodes", nodes[:, :6]),
                     ("boxes", boxes[:-1]), ("bounds", bounds[:-1]), ("bounds", bounds[:, :3]),
                     ("bounds", bounds.t().contiguous().t())):
        with pytest.raises(ValueError):
            cut_views(**dict(args, **{key: bad}))
    odd = CutBuffers(4000, gpu)
    odd.w = odd.w.double()
    with pytest.raises(ValueError):
        cut_views(**args, out=odd)
    seq = cut_views(**dict(args, planes=[planes[0], planes[1], planes[2]]))      # a sequence of [5,4] is fine
    for a, b in zip(seq, cut_views(**args)):
        _assert_same(a, b)
    assert cut_views(nodes, boxes, None, [], torch.zeros(0, 3)) == []


def test_two_calls_and_two_streams_give_the_same_bits(gpu):
    h, nodes, boxes, bounds = _case(20000)
    views = _eight()
    ref = [_bits(cv) for cv in _call(nodes, boxes, bounds, views)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=gpu) for _ in range(2)]
    runs = []
    for rep in range(2):
        for s in streams:
            with torch.cuda.stream(s):
                runs.append(_call(nodes, boxes, bounds, views))
    torch.cuda.synchronize()
    for cuts in runs:
        for k, cv in enumerate(cuts):
            _assert_same(cv, ref[k], f"view {k}")
