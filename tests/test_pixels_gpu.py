"""hgs_raster_pixels on the GPU: against the float64 spec (tests/pixels_spec.py), against K6's own per-pixel words,
against f-22 on the same forward, and the Python layers built on it.

On non-fragile pixels ``count``, ``front`` and ``back`` are EQUAL to the spec (the fragile share must stay under
parity.FRAGILE_FRAC -- a condition).  Near-ties of the heaviest row and of the median are verified, not excluded, with
``b_w = MIXED_REL w + MIXED_ABS (largest weight of the image)`` and ``b_T = MIXED_REL 0.5 + MIXED_ABS``: the device's
choice must be one the spec allows within the bound, and where the spec's decision is clear by twice the bound the id
must be the spec's.  The pixels on the loose branch are at most 1e-3 of those with a row / a median (a condition; the
float64 oracle has 0 heaviest near-ties on the eight cases and one median near-tie, of 3 340, on ``edge_tiles_b``)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import contribution_cases as cc
import parity as pa
import pixels_spec as ps
import ws_guard as wg
from hgs import _lib, synth

pytestmark = pytest.mark.gpu

PLANES = _lib.PIXEL_PLANES
ID_PLANES = ("front", "back", "heaviest", "median")
FLOAT_PLANES = ("alpha", "wmax", "median_depth")
LOOSE_FRAC = 1e-3


def _forward(gpu, cam, scene):
    """(settings, attribute tensors on the GPU) of the plain rows on the product path."""
    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(cam, torch.zeros(3), scene.sh_degree, do_depth=False,
                                                                device=gpu))
    s = scene.to(gpu)
    return rs, dict(means3D=s.means3D, opacities=s.opacities, shs=s.shs, scales=s.scales, rotations=s.rotations)


def _read(gpu, cam, scene, **kw):
    from hgs.picking import read_view
    rs, att = _forward(gpu, cam, scene)
    r, call = read_view(rs, **att, **kw)
    torch.cuda.synchronize()
    return r, call


def _flat(r):
    return {name: getattr(r, name).cpu().numpy().reshape(-1) for name in PLANES if getattr(r, name) is not None}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, names=PLANES):
    return all(torch.equal(_bits(getattr(a, n)), _bits(getattr(b, n))) for n in names)


# ---- against the spec ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.CASES))
def test_planes_match_the_spec(gpu, name):
    from diff_gaussian_rasterization import _C
    cam, scene, view, spec = ps.case(name)
    frag = view.out.fragile.reshape(-1)
    assert frag.mean() <= pa.FRAGILE_FRAC, f"fragile share {frag.mean():.2e}"
    ok = ~frag
    r, call = _read(gpu, cam, scene)
    assert (r.H, r.W) == (cam.image_height, cam.image_width)
    for p in PLANES:
        t = getattr(r, p)
        assert t.shape == (r.H, r.W) and t.dtype == (torch.float32 if p in FLOAT_PLANES else torch.int32)
    d = _flat(r)
    for p, ref in (("count", spec.n), ("front", spec.front), ("back", spec.back)):
        assert np.array_equal(d[p][ok], ref[ok]), (name, p, int((d[p][ok] != ref[ok]).sum()))
    # the heaviest row: one the spec weighs within b_w of its maximum; the spec's own where the runner-up is clear
    big = spec.wmax.max()
    b_w = pa.MIXED_REL * spec.wmax + pa.MIXED_ABS * big
    has = ok & (spec.n > 0)
    assert bool((d["heaviest"][has] >= 0).all()) and bool((d["heaviest"][ok & (spec.n == 0)] == -1).all())
    w_dev, _, _ = spec.of_row(d["heaviest"])
    assert not np.isnan(w_dev[has]).any(), "a heaviest row the spec does not blend at its pixel"
    assert bool((spec.wmax[has] - w_dev[has] <= b_w[has]).all())
    assert bool((np.abs(d["wmax"].astype(np.float64) - spec.wmax)[ok] <= b_w[ok]).all())
    clear = has & (spec.wmax - spec.second > 2.0 * b_w)
    assert np.array_equal(d["heaviest"][clear], spec.heaviest[clear])
    loose_w = int((has & ~clear).sum())
    # the median row: T crosses one half at it within b_T; the spec's own (or none) where no T of the pixel is near
    b_T = pa.MIXED_REL * 0.5 + pa.MIXED_ABS
    hm = ok & (d["median"] != -1)
    _, tb, ta = spec.of_row(d["median"])
    assert not np.isnan(ta[hm]).any(), "a median row the spec does not blend at its pixel"
    assert bool((ta[hm] < 0.5 + b_T).all()) and bool((tb[hm] >= 0.5 - b_T).all())
    nm = ok & (d["median"] == -1)
    assert bool(((1.0 - spec.alpha)[nm] >= 0.5 - b_T).all())
    clear_T = ok & (spec.t_gap > 2.0 * b_T)
    assert np.array_equal(d["median"][clear_T], spec.median[clear_T])
    loose_T = int((ok & ~clear_T).sum())
    n_med = int((spec.median != -1).sum())
    print(f"{name}: {int(frag.sum())} fragile of {frag.size}; loose heaviest {loose_w} of {int(has.sum())}, "
          f"loose median {loose_T} of {n_med}")
    assert loose_w <= LOOSE_FRAC * has.sum() and loose_T <= LOOSE_FRAC * max(n_med, 1)
    # the depth is the one K1 stored for the median row, bit for bit; zero bits where there is none
    depths = _C.raster_views(call)["depths"]
    med = r.median.reshape(-1).long()
    want = torch.where(med >= 0, _bits(depths)[med.clamp(min=0)], torch.zeros_like(med, dtype=torch.int32))
    assert torch.equal(_bits(r.median_depth).reshape(-1), want)
    none = r.count == 0
    for p in ID_PLANES:
        assert bool((getattr(r, p)[none] == -1).all())
    assert not bool(_bits(r.wmax)[none].any()) and not bool(_bits(r.alpha)[none].any())
    if name == "long_lists":
        assert int((view.out.final_T < 1e-2).sum()) > 1000 and int(spec.n.max()) > 64      # saturated pixels, several batches
    if name == "opaque_stack":
        assert int((spec.median != -1).sum()) > 50
    if name == "big_rows":
        assert int((view.out.geom.tiles_touched[:3] > 64).sum()) == 3


# ---- against K6 itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.CASES) + ["centred_row"])
def test_the_walk_repeats_k6s_decisions_on_every_pixel(gpu, name):
    """Exact on every pixel, the fragile ones included: the planes against the two words K6 itself kept."""
    from diff_gaussian_rasterization import _C
    cam, scene, _, _ = ps.case(name)
    r, call = _read(gpu, cam, scene)
    v = _C.raster_views(call)
    fT, nc = v["final_T"], v["n_contrib"].long()
    assert torch.equal(_bits(r.alpha), _bits(1.0 - fT))
    assert torch.equal(r.count == 0, nc == 0)
    assert bool((r.count.long() <= nc).all())
    H, W = r.H, r.W
    ys, xs = torch.meshgrid(torch.arange(H, device=gpu), torch.arange(W, device=gpu), indexing="ij")
    tile = (ys // 16) * ((W + 15) // 16) + xs // 16
    some = nc > 0
    last = v["point_list"].long()[(v["ranges"][:, 0].long()[tile] + nc - 1)[some]]
    assert torch.equal(r.back.long()[some], last)
    assert int(some.sum()) > 0


# ---- against f-22 on the same forward ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_tiles_b", "long_lists", "big_rows"])
def test_planes_agree_with_the_contribution_scores_of_the_same_forward(gpu, name):
    from diff_gaussian_rasterization import _C
    from hgs.importance import Scores
    cam, scene, _, _ = ps.case(name)
    r, call = _read(gpu, cam, scene)
    sc = Scores.zeros(scene.P, gpu)
    _C.raster_contributions(call, sc.wmax, sc.wsum, sc.count)
    torch.cuda.synchronize()
    assert int(r.count.sum()) == int(sc.count.sum()) > 0
    assert torch.equal(_bits(r.wmax.max()), _bits(sc.wmax.max()))
    some = r.heaviest >= 0
    assert bool((r.wmax[some] <= sc.wmax[r.heaviest[some].long()]).all())


# ---- a row centred on a pixel --------------------------------------------------------------------------------------------
def test_centred_opaque_row_is_front_heaviest_and_median_of_its_pixel(gpu):
    from diff_gaussian_rasterization import _C
    from hgs.picking import world_points
    cam, scene, _, _ = ps.case("centred_row")
    r, call = _read(gpu, cam, scene)
    x, y = 10, 12
    assert (int(r.front[y, x]), int(r.heaviest[y, x]), int(r.median[y, x])) == (0, 0, 0)
    depths = _C.raster_views(call)["depths"]
    assert torch.equal(_bits(r.median_depth[y, x]), _bits(depths[0]))
    got = world_points(r, cam)[y, x].double().cpu()
    mean = scene.means3D[0].double()
    assert bool(((got - mean).abs() <= pa.MIXED_REL * mean.abs() + pa.MIXED_ABS).all()), (got, mean)
    assert bool(torch.isnan(world_points(r, cam)[r.median == -1]).all())


# ---- slot maps -----------------------------------------------------------------------------------------------------------
def test_slot_map_renames_ids_exactly_and_changes_no_float_bit(gpu):
    cam, scene, _, _ = ps.case("edge_tiles_a")
    P, S = scene.P, scene.P + 37
    base, _ = _read(gpu, cam, scene)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(S)[:P].astype(np.int32)).to(gpu)
    got, _ = _read(gpu, cam, scene, slot_of_row=perm, n_slots=S)
    assert _same_bits(base, got, FLOAT_PLANES + ("count",))
    for p in ID_PLANES:
        b, g = getattr(base, p), getattr(got, p)
        assert torch.equal(g, torch.where(b >= 0, perm[b.clamp(min=0).long()], b)), p
    # rows the map ignores (-1, or beyond n_slots) are named -2 where they win; they still occlude and count
    for slot in (torch.where(torch.arange(P, device=gpu) % 2 == 0, -1, S + 5).to(torch.int32),
                 torch.where(torch.arange(P, device=gpu) % 3 == 0, -1, torch.arange(P, device=gpu)).to(torch.int32)):
        got, _ = _read(gpu, cam, scene, slot_of_row=slot, n_slots=S)
        assert _same_bits(base, got, FLOAT_PLANES + ("count",))
        for p in ID_PLANES:
            b, g = getattr(base, p), getattr(got, p)
            s = slot[b.clamp(min=0).long()]
            named = (s >= 0) & (s < S)
            assert torch.equal(g, torch.where(b < 0, b, torch.where(named, s, torch.full_like(s, -2)))), p
            assert int((g == -2).sum()) > 0
    # n_slots bounds the map: the default names every non-negative entry
    wide, _ = _read(gpu, cam, scene, slot_of_row=perm)
    narrow, _ = _read(gpu, cam, scene, slot_of_row=perm, n_slots=P)
    assert torch.equal(wide.front, torch.where(base.front >= 0, perm[base.front.clamp(min=0).long()], base.front))
    assert torch.equal(narrow.front, torch.where(wide.front >= P, torch.full_like(wide.front, -2), wide.front))
    assert int((narrow.front == -2).sum()) > 0


def test_want_subsets_give_the_bits_of_the_full_call(gpu):
    from diff_gaussian_rasterization import _C
    cam, scene, _, _ = ps.case("edge_tiles_b")
    full, call = _read(gpu, cam, scene)
    for want in [(p,) for p in PLANES] + [("median_depth", "count"), ("heaviest", "wmax", "alpha"), "front"]:
        got = _C.raster_pixels(call, want=want)
        names = (want,) if isinstance(want, str) else want
        assert set(got) == set(names)
        for p in names:
            assert torch.equal(_bits(got[p]), _bits(getattr(full, p))), (want, p)
    slot = torch.zeros(scene.P, dtype=torch.int32, device=gpu)
    for bad in (dict(slot_of_row=slot.long()), dict(slot_of_row=slot[:-1]), dict(slot_of_row=slot.cpu()),
                dict(slot_of_row=slot, n_slots=0), dict(n_slots=5), dict(want=("depth",)), dict(want=())):
        with pytest.raises(RuntimeError):
            _C.raster_pixels(call, **bad)


# ---- nothing to show -----------------------------------------------------------------------------------------------------
def _planes_through_the_abi(gpu, call, fill, args=None, slot=None, n_slots=0):
    """All eight planes between guard words, pre-filled with ``fill``, written by one hgs_raster_pixels call."""
    HW = call.H * call.W
    bufs = {p: wg.guarded(HW * 4, gpu, fill, p) for p in PLANES}
    planes = _lib.RasterPixelPlanes(**{p: b.addr for p, b in bufs.items()})
    rc = _lib.lib().hgs_raster_pixels(C.byref(call.args if args is None else args), call.p_geom, call.p_bin, call.p_img,
                                      call.L_ws, None if slot is None else C.c_void_p(slot.data_ptr()), n_slots,
                                      C.byref(planes), C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream),
                                      gpu.index or 0)
    _lib.check(rc, "hgs_raster_pixels")
    wg.check(*bufs.values())
    return {p: b.view(torch.int32).clone() for p, b in bufs.items()}


def _assert_nothing(got):
    for p in PLANES:
        assert bool((got[p] == (-1 if p in ID_PLANES else 0)).all()), p


def test_nothing_visible_fills_every_plane_with_the_nothing_values(gpu):
    from diff_gaussian_rasterization import _C
    cam, scene, _, _ = pa.default_case(100, 40, 30, 3)
    scene.means3D[:, 2] = -scene.means3D[:, 2]                 # behind the camera
    r, call = _read(gpu, cam, scene)
    assert call.L == 0
    _assert_nothing({p: _bits(getattr(r, p)) for p in PLANES})
    for fill in (0x00, 0xFF):
        _assert_nothing(_planes_through_the_abi(gpu, call, fill))
    # P == 0 through the ABI on a frame that does show rows: no workspace is read, the planes say nothing
    cam, scene, _, _ = ps.case("5x3")
    r, call = _read(gpu, cam, scene)
    assert int(r.count.sum()) > 0
    a = _lib.RasterArgs.from_buffer_copy(call.args)
    a.P = 0
    _assert_nothing(_planes_through_the_abi(gpu, call, 0xFF, args=a))


# ---- guards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1x1", "5x3", "edge_tiles_a"])
@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_planes_stay_inside_their_buffers_and_repeat_their_bits(gpu, name, fill):
    """H * W off the 64 and 256 grids: every plane exactly sized between guard words; two runs, and the glue's own
    buffers, give equal bits whatever the planes held before."""
    cam, scene, _, _ = ps.case(name)
    r, call = _read(gpu, cam, scene)
    a = _planes_through_the_abi(gpu, call, fill)
    b = _planes_through_the_abi(gpu, call, fill)
    for p in PLANES:
        assert torch.equal(a[p], b[p]) and torch.equal(a[p], _bits(getattr(r, p)).reshape(-1)), p
    P = scene.P
    slot = torch.arange(P, dtype=torch.int32, device=gpu).flip(0).contiguous()
    c = _planes_through_the_abi(gpu, call, fill, slot=slot, n_slots=P)
    assert torch.equal(c["front"], torch.where(a["front"] >= 0, P - 1 - a["front"], a["front"]))
    assert torch.equal(c["alpha"], a["alpha"]) and torch.equal(c["median_depth"], a["median_depth"])


# ---- the in-op LOD route -----------------------------------------------------------------------------------------------
def test_in_op_lod_route_equals_the_gathered_rows(gpu):
    """The cut of hier2000() at 3 px with 7 skybox rows behind it: the in-op LOD forward (default slot map: the cut's
    render_indices) against the plain forward of the same rows gathered by hand under an explicit slot map."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    from hgs.importance import activated, tau_of, view_cut
    from hgs.picking import read_view
    K = 7
    hd, cam = cc.on_device(cc.hier2000(), gpu), cc.camera()
    N = hd.num_nodes
    ri, pi, w, kids = view_cut(hd, cam, tau_of(3.0, cam.tanfovx, cam.image_width), frustum=False)
    n = int(ri.numel())
    assert 0 < n < N
    sky = synth.make_scene(K, cam, seed=77, s_px=(6.0, 20.0), z_range=(25.0, 40.0)).to(gpu)
    rows = activated(hd)
    full = {k: torch.cat((rows[k], getattr(sky, k))).contiguous() for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    gm, gs, gr, gsh, gop = _C.lod_gather(ri, pi, w, full["means3D"], full["scales"], full["rotations"], full["shs"],
                                         full["opacities"])
    tail = lambda a, b: torch.cat((a, b[N:])).contiguous()
    gathered = dict(means3D=tail(gm, full["means3D"]), shs=tail(gsh, full["shs"]), opacities=tail(gop, full["opacities"]),
                    scales=tail(gs, full["scales"]), rotations=tail(gr, full["rotations"]))
    wa = torch.cat((w, torch.ones(K, device=gpu)))
    ka = torch.cat((kids, torch.ones(K, dtype=torch.int32, device=gpu)))
    e_i = torch.empty(0, dtype=torch.int32, device=gpu)

    def settings(r, p, ww, kk):
        kw = pa.settings_kwargs(cam, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=ww, num_node_kids=kk)
        kw["render_indices"], kw["parent_indices"] = r, p
        return dgr.GaussianRasterizationSettings(**kw)

    slot = torch.cat((ri, torch.full((K,), -1, dtype=torch.int32, device=gpu)))
    a, _ = read_view(settings(ri.contiguous(), pi.contiguous(), w.contiguous(), kids.contiguous()), **full, n_slots=N,
                     skybox_points=K)
    b, call_b = read_view(settings(e_i, e_i, wa, ka), **gathered, slot_of_row=slot, n_slots=N)
    plain, _ = read_view(settings(e_i, e_i, wa, ka), **gathered)
    torch.cuda.synchronize()
    assert call_b.P == n + K
    assert _same_bits(a, b)
    # the ids are the cut's nodes: the plain readout's rows through render_indices, the skybox rows unnamed
    for p in ID_PLANES:
        rows_p, got = getattr(plain, p), getattr(a, p)
        assert torch.equal(got, torch.where(rows_p < 0, rows_p, torch.where(rows_p < n, slot[rows_p.clamp(min=0).long()],
                                                                             torch.full_like(rows_p, -2)))), p
    in_cut = torch.zeros(N, dtype=torch.bool, device=gpu)
    in_cut[ri.long()] = True
    named = a.front[a.front >= 0].long()
    assert bool(in_cut[named].all()) and named.unique().numel() > 100
    # the skybox lies behind the cut: where it is blended it is the last row, and it has no name
    assert int((a.back == -2).sum()) > 0, "the skybox must be on screen for the case to mean anything"
    assert not bool((a.front == -2).any())


# ---- end to end ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hier():
    return cc.on_device(cc.hier2000(), torch.device("cuda:0"))


def test_picked_rectangle_is_gone_from_the_front_after_the_prune(gpu):
    from hgs.hierarchy import prune_hierarchy_gpu
    from hgs.picking import leaves_below, node_depth_image, pick, read_hierarchy_view
    h, cam = _hier(), cc.camera()
    r = read_hierarchy_view(h, cam, tau_px=0.0)
    leaf = h.nodes[:, 6] == 0
    named = r.front[r.front >= 0].long()
    assert named.numel() > 300 and bool(leaf[named].all())              # at 0 px the cut is the leaves
    assert bool((node_depth_image(r.front, h.nodes)[r.front >= 0] > 0).all())
    ids = pick(r, (20, 14, 44, 34), which=("front",))
    assert 10 < ids.numel() < int(leaf.sum())
    mask = leaves_below(h.nodes, ids)
    assert mask.dtype == torch.uint8 and torch.equal(mask.nonzero().flatten(), ids)      # leaves mark themselves
    res = prune_hierarchy_gpu(h, remove=mask)
    again = read_hierarchy_view(res.hierarchy, cam, tau_px=0.0)
    torch.cuda.synchronize()
    front_old = res.old_of_new.long()[again.front[again.front >= 0].long()]
    assert front_old.numel() > 0 and not bool(mask.bool()[front_old].any())
    # a coarser cut names interior nodes, and the leaves below them are more than the nodes picked
    coarse = read_hierarchy_view(h, cam, tau_px=6.0, want=("front", "count"))
    assert coarse.alpha is None and coarse.median is None
    cid = pick(coarse, (20, 14, 44, 34))
    assert bool((~leaf[cid]).any()) and int(leaves_below(h.nodes, cid).sum()) > cid.numel()


def test_command_prints_the_pick_and_writes_the_mask_the_pruner_reads(gpu, tmp_path, capsys):
    import json
    from gaussian_hierarchy._C import write_hierarchy
    from hgs import pick_hierarchy as ph
    from hgs.picking import leaves_below, pick, read_hierarchy_view
    host = cc.hier2000()
    path, cams = tmp_path / "in.hier", tmp_path / "cameras.json"
    write_hierarchy(str(path), *[getattr(host, k) for k in cc.FIELDS])
    cams.write_text(json.dumps([cc.camera_entry(c) for c in cc.orbit(2)]))
    ids_out, mask_out, r_out = tmp_path / "ids.npy", tmp_path / "o" / "mask.npy", tmp_path / "r.npz"
    rc = ph.main([str(path), "--cameras", str(cams), "--camera", "1", "--rect", "10", "8", "30", "24", "--which", "front",
                  "--which", "median", "--ids-out", str(ids_out), "--mask-out", str(mask_out), "--readout-out", str(r_out)])
    out = capsys.readouterr().out
    assert rc == 0 and out.startswith("pick_hierarchy: N = 3999 nodes, camera 1 (64 x 48)")
    from hgs.score_hierarchy import read_cameras
    cam = read_cameras(str(cams))[1]
    h = _hier()
    r = read_hierarchy_view(h, cam)
    want = pick(r, (10, 8, 30, 24), ("front", "median"))
    ids = np.load(ids_out)
    assert ids.dtype == np.int64 and np.array_equal(ids, want.cpu().numpy()) and ids.size > 0
    assert np.array_equal(np.load(mask_out), leaves_below(h.nodes, want).cpu().numpy())
    z = np.load(r_out)
    assert set(z.files) == set(PLANES) | {"H", "W"} and np.array_equal(z["front"], r.front.cpu().numpy())
    lines = [l for l in out.splitlines() if l.startswith("node ")]
    assert len(lines) == min(ids.size, ph.MAX_LINES) and lines[0] == f"node {ids[0]} depth {int(h.nodes[ids[0], 0])}"
    # one pixel: its world point is printed and projects back into the pixel
    ys, xs = (r.median >= 0).nonzero(as_tuple=True)
    x, y = int(xs[0]), int(ys[0])
    rc = ph.main([str(path), "--cameras", str(cams), "--camera", "1", "--pixel", str(x), str(y), "--which", "median"])
    out = capsys.readouterr().out
    assert rc == 0 and f"node {int(r.median[y, x])} depth" in out
    p = torch.tensor([float(t) for t in out.splitlines()[-1].split(":")[1].split()] + [1.0], dtype=torch.float64)
    clip = p @ cam.full_proj_transform.double()
    px = ((clip[0] / clip[3] + 1.0) * cam.image_width - 1.0) * 0.5
    py = ((clip[1] / clip[3] + 1.0) * cam.image_height - 1.0) * 0.5
    assert abs(float(px) - x) < 1e-2 and abs(float(py) - y) < 1e-2          # (six printed digits)
