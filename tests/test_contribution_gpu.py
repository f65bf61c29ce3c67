"""hgs_raster_contrib on the GPU against the float64 spec (tests/contribution_spec.py).

Values within the project's element-wise bound ``1e-5 |ref| + 1e-6 max|ref|`` (parity.MIXED_REL / MIXED_ABS), ``count``
exact.  The pixel mask handed to the device is ``~oracle.fragile`` AND the case's own mask: on a knife-edge pixel a
float32 and a float64 evaluation may legitimately decide differently.  The fragile share must stay under
parity.FRAGILE_FRAC -- a condition, not a tolerance; the oracle reports no fragile pixel on any case below."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import contribution_cases as cc
import contribution_spec as cs
import parity as pa
import ws_guard as wg
from hgs import _lib, synth

pytestmark = pytest.mark.gpu

CAP = float(np.float32(0.99))       # the kernels' cap is the float32 constant: 0.9900000095


# ---- cases -------------------------------------------------------------------------------------------------------------
def _opaque_stack():
    cam, scene, _, _ = pa.default_case(200, 40, 24, 6)
    k = torch.arange(40, dtype=torch.float32)
    scene.means3D[:40] = torch.stack([torch.zeros(40), torch.zeros(40), 3.0 + 0.01 * k], 1)
    scene.scales[:40] = 0.15
    scene.opacities[:40] = 0.9
    scene.opacities[:8] = 1.0
    return cam, scene


def _centred_row():
    """Row 0: opacity 1, in front of everything (z = 1), centred on the centre of pixel (10, 12) of a 32 x 32 image."""
    cam, scene, _, _ = pa.default_case(50, 32, 32, 4)
    ndc = lambda p, n: (2.0 * p + 1.0) / n - 1.0
    scene.means3D[0] = torch.tensor([ndc(10, 32) * cam.tanfovx, ndc(12, 32) * cam.tanfovy, 1.0])
    scene.scales[0] = 0.05
    scene.opacities[0] = 1.0
    return cam, scene


def _big_rows():
    """Three rows that cover the whole 10 x 9 tile grid: runs of 90 instances, which the sum kernel adds up by the wave."""
    cam, scene, _, _ = pa.default_case(100, 160, 144, 7)
    scene.means3D[:3] = torch.tensor([[0.0, 0.0, 6.0], [0.5, -0.3, 9.0], [-0.4, 0.2, 12.0]])
    scene.scales[:3] = torch.tensor([[2.0, 1.5, 1.0], [3.0, 3.0, 3.0], [2.5, 4.0, 1.0]])
    scene.opacities[:3] = torch.tensor([[0.3], [0.5], [0.9]])
    return cam, scene


CASES = {
    "one_tile": lambda: pa.default_case(64, 16, 16, 3)[:2],
    "edge_tiles_a": lambda: pa.default_case(300, 70, 45, 0)[:2],
    "edge_tiles_b": lambda: pa.default_case(600, 130, 50, 2)[:2],
    "long_lists": lambda: pa.default_case(4000, 64, 64, 5)[:2],
    "opaque_stack": _opaque_stack,
    "1x1": lambda: pa.default_case(30, 1, 1, 9)[:2],
    "5x3": lambda: pa.default_case(40, 5, 3, 1)[:2],
    "big_rows": _big_rows,
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cam, scene, SpecView): the oracle runs once per case and is shared, unchanged, by every test."""
    cam, scene = (_centred_row if name == "centred_row" else CASES[name])()
    return cam, scene, cs.oracle_view(scene, cam)


def _forward(gpu, cam, scene):
    """(settings, attribute tensors on the GPU) of the plain rows on the product path."""
    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(cam, torch.zeros(3), scene.sh_degree, do_depth=False,
                                                                device=gpu))
    s = scene.to(gpu)
    return rs, dict(means3D=s.means3D, opacities=s.opacities, shs=s.shs, scales=s.scales, rotations=s.rotations)


def _score(gpu, cam, scene, S=None, **kw):
    from hgs.importance import Scores, score_view
    rs, att = _forward(gpu, cam, scene)
    scores = Scores.zeros(scene.P if S is None else S, gpu)
    call = score_view(scores, rs, **att, **kw)
    torch.cuda.synchronize()
    return scores, call


def _ok_mask(view, own=None):
    frag = view.out.fragile.reshape(-1)
    assert frag.mean() <= pa.FRAGILE_FRAC, f"fragile share {frag.mean():.2e}"
    ok = ~frag
    return ok if own is None else ok & (np.asarray(own).reshape(-1) != 0)


def _dev_mask(mask, gpu):
    return torch.from_numpy(mask.astype(np.uint8)).to(gpu)


def _assert_close(name, got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max() if ref.size else 0.0
    err = np.abs(got - ref)
    bound = pa.MIXED_REL * np.abs(ref) + pa.MIXED_ABS * scale
    worst = int(np.argmax(err - bound)) if ref.size else 0
    print(f"{name}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()) if scale else 0.0:.3f}")
    assert np.all(err <= bound), (name, worst, float(got[worst]), float(ref[worst]))


def _assert_scores(name, scores, spec):
    wmax, wsum, count = spec
    assert np.array_equal(scores.count.cpu().numpy(), count), name
    _assert_close(name + " wmax", scores.wmax.cpu().numpy(), wmax)
    _assert_close(name + " wsum", scores.wsum.cpu().numpy(), wsum)


# ---- against the spec ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_statistics_match_the_spec(gpu, name):
    cam, scene, view = _case(name)
    ok = _ok_mask(view)
    scores, call = _score(gpu, cam, scene, pixel_mask=_dev_mask(ok, gpu))
    spec = cs.fold(view, pixel_mask=ok)
    _assert_scores(name, scores, spec)
    assert float(scores.wmax.max()) <= CAP
    assert torch.equal(scores.entries, torch.ones_like(scores.entries)) and scores.views == 1
    # rows blended nowhere keep their zero BITS
    untouched = spec[2] == 0
    assert not scores.wmax.cpu().numpy().view(np.uint32)[untouched].any()
    assert not scores.wsum.cpu().numpy().view(np.uint64)[untouched].any()
    if name == "big_rows":
        assert int((view.out.geom.tiles_touched[:3] > 64).sum()) == 3
    if name == "long_lists":
        # rows that are blended nowhere, and saturated pixels (a stop leaves T in [1e-4, 1e-2)): rows behind the stop
        assert int(untouched.sum()) >= 1 and int((view.out.final_T < 1e-2).sum()) > 1000


def test_opaque_row_centred_on_a_pixel_reaches_the_cap(gpu):
    """Opacity 1, exponent ~0 at its centre pixel, nothing in front: w = min(0.99, 1 * G) * 1.  That pixel is a knife edge
    of the oracle's exponent-sign test (the one fragile pixel of the case), so the weight is checked on the UNMASKED run;
    the masked run is compared with the spec like every other case."""
    cam, scene, view = _case("centred_row")
    assert view.out.fragile.sum() <= 1
    scores, _ = _score(gpu, cam, scene)
    assert abs(float(scores.wmax[0]) - 0.99) <= pa.MIXED_REL * 0.99 + pa.MIXED_ABS * 0.99
    assert float(scores.wmax.max()) <= CAP
    ok = _ok_mask(view)
    masked, _ = _score(gpu, cam, scene, pixel_mask=_dev_mask(ok, gpu))
    _assert_scores("centred row, masked", masked, cs.fold(view, pixel_mask=ok))


def test_default_mask_sums_to_the_opacity_of_the_devices_own_image(gpu):
    """sum wsum == sum (1 - final_T) of the device's own final_T, all pixels counted (a fragile-free case)."""
    from diff_gaussian_rasterization import _C
    cam, scene, view = _case("edge_tiles_b")
    assert not view.out.fragile.any()
    scores, call = _score(gpu, cam, scene)
    fT = _C.raster_views(call)["final_T"].double()
    total, ref = float(scores.wsum.sum()), float((1.0 - fT).sum())
    assert abs(total - ref) <= 1e-5 * ref, (total, ref)
    _assert_scores("all pixels", scores, cs.fold(view))


def test_half_plane_mask_leaves_rows_outside_it_untouched(gpu):
    cam, scene, view = _case("edge_tiles_b")
    W, H = cam.image_width, cam.image_height
    own = np.zeros((H, W), dtype=bool)
    own[:, W // 2:] = True
    ok = _ok_mask(view, own)
    scores, _ = _score(gpu, cam, scene, pixel_mask=_dev_mask(ok, gpu))
    _assert_scores("half plane", scores, cs.fold(view, pixel_mask=ok))
    g = view.out.geom
    outside = (~g.visible) | (g.px + g.radii < W // 2 - 1)
    assert outside.sum() > 50 and (~outside).sum() > 50
    for t in (scores.wmax, scores.wsum, scores.count):
        assert not t.cpu().numpy()[outside].any()
    assert int(scores.count.sum()) > 0


def test_nothing_visible_touches_nothing(gpu):
    cam, scene, _, _ = pa.default_case(100, 40, 30, 3)
    scene.means3D[:, 2] = -scene.means3D[:, 2]                 # behind the camera
    from hgs.importance import Scores, score_view
    rs, att = _forward(gpu, cam, scene)
    scores = Scores.zeros(100, gpu)
    scores.wmax.fill_(7.0); scores.wsum.fill_(-3.0); scores.count.fill_(11)
    call = score_view(scores, rs, **att)
    torch.cuda.synchronize()
    assert call.L == 0
    assert bool((scores.wmax == 7.0).all()) and bool((scores.wsum == -3.0).all()) and bool((scores.count == 11).all())


# ---- several views -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _orbit():
    cam0, scene, _, _ = pa.default_case(500, 64, 48, 8)
    cams = [synth.orbit_camera(64, 48, k, 3) for k in range(3)]
    return scene, cams, [cs.oracle_view(scene, c) for c in cams]


def _accumulate(gpu, scene, cams, masks, order):
    from hgs.importance import Scores, score_view
    scores = Scores.zeros(scene.P, gpu)
    for k in order:
        rs, att = _forward(gpu, cams[k], scene)
        score_view(scores, rs, **att, pixel_mask=masks[k])
    torch.cuda.synchronize()
    return scores


def test_three_views_accumulate_reproducibly(gpu):
    scene, cams, views = _orbit()
    oks = [_ok_mask(v) for v in views]
    masks = [_dev_mask(ok, gpu) for ok in oks]
    spec = None
    for v, ok in zip(views, oks):
        spec = cs.fold(v, pixel_mask=ok, into=spec)
    a = _accumulate(gpu, scene, cams, masks, (0, 1, 2))
    _assert_scores("three views", a, spec)
    assert a.views == 3 and bool((a.entries == 3).all())
    b = _accumulate(gpu, scene, cams, masks, (0, 1, 2))
    for x, y in ((a.wmax, b.wmax), (a.wsum, b.wsum), (a.count, b.count)):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))              # bit for bit
    c = _accumulate(gpu, scene, cams, masks, (2, 0, 1))
    assert torch.equal(a.wmax.view(torch.int32), c.wmax.view(torch.int32)) and torch.equal(a.count, c.count)
    _assert_close("permuted order wsum", c.wsum.cpu().numpy(), spec[1])


# ---- slot maps ---------------------------------------------------------------------------------------------------------
def test_slot_map_permutes_bit_for_bit_and_ignores_rows(gpu):
    cam, scene, view = _case("edge_tiles_a")
    P, S = scene.P, scene.P + 37
    base, _ = _score(gpu, cam, scene)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(S)[:P].astype(np.int32)).to(gpu)
    got, _ = _score(gpu, cam, scene, S=S, slot_of_row=perm)
    pl = perm.long()
    for x, y in ((base.wmax, got.wmax), (base.wsum, got.wsum), (base.count, got.count), (base.entries, got.entries)):
        assert torch.equal(x.view(torch.uint8).view(P, -1), y[pl].contiguous().view(torch.uint8).view(P, -1))
        rest = torch.ones(S, dtype=torch.bool, device=gpu)
        rest[pl] = False
        assert not bool(y[rest].any())
    # rows mapped to -1 or beyond n_slots: every slot keeps its bits
    from hgs.importance import Scores
    from diff_gaussian_rasterization import _C
    rs, att = _forward(gpu, cam, scene)
    slot = torch.where(torch.arange(P, device=gpu) % 2 == 0, -1, S + 5).to(torch.int32)
    with torch.no_grad():
        call = _C.rasterize_gaussians(rs.bg, att["means3D"], None, att["opacities"], att["scales"], att["rotations"], 1.0,
                                      None, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
                                      rs.image_width, att["shs"], rs.sh_degree, rs.campos, False, False, rs.render_indices,
                                      rs.parent_indices, rs.interpolation_weights, rs.num_node_kids, False)[-1]
    sc = Scores.zeros(S, gpu)
    sc.wmax.fill_(0.25); sc.wsum.fill_(1.5); sc.count.fill_(9)
    _C.raster_contributions(call, sc.wmax, sc.wsum, sc.count, slot_of_row=slot)
    torch.cuda.synchronize()
    assert bool((sc.wmax == 0.25).all()) and bool((sc.wsum == 1.5).all()) and bool((sc.count == 9).all())
    # the glue's checks
    for bad in (dict(wmax=sc.wmax.double()), dict(wsum=sc.wsum[:-1]), dict(count=sc.count.cpu()),
                dict(slot_of_row=slot.long()), dict(slot_of_row=slot[:-1]), dict(pixel_mask=torch.ones(3, dtype=torch.uint8, device=gpu))):
        kw = dict(wmax=sc.wmax, wsum=sc.wsum, count=sc.count, slot_of_row=slot, pixel_mask=None)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            _C.raster_contributions(call, kw.pop("wmax"), kw.pop("wsum"), kw.pop("count"), **kw)
    with pytest.raises(RuntimeError, match="slot_of_row"):
        _C.raster_contributions(call, sc.wmax[:P - 1].contiguous(), sc.wsum[:P - 1].contiguous(), sc.count[:P - 1].contiguous())


# ---- guards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 65, 777])
@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_outputs_and_scratch_stay_inside_their_buffers(gpu, P, fill):
    """The three outputs and the scratch between guard words, P off the wave grid; the scratch 0x00- and 0xFF-filled (it
    needs no initialisation: both give the bits of the unguarded call)."""
    from diff_gaussian_rasterization import _C
    cam, scene, _, _ = pa.default_case(P, 70, 45, 12)
    ref, _ = _score(gpu, cam, scene)
    rs, att = _forward(gpu, cam, scene)
    with torch.no_grad():
        call = _C.rasterize_gaussians(rs.bg, att["means3D"], None, att["opacities"], att["scales"], att["rotations"], 1.0,
                                      None, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
                                      rs.image_width, att["shs"], rs.sh_degree, rs.campos, False, False, rs.render_indices,
                                      rs.parent_indices, rs.interpolation_weights, rs.num_node_kids, False)[-1]
    lib = _lib.lib()
    wmax, wsum, count = (wg.guarded(P * b, gpu, 0x00, n) for b, n in ((4, "wmax"), (8, "wsum"), (8, "count")))
    tmp = wg.guarded(lib.hgs_raster_contrib_tmp_bytes(call.L_ws), gpu, fill, "tmp")
    rc = lib.hgs_raster_contrib(C.byref(call.args), call.p_geom, call.p_bin, call.p_img, call.L_ws, None, None, P,
                                wmax.addr, wsum.addr, count.addr, tmp.addr,
                                C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream), gpu.index or 0)
    _lib.check(rc, "hgs_raster_contrib")
    wg.check(wmax, wsum, count, tmp)
    assert torch.equal(wmax.view(torch.int32), ref.wmax.view(torch.int32))
    assert torch.equal(wsum.view(torch.int64), ref.wsum.view(torch.int64))
    assert torch.equal(count.view(torch.int64), ref.count)
    assert int(ref.count.sum()) > 0 or P == 1


# ---- the in-op LOD route -----------------------------------------------------------------------------------------------
def test_in_op_lod_route_equals_the_gathered_rows(gpu):
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    from hgs.importance import Scores, activated, score_view, tau_of, view_cut
    K = 7
    hd, cam = cc.on_device(cc.hier2000(), gpu), cc.camera()
    N = hd.num_nodes
    ri, pi, w, kids = view_cut(hd, cam, tau_of(3.0, cam.tanfovx, cam.image_width), frustum=False)
    n = int(ri.numel())
    assert 0 < n < N
    sky = synth.make_scene(K, cam, seed=77, s_px=(6.0, 20.0), z_range=(25.0, 40.0)).to(gpu)
    att = activated(hd)
    full = dict(means3D=torch.cat((att["means3D"], sky.means3D)), shs=torch.cat((att["shs"], sky.shs)),
                opacities=torch.cat((att["opacities"], sky.opacities)), scales=torch.cat((att["scales"], sky.scales)),
                rotations=torch.cat((att["rotations"], sky.rotations)))
    full = {k: v.contiguous() for k, v in full.items()}
    # the rows lod_gather writes, the skybox rows behind them, the product path's weights for the tail
    gm, gs, gr, gsh, gop = _C.lod_gather(ri, pi, w, full["means3D"], full["scales"], full["rotations"], full["shs"],
                                         full["opacities"])
    tail = lambda a, b: torch.cat((a, b[N:])).contiguous()
    rows = dict(means3D=tail(gm, full["means3D"]), shs=tail(gsh, full["shs"]), opacities=tail(gop, full["opacities"]),
                scales=tail(gs, full["scales"]), rotations=tail(gr, full["rotations"]))
    wa = torch.cat((w, torch.ones(K, device=gpu)))
    ka = torch.cat((kids, torch.ones(K, dtype=torch.int32, device=gpu)))
    # the oracle on those rows says which pixels are decidable
    sc_cpu = synth.Scene(rows["means3D"].cpu(), rows["scales"].cpu(), rows["rotations"].cpu(), rows["opacities"].cpu(),
                         rows["shs"].cpu(), 3)
    view = cs.oracle_view(sc_cpu, cam, interpolation_weights=wa.cpu(), num_node_kids=ka.cpu())
    ok = _ok_mask(view)
    mask = _dev_mask(ok, gpu)
    e_i = torch.empty(0, dtype=torch.int32, device=gpu)

    def settings(r, p, ww, kk):
        kw = pa.settings_kwargs(cam, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=ww, num_node_kids=kk)
        kw["render_indices"], kw["parent_indices"] = r, p
        return dgr.GaussianRasterizationSettings(**kw)

    slot = torch.cat((ri, torch.full((K,), -1, dtype=torch.int32, device=gpu)))
    a, b = Scores.zeros(N, gpu), Scores.zeros(N, gpu)
    score_view(a, settings(ri.contiguous(), pi.contiguous(), w.contiguous(), kids.contiguous()), **full, pixel_mask=mask,
               skybox_points=K)
    call_b = score_view(b, settings(e_i, e_i, wa, ka), **rows, slot_of_row=slot, pixel_mask=mask)
    torch.cuda.synchronize()
    assert call_b.P == n + K
    spec = cs.fold(view, pixel_mask=ok, slot_of_row=slot.cpu().numpy(), n_slots=N)
    _assert_scores("gathered rows", b, spec)
    _assert_scores("in-op LOD", a, spec)
    assert torch.equal(a.count, b.count) and torch.equal(a.entries, b.entries)
    _assert_close("routes wmax", a.wmax.cpu().numpy(), b.wmax.cpu().numpy())
    _assert_close("routes wsum", a.wsum.cpu().numpy(), b.wsum.cpu().numpy())
    # only the cut's nodes were entered and touched; the skybox rows (drawn: the spec sees them) reach no slot
    in_cut = torch.zeros(N, dtype=torch.bool, device=gpu)
    in_cut[ri.long()] = True
    assert torch.equal(a.entries, in_cut.long())
    assert not bool(a.count[~in_cut].any()) and not bool(a.wmax[~in_cut].any()) and not bool(a.wsum[~in_cut].any())
    sky_only = cs.fold(view, pixel_mask=ok, slot_of_row=np.concatenate([np.full(n, -1), np.arange(K)]), n_slots=K)
    assert sky_only[2].sum() > 0, "the skybox must be on screen for the case to mean anything"
    assert int(a.count.sum()) == int(spec[2].sum())
