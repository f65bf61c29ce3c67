"""hgs_raster_attribute on the GPU against the float64 spec (tests/attribution_spec.py), tied to hgs_raster_contrib, and
the per-node LOD error built on it (hgs.importance, python -m hgs.lod_error).

Against the spec the image is a seeded SIGNED random one, so the element-wise bound is taken against the fold of ``|f|``:
``|got - A| <= MIXED_REL * Aabs + MIXED_ABS * max Aabs`` (parity's constants).  The pixel mask handed to the device is
``~oracle.fragile``; the fragile share must stay under parity.FRAGILE_FRAC -- a condition, not a tolerance (the oracle
reports one fragile pixel of 23 040 on ``big_rows`` and none on the other cases of ``test_contribution_gpu.CASES``).  Everything else is an exact statement between
two device results and is compared bit for bit.

The cases, their cameras and their oracle forwards are the contribution tests' own (one oracle run per case and session,
shared through that module's cache and left unchanged)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attribution_spec as asp
import contribution_cases as cc
import parity as pa
import test_contribution_gpu as tcg          # CASES, _case (cached oracle views), _forward, _ok_mask, _dev_mask, _orbit
import ws_guard as wg
from hgs import _lib, hierarchy, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hierarchical-3d-gaussians_amd")


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _image(name, channels=3):
    """The case's seeded signed image, float32 [channels, H, W] on the host (never modified)."""
    cam = tcg._case(name)[0]
    seed = sorted(tcg.CASES).index(name) + 100
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((channels, cam.image_height, cam.image_width))
                            .astype(np.float32))


def _attr(gpu, cam, scene, image, S=None, **kw):
    """One ``attribute_view`` on the plain rows -> (Attribution, call)."""
    from hgs.importance import Attribution, attribute_view
    rs, rows = tcg._forward(gpu, cam, scene)
    image = image.to(gpu)
    att = Attribution.zeros(scene.P if S is None else S, gpu, channels=1 if image.dim() == 2 else image.shape[0])
    call = attribute_view(att, rs, image, **rows, **kw)
    torch.cuda.synchronize()
    return att, call


def _plain_call(gpu, cam, scene):
    from diff_gaussian_rasterization import _C
    rs, a = tcg._forward(gpu, cam, scene)
    with torch.no_grad():
        return _C.rasterize_gaussians(rs.bg, a["means3D"], None, a["opacities"], a["scales"], a["rotations"], 1.0, None,
                                      rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
                                      rs.image_width, a["shs"], rs.sh_degree, rs.campos, False, False, rs.render_indices,
                                      rs.parent_indices, rs.interpolation_weights, rs.num_node_kids, False)[-1]


def _assert_close(name, got, A, Aabs):
    got = np.asarray(got, dtype=np.float64).reshape(A.shape)
    err = np.abs(got - A)
    bound = pa.MIXED_REL * Aabs + pa.MIXED_ABS * Aabs.max()
    worst = np.unravel_index(int(np.argmax(err - bound)), err.shape)
    print(f"{name}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()) if Aabs.max() else 0.0:.3f}")
    assert np.all(err <= bound), (name, worst, float(got[worst]), float(A[worst]), float(bound[worst]))


# ---- against the spec ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("name", list(tcg.CASES))
def test_attribution_matches_the_spec(gpu, name, channels):
    cam, scene, view = tcg._case(name)
    ok = tcg._ok_mask(view)                                     # (asserts the fragile share)
    f = _image(name)[:channels].contiguous()
    att, call = _attr(gpu, cam, scene, f, pixel_mask=tcg._dev_mask(ok, gpu))
    A, Aabs, wsum = asp.fold_image(view, f.numpy(), pixel_mask=ok)
    assert att.acc.shape == (scene.P, channels)
    _assert_close(f"{name} C={channels}", att.acc.cpu().numpy(), A, Aabs)
    _assert_close(f"{name} C={channels} wsum", att.wsum.cpu().numpy(), wsum, wsum)
    assert torch.equal(att.entries, torch.ones_like(att.entries)) and att.views == 1
    # rows blended nowhere keep their zero BITS
    untouched = wsum == 0
    assert not att.acc.cpu().numpy().view(np.uint64)[untouched].any()
    assert not att.wsum.cpu().numpy().view(np.uint64)[untouched].any()
    if name == "big_rows":
        assert int((view.out.geom.tiles_touched[:3] > 64).sum()) == 3            # runs the sum kernel adds by the wave
    if name == "long_lists":
        assert int(untouched.sum()) >= 1 and int((view.out.final_T < 1e-2).sum()) > 1000


# ---- tied to the contribution call, and exact algebra --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tcg.CASES))
def test_wsum_and_a_channel_of_ones_are_the_contribution_calls_wsum_and_the_algebra_is_exact(gpu, name):
    """Bit for bit: ``wsum`` and a channel of ones against raster_contributions' ``wsum`` (w * 1.0f is w, the sums have
    one order); the image times 0.25 gives the outputs times 0.25 (a power of two commutes with every rounding); permuted
    channels give permuted outputs; channel 0 of a C = 3 call is the C = 1 call on that channel (no channel's sum
    depends on another)."""
    from diff_gaussian_rasterization import _C
    from hgs.importance import Scores
    cam, scene, view = tcg._case(name)
    P = scene.P
    mask = tcg._dev_mask(tcg._ok_mask(view), gpu)
    f = _image(name).to(gpu)
    call = _plain_call(gpu, cam, scene)
    sc = Scores.zeros(P, gpu)
    _C.raster_contributions(call, sc.wmax, sc.wsum, sc.count, pixel_mask=mask)

    def run(image, with_wsum=True):
        Cn = 1 if image.dim() == 2 else image.shape[0]
        out = torch.zeros(P, Cn, dtype=torch.float64, device=gpu)
        ws = torch.zeros(P, dtype=torch.float64, device=gpu) if with_wsum else None
        _C.raster_attribute(call, image, out, wsum=ws, pixel_mask=mask)
        return out, ws

    base, ws = run(f)
    assert _same(ws, sc.wsum)
    ones, ws1 = run(torch.ones_like(f[0]))                      # [H, W]: one channel
    assert _same(ones[:, 0], sc.wsum) and _same(ws1, sc.wsum)
    mixed, _ = run(torch.stack((f[1], torch.ones_like(f[0]), f[0])))
    assert _same(mixed[:, 1], sc.wsum)
    assert _same(mixed[:, 0], base[:, 1]) and _same(mixed[:, 2], base[:, 0])          # permuted channels
    quarter, wsq = run(f * 0.25)
    assert _same(quarter, base * 0.25) and _same(wsq, sc.wsum)
    one, none = run(f[:1].contiguous(), with_wsum=False)
    assert none is None and _same(one[:, 0], base[:, 0])
    two, _ = run(f[:2].contiguous())
    assert _same(two, base[:, :2])
    assert int((sc.count > 0).sum()) > 0 and bool((base != 0).any())
    torch.cuda.synchronize()


# ---- selection, not multiplication ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_tiles_b", "long_lists"])
def test_nan_and_infinity_at_pixels_that_do_not_count_reach_no_output(gpu, name):
    """NaN / infinity at masked-out pixels and at counted pixels outside every row's reach (the device's own final_T
    says where nothing is blended): the outputs equal, bit for bit, those with zeros there."""
    from diff_gaussian_rasterization import _C
    cam, scene, view = tcg._case(name)
    W, H = cam.image_width, cam.image_height
    own = (np.arange(W * H) % 7 != 3)
    ok = tcg._ok_mask(view, own)
    f = _image(name).clone()
    clean, call = _attr(gpu, cam, scene, f, pixel_mask=tcg._dev_mask(ok, gpu))
    final_T = _C.raster_views(call)["final_T"].reshape(-1).cpu().numpy()
    unreached = (final_T == 1.0) & ok                           # (a blended row takes at least 1/255 of T away)
    flat = f.reshape(3, -1)
    for sel, vals in ((~ok, (float("nan"), float("inf"), float("-inf"))), (unreached, (float("inf"), float("nan"), float("nan")))):
        idx = torch.from_numpy(np.nonzero(sel)[0])
        for c, v in enumerate(vals):
            flat[c, idx] = v
    assert int((~ok).sum()) > 100 and not torch.isfinite(f).all()
    zeroed = f.clone()
    zeroed[~torch.isfinite(zeroed)] = 0.0
    got, _ = _attr(gpu, cam, scene, f, pixel_mask=tcg._dev_mask(ok, gpu))
    ref, _ = _attr(gpu, cam, scene, zeroed, pixel_mask=tcg._dev_mask(ok, gpu))
    assert _same(got.acc, ref.acc) and _same(got.wsum, ref.wsum) and _same(ref.wsum, clean.wsum)
    assert bool(torch.isfinite(got.acc).all()) and bool((got.acc != 0).any())
    if name == "edge_tiles_b":
        assert int(unreached.sum()) > 0, "the case must have counted pixels that nothing is blended at"


def test_half_plane_mask_leaves_rows_outside_it_their_sentinel_bits(gpu):
    from diff_gaussian_rasterization import _C
    cam, scene, view = tcg._case("edge_tiles_b")
    W, H, P = cam.image_width, cam.image_height, scene.P
    own = np.zeros((H, W), dtype=bool)
    own[:, W // 2:] = True
    ok = tcg._ok_mask(view, own)
    f = _image("edge_tiles_b").to(gpu)
    call = _plain_call(gpu, cam, scene)
    out = torch.full((P, 3), -7.5, dtype=torch.float64, device=gpu)
    ws = torch.full((P,), 3.25, dtype=torch.float64, device=gpu)
    _C.raster_attribute(call, f, out, wsum=ws, pixel_mask=tcg._dev_mask(ok, gpu))
    torch.cuda.synchronize()
    A, Aabs, wsum = asp.fold_image(view, f.cpu().numpy(), pixel_mask=ok)
    _assert_close("half plane", (out + 7.5).cpu().numpy(), A, Aabs)
    g = view.out.geom
    outside = torch.as_tensor(np.asarray((~g.visible) | (g.px + g.radii < W // 2 - 1))).to(gpu)
    assert int(outside.sum()) > 50 and int((~outside).sum()) > 50
    assert bool((out[outside] == -7.5).all()) and bool((ws[outside] == 3.25).all())
    assert bool((ws[torch.from_numpy(wsum > 0).to(gpu)] > 3.25).all())


def test_nothing_visible_touches_nothing(gpu):
    from hgs.importance import Attribution, attribute_view
    cam, scene, _, _ = pa.default_case(100, 40, 30, 3)
    scene.means3D[:, 2] = -scene.means3D[:, 2]                 # behind the camera
    rs, rows = tcg._forward(gpu, cam, scene)
    att = Attribution.zeros(100, gpu, channels=2)
    att.acc.fill_(7.0); att.wsum.fill_(-3.0)
    call = attribute_view(att, rs, torch.full((2, 30, 40), float("nan"), device=gpu), **rows)
    torch.cuda.synchronize()
    assert call.L == 0 and att.views == 1
    assert bool((att.acc == 7.0).all()) and bool((att.wsum == -3.0).all())


# ---- slot maps and the glue's refusals -------------------------------------------------------------------------------------
def test_slot_map_permutes_bit_for_bit_and_ignores_rows(gpu):
    from diff_gaussian_rasterization import _C
    cam, scene, view = tcg._case("edge_tiles_a")
    P, S = scene.P, scene.P + 37
    f = _image("edge_tiles_a")
    base, _ = _attr(gpu, cam, scene, f)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(S)[:P].astype(np.int32)).to(gpu)
    perm[::5] = -1                                             # some rows ignored
    perm[1::11] = S + 3
    got, call = _attr(gpu, cam, scene, f, S=S, slot_of_row=perm)
    used = (perm >= 0) & (perm < S)
    pl = perm[used].long()
    assert int(used.sum()) < P and bool((base.wsum[~used] > 0).any())
    for x, y in ((base.acc, got.acc), (base.wsum, got.wsum), (base.entries, got.entries)):
        assert _same(x[used], y[pl])
        rest = torch.ones(S, dtype=torch.bool, device=gpu)
        rest[pl] = False
        assert not bool(y[rest].any())
    # the glue's checks, in the wording of raster_contributions
    fd = f.to(gpu)
    out, ws = torch.zeros(S, 3, dtype=torch.float64, device=gpu), torch.zeros(S, dtype=torch.float64, device=gpu)
    good = dict(image=fd, out=out, wsum=ws, slot_of_row=perm, pixel_mask=None)
    for bad, word in ((dict(image=fd.cpu()), "image must be a tensor on the forward's device"),
                      (dict(image=fd.double()), "float32"), (dict(image=fd[None]), "float32 tensor"),
                      (dict(image=torch.zeros(4, *fd.shape[1:], device=gpu)), "1 to 3 channels"),
                      (dict(image=fd[:, :-1].contiguous()), "like the forward's"),
                      (dict(out=out.cpu()), "out must be a tensor on the forward's device"),
                      (dict(out=out.float()), "out must be a contiguous"), (dict(out=out[:, :2]), "out must be a contiguous"),
                      (dict(out=out[:, :2].contiguous()), r"out must be \[S, 3\]"), (dict(out=ws), r"out must be \[S, 3\]"),
                      (dict(wsum=ws[:-1]), "same length"), (dict(wsum=ws.float()), "wsum must be a contiguous"),
                      (dict(wsum=out), "same length"),
                      (dict(slot_of_row=perm.long()), "slot_of_row must be an int32"),
                      (dict(slot_of_row=perm[:-1]), "one entry per op row"),
                      (dict(pixel_mask=torch.ones(3, dtype=torch.uint8, device=gpu)), "pixel_mask must hold"),
                      (dict(pixel_mask=torch.ones(cam.image_width * cam.image_height, device=gpu)), "pixel_mask must be a uint8"),
                      (dict(slot_of_row=None, out=out[:P - 1].contiguous(), wsum=None), "pass slot_of_row")):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(RuntimeError, match=word):
            _C.raster_attribute(call, kw.pop("image"), kw.pop("out"), **kw)
    torch.cuda.synchronize()
    assert not bool(out.any()) and not bool(ws.any())


# ---- several views -----------------------------------------------------------------------------------------------------
def test_three_orbit_views_accumulate_to_identical_bits_twice(gpu):
    from hgs.importance import Attribution, attribute_view
    scene, cams, views = tcg._orbit()
    masks = [tcg._dev_mask(tcg._ok_mask(v), gpu) for v in views]
    g = np.random.default_rng(9)
    images = [torch.from_numpy(g.standard_normal((3, c.image_height, c.image_width)).astype(np.float32)).to(gpu) for c in cams]

    def accumulate():
        att = Attribution.zeros(scene.P, gpu, channels=3)
        for cam, m, f in zip(cams, masks, images):
            rs, rows = tcg._forward(gpu, cam, scene)
            attribute_view(att, rs, f, **rows, pixel_mask=m)
        torch.cuda.synchronize()
        return att

    a, b = accumulate(), accumulate()
    assert _same(a.acc, b.acc) and _same(a.wsum, b.wsum) and a.views == 3 and bool((a.entries == 3).all())
    A, Aabs, wsum = (sum(x) for x in zip(*[asp.fold_image(v, f.cpu().numpy(), pixel_mask=tcg._ok_mask(v))
                                           for v, f in zip(views, images)]))
    _assert_close("three views", a.acc.cpu().numpy(), A, Aabs)
    _assert_close("three views wsum", a.wsum.cpu().numpy(), wsum, wsum)


# ---- conservation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_tiles_b", "long_lists"])
def test_attributions_add_up_to_the_image_under_the_devices_own_opacity(gpu, name):
    """sum_s A[s, c] == sum_p f_c(p) (1 - final_T(p)) with the device's own final_T, all pixels counted, within
    MIXED_REL * sum_p |f_c| (1 - final_T)."""
    from diff_gaussian_rasterization import _C
    cam, scene, view = tcg._case(name)
    f = _image(name)
    att, call = _attr(gpu, cam, scene, f)
    fT = _C.raster_views(call)["final_T"].double().reshape(1, -1).cpu()
    fd = f.double().reshape(3, -1)
    ref, scale = (fd * (1.0 - fT)).sum(dim=1), (fd.abs() * (1.0 - fT)).sum(dim=1)
    got = att.acc.sum(dim=0).cpu()
    print(f"{name}: conservation err / bound = {((got - ref).abs() / (pa.MIXED_REL * scale)).tolist()}")
    assert bool(((got - ref).abs() <= pa.MIXED_REL * scale).all()), (got.tolist(), ref.tolist(), scale.tolist())
    assert abs(float(att.wsum.sum()) - float((1.0 - fT).sum())) <= pa.MIXED_REL * float((1.0 - fT).sum())


# ---- guards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("P", [1, 63, 65, 777])
def test_outputs_and_scratch_stay_inside_their_buffers(gpu, P, fill, channels):
    """``out``, ``wsum`` and the scratch between guard words through the raw C ABI, P off the wave grid; the scratch 0x00-
    and 0xFF-filled (it needs no initialisation: both give the bits of the unguarded call)."""
    cam, scene, _, _ = pa.default_case(P, 70, 45, 12)
    f = torch.from_numpy(np.random.default_rng(P).standard_normal((channels, 45, 70)).astype(np.float32)).to(gpu)
    ref, _ = _attr(gpu, cam, scene, f)
    call = _plain_call(gpu, cam, scene)
    lib = _lib.lib()
    out, ws = wg.guarded(P * channels * 8, gpu, 0x00, "out"), wg.guarded(P * 8, gpu, 0x00, "wsum")
    tmp = wg.guarded(lib.hgs_raster_attribute_tmp_bytes(call.L_ws), gpu, fill, "tmp")
    rc = lib.hgs_raster_attribute(C.byref(call.args), call.p_geom, call.p_bin, call.p_img, call.L_ws, f.data_ptr(), channels,
                                  None, None, P, out.addr, ws.addr, tmp.addr,
                                  C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream), gpu.index or 0)
    _lib.check(rc, "hgs_raster_attribute")
    wg.check(out, ws, tmp)
    assert torch.equal(out.view(torch.int64, P, channels), ref.acc.view(torch.int64))
    assert torch.equal(ws.view(torch.int64), ref.wsum.view(torch.int64))
    assert bool((ref.wsum > 0).any()) or P == 1


# ---- the in-op LOD route -----------------------------------------------------------------------------------------------
def test_in_op_lod_route_equals_the_gathered_rows_bit_for_bit(gpu):
    """The cut of hier2000() at 3 px with 7 skybox rows behind it: the in-op LOD forward (node rows interpolated in K1,
    default slot map) against the plain forward of the same rows gathered by hand (``lod_gather``, the product path's
    weights, an explicit slot map)."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    from hgs.importance import Attribution, activated, attribute_view, tau_of, view_cut
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

    f = torch.from_numpy(np.random.default_rng(5).standard_normal((3, cc.H, cc.W)).astype(np.float32)).to(gpu)
    slot = torch.cat((ri, torch.full((K,), -1, dtype=torch.int32, device=gpu)))
    a, b = Attribution.zeros(N, gpu, channels=3), Attribution.zeros(N, gpu, channels=3)
    attribute_view(a, settings(ri.contiguous(), pi.contiguous(), w.contiguous(), kids.contiguous()), f, **full, skybox_points=K)
    call_b = attribute_view(b, settings(e_i, e_i, wa, ka), f, **gathered, slot_of_row=slot)
    torch.cuda.synchronize()
    assert call_b.P == n + K
    d = (a.acc - b.acc).abs().max().item()
    print(f"in-op LOD against gathered rows: max |difference| = {d:.3e} of max {b.acc.abs().max().item():.3e}")
    assert _same(a.acc, b.acc) and _same(a.wsum, b.wsum) and torch.equal(a.entries, b.entries)
    in_cut = torch.zeros(N, dtype=torch.bool, device=gpu)
    in_cut[ri.long()] = True
    assert torch.equal(a.entries, in_cut.long()) and not bool(a.acc[~in_cut].any()) and not bool(a.wsum[~in_cut].any())
    assert int((a.wsum > 0).sum()) > 100


# ---- the per-node LOD error ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hier():
    return cc.on_device(cc.hier2000(), torch.device("cuda:0"))


def test_lod_error_against_the_same_cut_is_zero_bits_and_wsum_is_score_hierarchys(gpu):
    from hgs.importance import lod_error_hierarchy, score_hierarchy
    h = _hier()
    err = lod_error_hierarchy(h, cc.orbit(), 3.0, ref_tau_px=3.0)
    sc = score_hierarchy(h, cc.orbit(), tau_px=3.0)
    torch.cuda.synchronize()
    assert err.acc.shape == (h.num_nodes, 1) and err.views == 3
    assert not bool(_bits(err.acc).any())
    assert _same(err.wsum, sc.wsum) and torch.equal(err.entries, sc.entries) and int((err.wsum > 0).sum()) > 100


def test_lod_error_against_the_leaves_is_the_hand_composition(gpu):
    from diff_gaussian_rasterization import _C
    from hgs.frustum import cull_bounds
    from hgs.importance import Attribution, _settings, activated, attribute_view, lod_error_hierarchy, tau_of, view_cut
    h = _hier()
    N = h.num_nodes
    got = lod_error_hierarchy(h, cc.orbit(), 3.0)
    e = got.acc[:, 0]
    assert bool((e >= 0).all()) and bool((e > 0).any()) and not bool(e[got.entries == 0].any())
    assert bool((got.entries[h.nodes[:, 6] != 0] > 0).any())                      # interior nodes are in these cuts
    m = got.mean()[:, 0]
    assert bool((m >= 0).all()) and not bool(m[got.wsum == 0].any()) and bool(torch.isfinite(m).all())
    rows = activated(h)
    bounds = cull_bounds(h.nodes, rows["means3D"], rows["scales"])
    ref = Attribution.zeros(N, gpu, channels=1)
    empty = torch.empty(0, dtype=torch.int32, device=gpu)
    for cam in cc.orbit():
        cut = lambda px: [t.contiguous() for t in view_cut(h, cam, tau_of(px, cam.tanfovx, cam.image_width), True, bounds)]
        ri, pi, w, kids = cut(0.0)
        rs = _settings(cam, gpu, ri, pi, w, kids)
        with torch.no_grad():
            target = _C.rasterize_gaussians(
                rs.bg, rows["means3D"], None, rows["opacities"], rows["scales"], rows["rotations"], 1.0, None, rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rows["shs"], 3, rs.campos, False,
                False, empty, empty, w, kids, False, prepare_backward=False, lod=(ri, pi, 0))[1].clone()
        attribute_view(ref, _settings(cam, gpu, *cut(3.0)),
                       lambda color: (color - target).abs().mean(dim=0, keepdim=True), **rows)
    torch.cuda.synchronize()
    assert _same(got.acc, ref.acc) and _same(got.wsum, ref.wsum) and torch.equal(got.entries, ref.entries) and ref.views == 3


def test_command_writes_the_apis_arrays(gpu, tmp_path):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from hgs import score_hierarchy as cmd
    from hgs.importance import lod_error_hierarchy, render_hierarchy
    host = cc.hier2000()
    src = str(tmp_path / "in.hier")
    write_hierarchy(src, *[getattr(host, k) for k in cc.FIELDS])
    cams_json = tmp_path / "cameras.json"
    cams_json.write_text(json.dumps([cc.camera_entry(c) for c in cc.orbit()]))
    npz, npz_t, gt = str(tmp_path / "out" / "err.npz"), str(tmp_path / "err_t.npz"), tmp_path / "gt"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    run = lambda *argv: subprocess.run([sys.executable, "-m", "hgs.lod_error", *argv], capture_output=True, text=True,
                                       env=env, timeout=300)
    r = run(src, npz, "--cameras", str(cams_json), "--tau-px", "3")
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("\n") == 1 and "3 views at 3 px against the cut at 0 px" in r.stdout
    # the function on what the command read
    loaded = hierarchy.Hierarchy(*load_hierarchy(src))
    hl = cc.on_device(loaded, gpu, boxes=loaded.boxes.reshape(-1, 2, 4))
    cams = cmd.read_cameras(str(cams_json))
    want = lod_error_hierarchy(hl, cams, 3.0).numpy()
    got = np.load(npz)
    assert sorted(got.files) == ["entries", "err", "views", "wsum"]
    assert got["err"].dtype == np.float64 and got["err"].shape == (hl.num_nodes,)
    assert np.array_equal(got["err"], want["acc"][:, 0]) and got["err"].max() > 0
    for k in ("wsum", "entries"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert int(got["views"]) == 3
    # --targets with the leaves' own renders is the same attribution
    gt.mkdir()
    for k, cam in enumerate(cams):
        np.save(gt / f"{k}.npy", render_hierarchy(hl, cam, 0.0).cpu().numpy())
    r = run(src, npz_t, "--cameras", str(cams_json), "--tau-px", "3", "--targets", str(gt))
    assert r.returncode == 0, r.stderr
    got_t = np.load(npz_t)
    for k in got.files:
        assert np.array_equal(got_t[k], got[k]), k
