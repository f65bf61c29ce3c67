"""The fused geometry + SH backward (preprocess_bwd_sh_kernel, csrc/preprocess.hip) against the two kernels it replaces.

The drop-in training call ([P,M,3] coefficients with 3 M % 4 == 0, no LOD rows, no accumulation, no deferred SH backward)
runs K8a and K8b as one kernel; HGS_K8_FUSE=0 keeps them apart and is read on every call.  The fused kernel must give
the two kernels' gradients TO THE BIT: every comparison between the routes here is ``torch.equal``.  The calls that do not
qualify keep the two kernels and are checked against the oracle as the other suites do."""
import numpy as np
import pytest
import torch

import parity as pa
from hgs import synth

pytestmark = pytest.mark.gpu

GRADS = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")
BG = torch.tensor([0.1, 0.2, 0.3])


def _both_routes(monkeypatch, run):
    """run() with the two-kernel route, then with the default (fused) one."""
    monkeypatch.setenv("HGS_K8_FUSE", "0")
    two = run()
    monkeypatch.delenv("HGS_K8_FUSE")
    return two, run()


def _assert_same_bits(name, two, fused):
    for k in GRADS:
        a, b = two["grads"][k], fused["grads"][k]
        assert torch.isfinite(a).all(), (name, k)
        if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
            bad = torch.nonzero((a.view(torch.int32) != b.view(torch.int32)).reshape(a.shape[0], -1).any(1)).flatten()
            raise AssertionError(f"{name}: dL/d{k} differs between the routes on {bad.numel()} rows, first {bad[:8].tolist()}")


def _pair(monkeypatch, name, scene, cam, gc, gd, gpu, **kw):
    two, fused = _both_routes(monkeypatch, lambda: pa.run_hip(scene, cam, BG, gc, gd, gpu, grad_mask=None, **kw))
    _assert_same_bits(name, two, fused)
    return fused


@pytest.mark.parametrize("W,H", [(53, 37), (64, 48)])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 777])
def test_partial_waves_and_workgroups(gpu, monkeypatch, P, W, H):
    cam, scene, gc, gd = pa.default_case(P, W, H, seed=P + W)
    hip = _pair(monkeypatch, f"P={P} {W}x{H}", scene, cam, gc, gd, gpu, debug=False)
    assert P == 1 or float(hip["grads"]["shs"].abs().max()) > 0


def _awkward_scene(P, cam, seed):
    """Rows behind the camera and beside the frustum (culled), rows whose colour is clamped in all, one or two
    channels."""
    scene = synth.make_scene(P, cam, seed=seed)
    scene.means3D[0::7, 2] = -scene.means3D[0::7, 2]                 # behind the camera
    scene.means3D[3::11, 0] = 40.0 * scene.means3D[3::11, 2]         # far outside the frustum
    scene.shs[1::5, 0] = -3.0                                        # all three channels below zero: flags 1 | 2 | 4
    scene.shs[2::5, 0, 0] = -3.0                                     # red only
    scene.shs[4::5, 0, 1:] = -3.0                                    # green and blue
    return scene


@pytest.mark.parametrize("do_depth", [True, False])
def test_culled_rows_and_clamped_colours(gpu, monkeypatch, do_depth):
    P, W, H = 600, 64, 48
    cam = synth.make_camera(W, H)
    scene = _awkward_scene(P, cam, seed=17)
    gc, gd = synth.upstream_grads(H, W, seed=3)
    hip = _pair(monkeypatch, f"awkward depth={do_depth}", scene, cam, gc, gd, gpu, do_depth=do_depth)
    tt = hip["views"]["tiles_touched"]
    culled, vis = tt == 0, tt > 0
    assert int(culled.sum()) >= P // 8 and int(vis.sum()) >= P // 2
    g = hip["grads"]
    for k in GRADS:                                                  # culled rows: zeros everywhere
        assert not g[k][culled].any(), k
    # a clamped channel takes no gradient, its neighbours do
    rows = torch.arange(P)
    red_only = vis & (rows % 5 == 2) & (rows % 7 != 0) & (rows % 11 != 3)
    assert int(red_only.sum()) > 10
    assert not g["shs"][red_only][:, :, 0].any() and g["shs"][red_only][:, :, 1].any()
    all_three = vis & (rows % 5 == 1)
    assert int(all_three.sum()) > 10 and not g["shs"][all_three].any()


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_active_degrees_on_full_coefficient_tensors(gpu, monkeypatch, deg):
    cam, scene, gc, gd = pa.default_case(300, 53, 37, seed=5 + deg)
    scene.sh_degree = deg
    assert scene.shs.shape[1] == 16
    hip = _pair(monkeypatch, f"degree {deg}", scene, cam, gc, gd, gpu)
    nb = (deg + 1) ** 2
    assert hip["grads"]["shs"][:, :nb].any() and not hip["grads"]["shs"][:, nb:].any()


def test_long_runs_take_the_presum_route(gpu, monkeypatch):
    """L > 6 P: the worklist and presum kernels run in front, the fused kernel adds the segment sums (two segments for
    a run of more than 512 records) and walks the short runs of such a wave in global memory."""
    W = H = 512
    P = 300
    cam = synth.make_camera(W, H)
    scene = synth.make_scene(P, cam, seed=41, s_px=(4.0, 90.0))
    scene.opacities = scene.opacities * 0.35
    gc, gd = synth.upstream_grads(H, W, seed=9)
    hip = _pair(monkeypatch, "presum", scene, cam, gc, gd, gpu, debug=False)
    tt = hip["views"]["tiles_touched"].long()
    assert hip["L"] == int(tt.sum()) and hip["L"] > 6 * P, hip["L"]
    assert int((tt > 512).sum()) >= 1, int(tt.max())
    assert int(((tt >= 49) & (tt <= 512)).sum()) >= 1
    assert int(((tt > 0) & (tt <= 48)).sum()) >= 1                    # short runs next to the long ones


# ---- the calls that keep the two kernels (and M = 4, which the fused kernel takes) against the oracle ------------------
def test_four_coefficients_against_the_oracle(gpu):
    cam, scene, gc, gd = pa.default_case(300, 64, 48, seed=23, sh_degree=1)
    assert tuple(scene.shs.shape[1:]) == (4, 3)
    pa.assert_verified("[P,4,3]", pa.verify_pair(scene, cam, BG, gc, gd, gpu))


def test_precomputed_colours_against_the_oracle(gpu):
    cam, scene, gc, gd = pa.default_case(300, 64, 48, seed=24)
    cols = torch.rand(scene.P, 3, generator=torch.Generator().manual_seed(2))
    pa.assert_verified("colors_precomp", pa.verify_pair(scene, cam, BG, gc, gd, gpu, colors_precomp=cols))


def test_accumulated_gradients_against_the_oracle(gpu):
    import diff_gaussian_rasterization as dgr
    from hgs import dp
    W, H, P = 64, 48, 300
    scene = synth.make_scene(P, synth.make_camera(W, H), seed=25)
    cams = [synth.orbit_camera(W, H, j, 2, radius=0.3) for j in range(2)]
    gc, gd = synth.upstream_grads(H, W, seed=4)
    names = ("means3D", "shs", "opacities", "scales", "rotations")
    refs = []
    for c in cams:
        r = pa.verify(pa.run_hip(scene, c, BG, gc, gd, gpu, grad_mask=None), pa.oracle_run(scene, c, BG), gc, gd)
        assert r["stats"]["fragile_unmatched"] == 0 and r["stats"]["fragile_unenumerated"] == 0, r["stats"]
        refs.append(r["grads"])
    sc = scene.to(gpu)
    params = {n: getattr(sc, n).clone().requires_grad_(True) for n in names}
    bucket = dp.GradBucket({n: tuple(v.shape) for n, v in params.items()}, gpu)
    rc = dgr.RasterContext(grad_buffers=bucket.views)
    for j, c in enumerate(cams):
        rc.grad_accumulate = j > 0
        rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(c, BG, 3, device=gpu))
        m2 = torch.zeros(P, 3, device=gpu, requires_grad=True)
        color, _, invd = dgr.GaussianRasterizer(rs, context=rc)(
            means3D=params["means3D"], means2D=m2, shs=params["shs"], opacities=params["opacities"],
            scales=params["scales"], rotations=params["rotations"])
        ((color * gc.to(gpu)).sum() + (invd * gd.to(gpu)).sum()).backward()
    for n in names:
        st = pa.err_stats(bucket.views[n].cpu(), refs[0][n] + refs[1][n])
        assert st["maxrel"] <= pa.REL_TOL and st["l2"] <= pa.REL_TOL, (n, st)


def test_lod_rows_against_the_oracle(gpu):
    import test_workspace_bounds_gpu as wb
    cam, rows, gathered, ri, pi, w, ns = wb._lod_cut(600, seed=5)
    gc, gd = synth.upstream_grads(wb.H, wb.W, seed=11)
    wt, kt = torch.from_numpy(w), torch.from_numpy(ns.astype(np.int32))
    orc = pa.oracle_run(gathered, cam, wb.BG, interpolation_weights=wt, num_node_kids=kt)
    d = lambda t: t.contiguous().to(gpu)
    inp = dict(means3D=d(rows["means3D"]), opacity=d(rows["opacities"]), sh=d(rows["shs"]), colors=None, sh_rest=None,
               scales=d(rows["scales"]), rotations=d(rows["rotations"]), cov3D_precomp=None)
    lod = (d(torch.from_numpy(ri.astype(np.int32))), d(torch.from_numpy(pi.astype(np.int32))), 0)
    hip = wb.raster_chain(cam, inp, 3, gc, gd, gpu, 0xFF, lod=lod, weights=d(wt), kids=d(kt))[0]
    wb._check_against_reference(f"in-op LOD n={len(ri)}", hip, orc, gc, gd)


# ---- guard bytes behind every gradient buffer of the C-ABI call -------------------------------------------------------
@pytest.mark.parametrize("P", [1, 65, 257])
def test_gradient_buffers_stay_in_bounds(gpu, monkeypatch, P):
    """hgs_raster_bwd with every workspace and gradient buffer between guards (tests/ws_guard.py), 0x00- and 0xFF-filled:
    intact guards (checked inside raster_chain), the same bits for both fills and for both routes."""
    import test_workspace_bounds_gpu as wb
    cam, scene, gc, gd = wb._case(P, seed=P % 89)
    inp = wb._inputs("h48", scene, gpu)
    run = lambda: [wb.raster_chain(cam, inp, 3, gc, gd, gpu, fill)[0] for fill in wb.FILLS]
    two, fused = _both_routes(monkeypatch, run)
    wb._assert_same(fused[0], fused[1], "fused")
    _assert_same_bits(f"guarded P={P}", two[0], fused[0])
