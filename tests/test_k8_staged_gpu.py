"""K8's LDS-DMA staging (csrc/preprocess.hip: k8_sum_runs<true>, k8_stage_inputs, the Jacobian rows of the fused kernel)
against the loads through registers.

By default the K8 kernels bring a wave's instance records, its 64 rows of per-Gaussian inputs and (fused kernel) its
Jacobian rows into LDS by DMA; HGS_K8_STAGE=0, read on every call, selects the kernels that load them through registers
as before.  The same values enter the same operations in the same order, so every comparison here is ``torch.equal`` on
int32 views, with the fused kernel and (HGS_K8_FUSE=0) with K8a + K8b.  What the gradients are worth is the business of
the oracle suites; here only the two routes are held together."""
import pytest
import torch

import parity as pa
from hgs import synth

pytestmark = pytest.mark.gpu

BG = torch.tensor([0.1, 0.2, 0.3])


def _routes(monkeypatch, run, fuse):
    """run() with the register loads, then with the default (staged) route; ``fuse`` False keeps K8a and K8b apart."""
    if not fuse:
        monkeypatch.setenv("HGS_K8_FUSE", "0")
    monkeypatch.setenv("HGS_K8_STAGE", "0")
    plain = run()
    monkeypatch.delenv("HGS_K8_STAGE")
    staged = run()
    monkeypatch.delenv("HGS_K8_FUSE", raising=False)
    return plain, staged


def _assert_same_bits(name, plain, staged):
    assert set(plain) == set(staged) and plain, name
    for k in sorted(plain):
        a, b = plain[k], staged[k]
        assert torch.isfinite(a).all(), (name, k)
        ai, bi = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
        if not torch.equal(ai, bi):
            bad = torch.nonzero((ai != bi).reshape(a.shape[0], -1).any(1)).flatten()
            raise AssertionError(f"{name}: dL/d{k} differs between the routes on {bad.numel()} rows, first {bad[:8].tolist()}")


def _pair(monkeypatch, name, fuse, scene, cam, gc, gd, gpu, **kw):
    kw.setdefault("debug", False)
    plain, staged = _routes(monkeypatch, lambda: pa.run_hip(scene, cam, BG, gc, gd, gpu, grad_mask=None, **kw), fuse)
    _assert_same_bits(name, plain["grads"], staged["grads"])
    return staged


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 777])
def test_partial_waves_and_workgroups(gpu, monkeypatch, P, fuse):
    """Full waves take their inputs by DMA, the last wave of a P off the wave grid lane by lane."""
    cam, scene, gc, gd = pa.default_case(P, 53, 37, seed=P)
    hip = _pair(monkeypatch, f"P={P} fuse={fuse}", fuse, scene, cam, gc, gd, gpu)
    assert P == 1 or float(hip["grads"]["shs"].abs().max()) > 0
    if P == 777:        # a wave's records start at an even or an odd record: the DMA's two shifts (0 and 8 bytes)
        tt = hip["views"]["tiles_touched"].long()
        starts = (torch.cumsum(tt, 0) - tt)[0::64]
        assert {int(s) % 2 for s in starts} == {0, 1}, starts.tolist()


@pytest.mark.parametrize("fuse", [True, False])
def test_culled_block_and_empty_wave(gpu, monkeypatch, fuse):
    """A workgroup whose 256 rows are all culled (no records, no chain: its DMA is still retired before the buffer is
    reused) and a wave without instances between two waves that have some (its range of records is empty)."""
    P, W, H = 777, 53, 37
    cam = synth.make_camera(W, H)
    scene = synth.make_scene(P, cam, seed=31)
    scene.means3D[256:512, 2] = -scene.means3D[256:512, 2].abs() - 1.0      # workgroup 1: behind the camera
    scene.means3D[64:128, 2] = -scene.means3D[64:128, 2].abs() - 1.0        # wave 1 of workgroup 0
    gc, gd = synth.upstream_grads(H, W, seed=3)
    hip = _pair(monkeypatch, f"culled fuse={fuse}", fuse, scene, cam, gc, gd, gpu)
    tt = hip["views"]["tiles_touched"]
    assert not tt[256:512].any() and not tt[64:128].any()
    assert tt[:64].any() and tt[128:192].any() and tt[512:].any()
    for k, v in hip["grads"].items():
        assert not v[256:512].any() and not v[64:128].any(), k


def _large_scene(W, H):
    cam = synth.make_camera(W, H)
    scene = synth.make_scene(300, cam, seed=41, s_px=(20.0, 60.0))
    scene.opacities = scene.opacities * 0.35
    return cam, scene


@pytest.mark.parametrize("presum", [None, "1", "0"])
@pytest.mark.parametrize("fuse", [True, False])
def test_several_passes_per_wave(gpu, monkeypatch, fuse, presum):
    """300 large Gaussians on 12 tiles: a wave's 64 runs hold more records than the 254 of a DMA pass (256 of a register
    pass), so runs straddle pass boundaries -- at different records on the two routes.  HGS_K8_PRESUM=1 puts the worklist kernels in front (no run here is long enough for them to change a record)."""
    W, H = 64, 48
    cam, scene = _large_scene(W, H)
    gc, gd = synth.upstream_grads(H, W, seed=9)
    if presum is not None:
        monkeypatch.setenv("HGS_K8_PRESUM", presum)
    hip = _pair(monkeypatch, f"large fuse={fuse} presum={presum}", fuse, scene, cam, gc, gd, gpu)
    tt = hip["views"]["tiles_touched"].long()
    per_wave = [int(tt[i:i + 64].sum()) for i in range(0, 300, 64)]
    assert max(per_wave) > 2 * 256, per_wave                           # three passes and more on either route


def test_long_runs_next_to_staged_inputs(gpu, monkeypatch):
    """L > 6 P: waves with a long run add presummed segments and walk their short runs in global memory -- they stage no
    records, only their inputs and Jacobians."""
    W = H = 512
    cam = synth.make_camera(W, H)
    scene = synth.make_scene(300, cam, seed=41, s_px=(4.0, 90.0))
    scene.opacities = scene.opacities * 0.35
    gc, gd = synth.upstream_grads(H, W, seed=9)
    hip = _pair(monkeypatch, "presum", True, scene, cam, gc, gd, gpu)
    tt = hip["views"]["tiles_touched"].long()
    assert hip["L"] > 6 * 300 and int((tt > 48).sum()) >= 1


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("which", ["means3D", "scales", "opacities"])
def test_input_views_with_a_storage_offset(gpu, monkeypatch, which, fuse):
    """One input as a contiguous view one float into its storage: its base is not 16-byte aligned, so no input goes by
    DMA and every wave loads its rows lane by lane (the records and Jacobians are still staged).  (Of the staged inputs
    these three can arrive so: the call refuses rotations that are not 16-byte aligned, and the flags are the
    workspace's.)"""
    import diff_gaussian_rasterization as dgr
    P, W, H = 300, 53, 37
    cam, scene, gc, gd = pa.default_case(P, W, H, seed=7)
    names = ("means3D", "shs", "opacities", "scales", "rotations")

    def run():
        lv = {}
        for n in names:
            t = getattr(scene, n).to(gpu)
            if n == which:
                buf = torch.zeros(t.numel() + 1, device=gpu)
                buf[1:] = t.reshape(-1)
                t = buf[1:].view(t.shape)
                assert t.data_ptr() % 16 == 4 and t.is_contiguous()
            lv[n] = t.detach().requires_grad_(True)
        m2 = torch.zeros(P, 3, device=gpu, requires_grad=True)
        rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(cam, BG, 3, device=gpu))
        color, _, invd = dgr.GaussianRasterizer(rs)(means3D=lv["means3D"], means2D=m2, shs=lv["shs"], opacities=lv["opacities"],
                                                    scales=lv["scales"], rotations=lv["rotations"])
        ((color * gc.to(gpu)).sum() + (invd * gd.to(gpu)).sum()).backward()
        torch.cuda.synchronize()
        out = {n: v.grad.detach().cpu() for n, v in lv.items()}
        out["means2D"] = m2.grad.detach().cpu()
        return out

    aligned = pa.run_hip(scene, cam, BG, gc, gd, gpu, grad_mask=None, debug=False)["grads"]
    plain, staged = _routes(monkeypatch, run, fuse)
    _assert_same_bits(f"{which} offset fuse={fuse}", plain, staged)
    _assert_same_bits(f"{which} offset against aligned inputs", aligned, staged)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("do_depth", [True, False])
def test_depth_gradient_on_and_off(gpu, monkeypatch, do_depth, fuse):
    cam, scene, gc, gd = pa.default_case(600, 64, 48, seed=17)
    _pair(monkeypatch, f"depth={do_depth} fuse={fuse}", fuse, scene, cam, gc, gd, gpu, do_depth=do_depth)


@pytest.mark.parametrize("act", ["sigmoid", "abs"])
def test_activations_from_staged_raw_values(gpu, monkeypatch, act):
    """The raw entrance (split SH: K8a + K8b): exp, normalisation and sigmoid | abs applied to values read from LDS."""
    from raw_cases import _raw_from_scene, _run_hip_raw
    cam = synth.make_camera(64, 48)
    scene = synth.make_scene(600, cam, seed=3)
    raw = _raw_from_scene(scene, seed=4, logit=(act == "sigmoid"))
    gc, gd = synth.upstream_grads(48, 64, seed=1)
    plain, staged = _routes(monkeypatch, lambda: _run_hip_raw(raw, cam, BG, gc, gd, 3, act, gpu, debug=False), True)
    _assert_same_bits(f"raw {act}", plain["grads"], staged["grads"])
    assert all(bool(v.any()) for v in staged["grads"].values())


def test_precomputed_covariance(gpu, monkeypatch):
    """No scales or rotations: their slots of the staged block stay unfilled and unread."""
    cam, scene, gc, gd = pa.default_case(300, 64, 48, seed=24)
    cov = torch.eye(3).mul(1e-3)[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]].repeat(scene.P, 1).contiguous()
    hip = _pair(monkeypatch, "cov3D_precomp", True, scene, cam, gc, gd, gpu, cov3D_precomp=cov)
    assert hip["grads"]["cov3D_precomp"].any()


def test_accumulated_gradients_through_a_context(gpu, monkeypatch):
    """accumulate_grads (K8a<ACC> + K8b<ACC>): two views added into the buffers of a RasterContext."""
    import diff_gaussian_rasterization as dgr
    from hgs import dp
    W, H, P = 64, 48, 300
    scene = synth.make_scene(P, synth.make_camera(W, H), seed=25)
    cams = [synth.orbit_camera(W, H, j, 2, radius=0.3) for j in range(2)]
    gc, gd = synth.upstream_grads(H, W, seed=4)
    names = ("means3D", "shs", "opacities", "scales", "rotations")

    def run():
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
        torch.cuda.synchronize()
        return {n: bucket.views[n].detach().cpu().clone() for n in names}

    plain, staged = _routes(monkeypatch, run, True)
    _assert_same_bits("accumulated", plain, staged)
    assert all(bool(v.any()) for v in staged.values())
