"""Raw-parameter path (include/hgs.h HGS_ACT_*, shs_rest): the op applies exp / normalize / sigmoid|abs
and reads features_dc / features_rest separately.  Checked against the oracle driven through the activation spec
(oracle.raster_oracle.activate_raw): indices bit-exact, pixels and gradients w.r.t. the RAW tensors <= 1e-5, and
against the op's own standard path fed with torch-activated inputs."""
import pytest
import torch

import parity as pa
from hgs import synth
from raw_cases import _compare, _oracle_raw, _raw_from_scene, _run_hip_raw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P,size,deg,act", [(1000, 128, 3, "sigmoid"), (1000, 128, 3, "abs"), (777, 96, 1, "sigmoid"),
                                            (5000, 256, 2, "sigmoid")])
def test_raw_path_matches_oracle(gpu, P, size, deg, act):
    cam = synth.make_camera(size, size)
    scene = synth.make_scene(P, cam, seed=3, sh_degree=deg)
    raw = _raw_from_scene(scene, seed=4, logit=(act == "sigmoid"))
    bg = torch.tensor([0.1, 0.2, 0.3])
    gc, gd = synth.upstream_grads(size, size, seed=1)
    hip = _run_hip_raw(raw, cam, bg, gc, gd, deg, act, gpu)
    _compare(hip, pa.verify(hip, _oracle_raw(raw, cam, bg, deg, act), gc, gd))


def test_raw_path_equals_standard_path_on_activated_inputs(gpu):
    """Same op, two entrances: raw tensors + fused activations vs torch activations + cat (what
    scene/gaussian_model.py:108-128 does).  Equal up to float32 rounding of the activations."""
    import diff_gaussian_rasterization as dgr
    W, H = 640, 360
    cam = synth.make_camera(W, H)
    scene = synth.make_scene(50_000, cam, seed=8)
    raw = _raw_from_scene(scene, seed=9)
    bg = torch.zeros(3)
    gc, gd = synth.upstream_grads(H, W, seed=1)
    hip = _run_hip_raw(raw, cam, bg, gc, gd, 3, "sigmoid", gpu, debug=False)
    leaves = {k: v.clone().to(gpu).requires_grad_(True) for k, v in raw.items()}
    m2 = torch.zeros(scene.P, 3, device=gpu, requires_grad=True)
    rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(cam, bg, 3, do_depth=True, device=gpu))
    color, radii, invd = dgr.GaussianRasterizer(rs)(
        means3D=leaves["xyz"], means2D=m2, shs=torch.cat([leaves["f_dc"], leaves["f_rest"]], 1),
        opacities=torch.sigmoid(leaves["opacity"]), scales=torch.exp(leaves["scaling"]),
        rotations=torch.nn.functional.normalize(leaves["rotation"]))
    ((color * gc.to(gpu)).sum() + (invd * gd.to(gpu)).sum()).backward()
    assert (radii.cpu() != hip["radii"]).float().mean() < 1e-4      # activations differ in the last float32 bit
    assert pa.err_stats(color.detach().cpu(), hip["color"])["l2"] < 1e-5
    for k in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"):
        st = pa.err_stats(leaves[k].grad.cpu(), hip["grads"][k])
        assert st["l2"] < 1e-4, (k, st)


def test_raw_path_argument_checks(gpu):
    import diff_gaussian_rasterization as dgr
    cam = synth.make_camera(64, 64)
    scene = synth.make_scene(10, cam, seed=0).to(gpu)
    rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(cam, torch.zeros(3), 3, device=gpu))
    m2 = torch.zeros(10, 3, device=gpu)
    with pytest.raises(RuntimeError):      # features_dc must be [P,1,3]
        dgr.GaussianRasterizer(rs).forward_raw(scene.means3D, m2, scene.shs[:, :2].contiguous(),
                                               scene.shs[:, 2:].contiguous(), scene.opacities, scene.scales,
                                               scene.rotations)
    with pytest.raises(RuntimeError):
        dgr.GaussianRasterizer(rs).forward_raw(scene.means3D, m2, scene.shs[:, :1].contiguous(),
                                               scene.shs[:, 1:].contiguous(), scene.opacities, scene.scales,
                                               scene.rotations, opacity_activation="tanh")
    # a contiguous slice whose first byte is not 16-byte aligned (12-byte rows) is refused, not mis-read
    dc11 = torch.zeros(11, 1, 3, device=gpu)
    with pytest.raises(RuntimeError, match="16-byte"):
        dgr.GaussianRasterizer(rs).forward_raw(scene.means3D, m2, dc11[1:], scene.shs[:, 1:].contiguous(),
                                               scene.opacities, scene.scales, scene.rotations)
