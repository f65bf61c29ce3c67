"""The frustum-cull rule without a GPU (tests/frustum_spec.py restates it): known answers of the planes, soundness of
the rule against the float32 geometry spec of the rasterizer's per-Gaussian pass -- nothing it would draw is dropped --
on inputs that DO catch the two cheaper rules, and that the cull removes a real share of the cut."""
import math
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import frustum_cases as fc
import frustum_spec as fs
from hgs import frustum, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _planes(cam, **kw):
    return fs.planes_spec(cam.world_view_transform.numpy(), cam.tanfovx, cam.tanfovy, fc.W, fc.H, **kw)


def _signed(planes, x):
    return planes[:, :3].astype(np.float64) @ np.asarray(x, dtype=np.float64) + planes[:, 3].astype(np.float64)


def test_identity_camera_planes_have_the_known_answers():
    cam = synth.make_camera(fc.W, fc.H)
    planes, rs = _planes(cam)
    assert planes.dtype == np.float32 and planes.shape == (5, 4)
    assert np.allclose(np.linalg.norm(planes[:, :3].astype(np.float64), axis=1), 1.0, atol=1e-6)
    scale = max(1.3, 1 + 36 / 160)
    assert scale == 1.3
    tx, ty = scale * cam.tanfovx, scale * cam.tanfovy
    assert np.all(_signed(planes, (0, 0, 0))[:4] == 0.0)                    # the camera centre is on the four side planes
    z, eps = 5.0, 1e-3
    # (point, the plane it is just outside of); the same point moved inwards by 2 eps is inside every plane
    for k, out_pt, in_pt in ((0, (-z * tx - eps, 0, z), (-z * tx + eps, 0, z)), (1, (z * tx + eps, 0, z), (z * tx - eps, 0, z)),
                             (2, (0, -z * ty - eps, z), (0, -z * ty + eps, z)), (3, (0, z * ty + eps, z), (0, z * ty - eps, z)),
                             (4, (0, 0, 0.2 - eps), (0, 0, 0.2 + eps))):
        so, si = _signed(planes, out_pt), _signed(planes, in_pt)
        assert so[k] < 0 and np.all(np.delete(so, k) > 0), (k, so)
        assert np.all(si > 0), (k, si)
    assert rs == pytest.approx(1.3865, abs=1e-4)                            # 60 degrees on 16:10
    assert _planes(cam, scale_modifier=2.0)[1] == pytest.approx(2 * rs) and _planes(cam, scale_modifier=0.5)[1] == rs
    # a small image widens the planes: 36 px of the narrower side
    p_small, _ = fs.planes_spec(cam.world_view_transform.numpy(), cam.tanfovx, cam.tanfovy, 64, 40)
    assert fs.fov_scale(64, 40) == pytest.approx(1.9)
    assert _signed(p_small, (-z * 1.9 * cam.tanfovx + eps, 0, z))[0] > 0 > _signed(p_small, (-z * 1.9 * cam.tanfovx - eps, 0, z))[0]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_the_package_builds_the_planes_of_the_spec(name):
    cam = fc.camera(name)
    for sm, near, wh in ((1.0, 0.2, (fc.W, fc.H)), (1.7, 0.5, (64, 40))):
        p_spec, rs_spec = fs.planes_spec(cam.world_view_transform.numpy(), cam.tanfovx, cam.tanfovy, *wh,
                                         scale_modifier=sm, near=near)
        p, rs = frustum.frustum_planes(cam.world_view_transform, cam.tanfovx, cam.tanfovy, *wh, scale_modifier=sm, near=near)
        assert p.dtype == torch.float32 and tuple(p.shape) == (5, 4) and not p.is_cuda
        # both are double computations rounded once: they may differ in the last bit of the sums
        assert np.allclose(p.numpy(), p_spec, rtol=0, atol=4 * np.finfo(np.float32).eps * max(1.0, float(np.abs(p_spec).max())))
        assert rs == pytest.approx(rs_spec, rel=1e-12)
    # the camera centre is on the side planes, and a point straight ahead is inside all five
    c = cam.camera_center.double().numpy()
    assert np.all(np.abs(_signed(p_spec, c)[:4]) < 1e-5)
    fwd = cam.world_view_transform.double().numpy()[:3, 2]
    assert np.all(_signed(fs.planes_spec(cam.world_view_transform.numpy(), cam.tanfovx, cam.tanfovy, fc.W, fc.H)[0],
                          c + 3.0 * fwd) > 0)


def test_bounds_contain_three_sigma_of_every_row():
    """Hand-built node list with several rows per node (this project's builder gives one): the centre is the mean of
    the means, every row's 3-sigma ball lies inside, and a node without rows is never outside a plane."""
    nodes, means, scales = fc.multi_row_case()
    b = fs.bounds_spec(nodes, means, scales)
    for n, (s, c) in enumerate(((0, 3), (3, 4), (7, 1), (8, 4))):
        assert np.allclose(b[n, :3], means[s:s + c].astype(np.float64).mean(0), atol=1e-6)
        reach = np.linalg.norm(means[s:s + c].astype(np.float64) - b[n, :3], axis=1) + 3 * scales[s:s + c].max(1)
        assert b[n, 3] == pytest.approx(reach.max(), rel=1e-6)
    assert np.isinf(b[4, 3]) and not fs.ball_outside(b, np.array([4]), np.array([0, 0, 1, -1e30], np.float32), 1.4)[0]


@pytest.fixture(scope="module")
def verdicts():
    """Per (camera, tau px): visible entries of the unculled cut and what the rule and the two cheaper rules drop."""
    h, _, bounds = fc.hier20k()
    nodes = h.nodes.numpy()
    out = {}
    for name in "ABC":
        for tau_px in fc.TAUS_PX:
            u = fc.unculled(name, tau_px)
            planes, rs = _planes(u["cam"])
            out[name, tau_px] = dict(
                n=len(u["ni"]), visible=u["radii"] > 0,
                rule=fs.culled_spec(nodes, bounds, u["ni"], planes, rs),
                unit_radius=fs.culled_spec(nodes, bounds, u["ni"], planes, 1.0),
                own_ball=fs.culled_spec(nodes, bounds, u["ni"], planes, rs, own_ball_only=True))
    return out


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("tau_px", fc.TAUS_PX)
def test_no_culled_entry_is_drawn(verdicts, name, tau_px):
    v = verdicts[name, tau_px]
    wrong = int((v["rule"] & v["visible"]).sum())
    print(f"{name} tau {tau_px}: cut {v['n']}, visible {int(v['visible'].sum())}, kept {int((~v['rule']).sum())}, "
          f"culled but drawn {wrong}")
    assert v["n"] > 1000 and int(v["rule"].sum()) > 0
    assert wrong == 0


def test_the_same_inputs_catch_the_two_cheaper_rules(verdicts):
    """radius_scale = 1 (no allowance for the off-axis growth of the footprint) and the node's own ball alone (no
    parent: the entry is a lerp of both rows) each drop entries that K1 draws -- the soundness test has teeth."""
    unit = {k: int((v["unit_radius"] & v["visible"]).sum()) for k, v in verdicts.items() if k[0] in "BC"}
    own = {k: int((v["own_ball"] & v["visible"]).sum()) for k, v in verdicts.items() if k[1] == 40.0}
    print("radius_scale = 1:", unit, "own ball only:", own)
    assert len(unit) == 4 and all(c > 0 for c in unit.values()), unit
    assert len(own) == 3 and all(c > 0 for c in own.values()), own


@pytest.mark.parametrize("name", ["B", "C"])
def test_the_cull_removes_at_least_half_of_the_cut_from_inside_the_scene(verdicts, name):
    v = verdicts[name, 3.0]
    kept, visible = int((~v["rule"]).sum()), int(v["visible"].sum())
    print(f"{name}: kept {kept / v['n']:.1%}, visible {visible / v['n']:.1%}")
    assert visible <= kept <= v["n"] // 2


def test_cut_view_spec_is_the_unculled_cut_minus_the_culled_entries():
    from oracle import lod_oracle as lo
    h, _, bounds = fc.hier20k()
    u = fc.unculled("C", 3.0)
    planes, rs = _planes(u["cam"])
    nodes, boxes = h.nodes.numpy(), h.boxes.numpy()
    cv = fs.cut_view_spec(nodes, boxes, bounds, u["tau"], u["cam"].camera_center.numpy(), planes, rs)
    assert cv["n_unculled"] == len(u["r"]) and 0 < cv["n"] < cv["n_unculled"]
    keep = ~cv["culled"]
    for got, ref in ((cv["render_indices"], u["r"]), (cv["parent_indices"], u["p"]), (cv["node_indices"], u["ni"]),
                     (cv["kids"], u["kids"])):
        assert np.array_equal(got, ref[keep])
    assert np.array_equal(cv["weights"].view(np.uint32), u["w"][keep].view(np.uint32))


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("c++filt")),
                    reason="needs hipcc (cross-compiles without a GPU) and c++filt")
def test_no_frustum_kernel_uses_scratch_or_doubles():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    rows = kernel_resources.collect([os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc", "lod_frustum.hip")])
    names = {r["kernel"] for r in rows}
    assert {"frustum_bounds_kernel", "frustum_mark_kernel", "frustum_cull_kernel", "frustum_emit_kernel"} <= names, names
    for r in rows:
        assert r["scratch"] == 0, (r["kernel"], r["scratch"])
        assert r["mix"]["valu_f64"] == 0, r["kernel"]
        assert r["waves_regs"] >= 8, (r["kernel"], r["vgpr"])


def test_cut_view_refuses_cpu_tensors_without_touching_the_gpu():
    nodes = torch.zeros(3, 7, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU tensor"):
        frustum.cut_view(nodes, torch.zeros(3, 2, 4), torch.zeros(3, 4), 0.1, torch.zeros(3), torch.zeros(5, 4), 1.4)
    with pytest.raises(ValueError, match="GPU tensor"):
        frustum.cull_bounds(nodes, torch.zeros(3, 3), torch.zeros(3, 3))
    with pytest.raises(ValueError):
        frustum.frustum_planes(torch.eye(4), 0.0, 0.5, 64, 64)
    assert math.isclose(frustum.frustum_planes(torch.eye(4), 0.5, 0.5, 640, 640)[1], math.sqrt(1.845 / 1.4225))
