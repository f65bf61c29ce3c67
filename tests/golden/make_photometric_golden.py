"""Generates tests/golden/ref_photometric_golden.npz by running the REFERENCE's own loss code in float64 on the CPU:
``utils.loss_utils.l1_loss`` and ``ssim`` are imported from the reference checkout HGS_REFERENCE names, and the
exposure-and-clamp lines are run by calling its ``gaussian_renderer.render`` (on the CPU stand-ins of
tests/harness/cpu_backends.py, under the harness's CudaToCpu mode) with a stand-in rasterizer that returns the recorded
image ``r``.  Run in the build container:

    HGS_REFERENCE=<checkout> python tests/golden/make_photometric_golden.py

What exists only inside the reference's ``training()`` functions is stated here in this file's own words: the mask
multiply (train_single.py:102-104), the lambda mix (:108) and the inverse-depth term (:115-117).  ``render_post`` and
``render_coarse`` need a hierarchy around them; their exposure lines (gaussian_renderer/__init__.py:279-285) are the
same two as ``render``'s (:115-118), so the train_post-shaped case calls ``render`` with an exposure that does not
require grad, and the train_coarse-shaped case takes ``r`` as it is (``render_coarse`` applies neither exposure nor
clamp).

Stored per case (numbers only, float64): the inputs, lambda, depth weight, the four loss terms and autograd's gradients
of the loss with respect to r, the exposure and the inverse depth.  The inputs come from tests/photometric_cases.py,
repaired so that no pixel sits on a knife edge of the definition.  Note: the reference builds
its SSIM window in float32 (loss_utils.py:23-31) and casts it to the image's dtype, so these numbers carry that window;
tests/test_photometric_cpu.py restates it when it compares.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["HGS_REFERENCE"]
sys.path[:0] = [REF, os.path.join(ROOT, "tests", "shims"), os.path.join(ROOT, "hierarchical-3d-gaussians_amd"), ROOT,
                os.path.join(ROOT, "tests")]

from harness import cpu_backends                       # noqa: E402
from harness.run_reference_script import CudaToCpu     # noqa: E402
import photometric_cases as pc                         # noqa: E402

SHAPE = (3, 40, 56)
LAMBDA = 0.2                       # arguments/__init__.py: lambda_dssim
# name, seed, exposure, exposure requires grad, identity exposure, mask, depth, clamp, depth weight
CASES = [
    ("exposure_mask_depth", 11, True, True, False, True, True, True, 0.7),
    ("identity_zero_background", 12, True, True, True, True, True, True, 0.7),
    ("train_post", 13, True, False, False, True, False, True, 0.0),
    ("train_coarse", 14, False, False, False, True, False, False, 0.0),
]


def rendered_by_the_reference(render, r, exposure):
    """gaussian_renderer.render's output for a rasterizer that returns r: the exposure transform and the clamp."""
    import gaussian_renderer as gr

    class Rasterizer:
        def __init__(self, raster_settings):
            pass

        def __call__(self, **kw):
            return r, torch.ones(4, dtype=torch.int32), torch.zeros(1, *r.shape[1:], dtype=r.dtype)

    z = torch.zeros(4, 3, dtype=r.dtype)
    cam = types.SimpleNamespace(FoVx=1.0, FoVy=1.0, image_height=r.shape[1], image_width=r.shape[2],
                                world_view_transform=torch.eye(4), full_proj_transform=torch.eye(4),
                                camera_center=torch.zeros(3), image_name="view")
    model = types.SimpleNamespace(get_xyz=z, _xyz=z, active_sh_degree=0, max_sh_degree=0, get_opacity=z[:, :1],
                                  get_scaling=z, get_rotation=torch.zeros(4, 4), get_features=torch.zeros(4, 1, 3),
                                  get_exposure_from_name=lambda name: exposure)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    saved = gr.GaussianRasterizer, gr.GaussianRasterizationSettings
    gr.GaussianRasterizer, gr.GaussianRasterizationSettings = Rasterizer, (lambda **kw: kw)
    try:
        return render(cam, model, pipe, torch.zeros(3), use_trained_exp=exposure is not None)["render"]
    finally:
        gr.GaussianRasterizer, gr.GaussianRasterizationSettings = saved


def run_case(render, l1_loss, ssim, name, seed, exposure, exposure_grad, identity, mask, depth, clamp, depth_weight):
    inp = pc.make(SHAPE, seed=seed, exposure=exposure, mask=mask, depth=depth, identity=identity, clamp=clamp)
    assert pc.band_counts(inp) == (0, 0, 0)
    t = {k: v.double() for k, v in inp.items() if isinstance(v, torch.Tensor)}
    r = t["rendered"].clone().requires_grad_(True)
    E = t.get("exposure")
    if E is not None and exposure_grad:
        E = E.clone().requires_grad_(True)
    d = t["invdepth"].clone().requires_grad_(True) if depth else None
    with CudaToCpu():
        image = rendered_by_the_reference(render, r, E) if clamp else r
        if mask:
            image = image * t["alpha_mask"]
        Ll1 = l1_loss(image, t["gt"])
        s = ssim(image, t["gt"])
    loss = (1.0 - LAMBDA) * Ll1 + LAMBDA * (1.0 - s)
    D = torch.zeros((), dtype=torch.float64)
    if depth:
        D = torch.abs((d - t["mono_invdepth"]) * t["depth_mask"]).mean()
        loss = loss + depth_weight * D
    loss.backward()
    out = {f"{name}.in.{k}": v.numpy() for k, v in t.items()}
    out[f"{name}.scalars"] = np.array([LAMBDA, depth_weight, float(clamp), float(exposure_grad)], dtype=np.float64)
    for k, v in (("loss", loss), ("l1", Ll1), ("ssim", s), ("depth", D)):
        out[f"{name}.out.{k}"] = v.detach().numpy()
    out[f"{name}.out.grad_rendered"] = r.grad.numpy()
    if E is not None and exposure_grad:
        out[f"{name}.out.grad_exposure"] = E.grad.numpy()
    if depth:
        out[f"{name}.out.grad_invdepth"] = d.grad.numpy()
    print(f"{name}: loss {loss.item():.9f} L1 {Ll1.item():.9f} SSIM {s.item():.9f} D {D.item():.9f}")
    return out


def main():
    cpu_backends.install()
    with CudaToCpu():
        from gaussian_renderer import render
        from utils.loss_utils import l1_loss, ssim
    out = {"case_names": np.array([c[0] for c in CASES])}
    for case in CASES:
        out.update(run_case(render, l1_loss, ssim, *case))
    path = os.path.join(HERE, "ref_photometric_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
