"""Generates tests/golden/ref_densify_golden.npz by running the REFERENCE's own adaptive density control:
scene/gaussian_model.py is plain Python, so GaussianModel is imported from the reference checkout HGS_REFERENCE names
(on the CPU stand-ins of tests/harness/cpu_backends.py, under the harness's CudaToCpu mode) and its
``densify_and_prune`` is called on seeded float32 inputs.  ``torch.normal`` is replaced by ``mean + z * std`` with a
recorded ``z`` for the duration of the call, which is the only way to know the noise the split children got.  Run in
the build container:

    HGS_REFERENCE=<checkout> python tests/golden/make_densify_golden.py

Stored per case (numbers only): the inputs as the optimizer holds them, their Adam moments after two real optimizer
steps, accumulator, radii, the scalars, ``z``, the reference's outputs and moments, and the smallest relative distance
of any row to any of the four thresholds in float64.  A case whose distance is below 1e-4 is re-seeded: the contract
 lets a row within 1e-5 of a threshold take either class, and the fixture must not depend on
which.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["HGS_REFERENCE"]
sys.path[:0] = [REF, os.path.join(ROOT, "tests", "shims"), os.path.join(ROOT, "hierarchical-3d-gaussians_amd"), ROOT,
                os.path.join(ROOT, "tests")]

from harness import cpu_backends                       # noqa: E402
from harness.run_reference_script import CudaToCpu     # noqa: E402
from densify_spec import NAMES, threshold_distance     # noqa: E402

ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
             rotation="_rotation")
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=5e-2, scaling=5e-3, rotation=1e-3)
PERCENT_DENSE = 0.01
MIN_DISTANCE = 1e-4

# name, rows, K, scaffold_points, optimizer, max_grad, min_opacity, seed
CASES = [
    ("general", 300, 15, 40, "our", 4.0, 0.1, 101),
    ("no_scaffold_torch_adam", 160, 3, None, "torch", 4.0, 0.05, 102),
    ("prune_only", 96, 3, 10, "our", 1e9, 0.1, 103),
    ("min_opacity_03", 200, 3, 16, "our", 4.0, 0.3, 104),
    ("all_protected", 64, 3, 64, "our", 4.0, 0.1, 105),
]


def make_inputs(P, K, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = dict(xyz=(3,), f_dc=(1, 3), f_rest=(K, 3), opacity=(1,), scaling=(3,), rotation=(4,))
    t = {n: torch.randn(P, *s, generator=g) for n, s in shapes.items()}
    t["opacity"] = t["opacity"] * 1.5
    t["scaling"] = t["scaling"] * 0.7 - 3.0
    accum = torch.randn(P, 1, generator=g).abs() * 0.4
    accum[torch.rand(P, generator=g) < 0.05] *= -1.0            # the split test takes no absolute value
    accum[torch.rand(P, generator=g) < 0.04] = float("nan")
    radii = torch.rand(P, generator=g) * 60.0
    radii[torch.rand(P, generator=g) < 0.1] = 0.0
    grads = [{n: torch.randn(P, *s, generator=g) * 0.01 for n, s in shapes.items()} for _ in range(2)]
    return t, accum, radii, grads, g


def run_case(GaussianModel, OurAdam, name, P, K, F, optimizer, max_grad, min_opacity, seed):
    t, accum, radii, grads, g = make_inputs(P, K, seed)
    extent = float(torch.exp(t["scaling"]).max(dim=1).values.median()) / PERCENT_DENSE
    m = GaussianModel(3)
    for n in NAMES:
        setattr(m, ATTRS[n], torch.nn.Parameter(t[n].clone()))
    groups = [dict(params=[getattr(m, ATTRS[n])], lr=LRS[n], name=n) for n in NAMES]
    m.optimizer = OurAdam(groups, lr=0.0, eps=1e-15) if optimizer == "our" else torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for gr in grads:                                            # two real steps: non-trivial moments
        for n in NAMES:
            getattr(m, ATTRS[n]).grad = gr[n].clone()
        m.optimizer.step(torch.empty(0)) if optimizer == "our" else m.optimizer.step()
    m.percent_dense, m.scaffold_points = PERCENT_DENSE, F
    m.xyz_gradient_accum, m.denom, m.max_radii2D = accum.clone(), torch.ones(P, 1), radii.clone()
    out = {}
    for n in NAMES:
        p = getattr(m, ATTRS[n])
        out[f"{name}.in.{n}"] = p.detach().clone().numpy()
        out[f"{name}.in.{n}.exp_avg"] = m.optimizer.state[p]["exp_avg"].clone().numpy()
        out[f"{name}.in.{n}.exp_avg_sq"] = m.optimizer.state[p]["exp_avg_sq"].clone().numpy()
        out[f"{name}.step.{n}"] = np.array(float(m.optimizer.state[p]["step"]))
    now = {n: getattr(m, ATTRS[n]).detach() for n in NAMES}
    dist = float(threshold_distance(accum, radii, now["opacity"], now["scaling"], max_grad, min_opacity,
                                    PERCENT_DENSE * extent).min())
    if dist < MIN_DISTANCE:
        return None
    recorded = []
    real_normal = torch.normal

    def recorded_normal(mean, std, **kw):
        z = torch.randn(std.shape, generator=g)
        recorded.append(z)
        return mean + z * std

    torch.normal = recorded_normal
    try:
        with CudaToCpu():
            m.densify_and_prune(max_grad, min_opacity, extent)
    finally:
        torch.normal = real_normal
    assert len(recorded) == 1
    out[f"{name}.accum"], out[f"{name}.radii"], out[f"{name}.z"] = accum.numpy(), radii.numpy(), recorded[0].numpy()
    out[f"{name}.scalars"] = np.array([-1 if F is None else F, max_grad, min_opacity, PERCENT_DENSE, extent, dist],
                                      dtype=np.float64)
    for n in NAMES:
        p = getattr(m, ATTRS[n])
        assert m.optimizer.param_groups[NAMES.index(n)]["params"][0] is p
        out[f"{name}.out.{n}"] = p.detach().numpy()
        out[f"{name}.out.{n}.exp_avg"] = m.optimizer.state[p]["exp_avg"].numpy()
        out[f"{name}.out.{n}.exp_avg_sq"] = m.optimizer.state[p]["exp_avg_sq"].numpy()
        assert float(m.optimizer.state[p]["step"]) == float(out[f"{name}.step.{n}"])
    P_new = m._xyz.shape[0]
    # the four totals, counted here in float64 numpy (every row is MIN_DISTANCE away from every threshold, so float64
    # and the reference's float32 agree on every class) and cross-checked against what the reference produced
    a64 = np.nan_to_num(accum.numpy().astype(np.float64).reshape(P), nan=0.0)
    o64 = 1.0 / (1.0 + np.exp(-out[f"{name}.in.opacity"].astype(np.float64).reshape(P)))
    m64 = np.exp(out[f"{name}.in.scaling"].astype(np.float64)).max(axis=1)
    w64 = radii.numpy().astype(np.float64) * o64 ** 0.2
    free = np.arange(P) >= (F or 0)
    clone = (np.abs(a64) * w64 >= max_grad) & (o64 > 0.15) & (m64 <= PERCENT_DENSE * extent) & free
    split = (a64 * w64 >= max_grad) & (o64 > 0.15) & (m64 > PERCENT_DENSE * extent) & free
    low = o64 < min_opacity
    totals = [int((~split & ~(low & free)).sum()), int((clone & ~low).sum()), int(split.sum()), int((split & ~low).sum())]
    assert totals[2] * 2 == recorded[0].shape[0] and totals[0] + totals[1] + 2 * totals[3] == P_new, (totals, P_new)
    out[f"{name}.totals"] = np.array(totals, dtype=np.int64)
    assert tuple(m.xyz_gradient_accum.shape) == (P_new, 1) and tuple(m.denom.shape) == (P_new, 1)
    assert tuple(m.max_radii2D.shape) == (P_new,)
    assert not m.xyz_gradient_accum.any() and not m.denom.any() and not m.max_radii2D.any()
    print(f"{name}: P {P} -> {P_new}, totals {totals}, clone rows {int(clone.sum())}, threshold distance {dist:.2e}, seed {seed}")
    return out


def main():
    cpu_backends.install()
    torch.cuda.empty_cache = lambda: None
    with CudaToCpu():
        from scene.gaussian_model import GaussianModel
        from scene.OurAdam import Adam as OurAdam
    out = {"case_names": np.array([c[0] for c in CASES])}
    for name, P, K, F, optimizer, max_grad, min_opacity, seed in CASES:
        for attempt in range(50):
            got = run_case(GaussianModel, OurAdam, name, P, K, F, optimizer, max_grad, min_opacity, seed + 1000 * attempt)
            if got is not None:
                break
        else:
            raise SystemExit(f"{name}: no seed keeps every row {MIN_DISTANCE} away from the thresholds")
        out.update(got)
    path = os.path.join(HERE, "ref_densify_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
