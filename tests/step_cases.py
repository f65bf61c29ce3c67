"""Shared by tests/test_step_cpu.py, tests/test_step_gpu.py and scripts/bench_step.py (a helper module, not a test): the
cases of tests/golden/ref_step_golden.npz (the reference's train_single.py and train_post.py, unmodified, before and
after the block hgs.step replaces), seeded inputs at any size whose rows keep 1e-4 away from the clamp threshold, and
the comparisons both suites use."""
import math
import os

import numpy as np
import torch

from step_spec import NAMES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_step_golden.npz")
BAND = 1e-4           # tests keep every row this far (relative) from the clamp threshold; the contract's band is 1e-5
TOL = 2e-6            # float32 reference against float64 (tests/test_adam_cpu.py's bound)
ACCUM_TOL = 4 * 2.0 ** -23
EPS = 1e-15
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=5e-2, scaling=5e-3, rotation=1e-3)
SHAPES = lambda K: dict(xyz=(3,), f_dc=(1, 3), f_rest=(K, 3), opacity=(1,), scaling=(3,), rotation=(4,))


def golden_case_names():
    return [str(n) for n in np.load(GOLDEN)["case_names"]]


def load_case(name, device="cpu", dtype=None):
    """-> dict: params / grads / exp_avg / exp_avg_sq / after* (dict name -> tensor), steps, lrs, radii (compacted),
    visible, means2D_grad, max_radii2D / accum / denom (before; None for train_post.py) and their after values, and
    ``config``: the keyword arguments of the rule (lock_head, lock_tail, lock_mask, select, clamp)."""
    z = np.load(GOLDEN)

    def t(key, cast=True):
        x = torch.from_numpy(z[f"{name}.{key}"]).to(device)
        return x.to(dtype) if cast and dtype is not None and x.is_floating_point() else x
    P = z[f"{name}.before.xyz"].shape[0]
    single = name.startswith("single")
    sky = int(z[f"{name}.skybox_points"])
    c = dict(P=P, single=single,
             params={n: t(f"before.{n}") for n in NAMES}, grads={n: t(f"grad.{n}") for n in NAMES},
             exp_avg={n: t(f"before.{n}.exp_avg") for n in NAMES}, exp_avg_sq={n: t(f"before.{n}.exp_avg_sq") for n in NAMES},
             steps={n: float(z[f"{name}.before.{n}.step"]) for n in NAMES}, lrs={n: float(z[f"{name}.lr.{n}"]) for n in NAMES},
             after={n: t(f"after.{n}") for n in NAMES}, after_exp_avg={n: t(f"after.{n}.exp_avg") for n in NAMES},
             after_exp_avg_sq={n: t(f"after.{n}.exp_avg_sq") for n in NAMES},
             radii=t("radii"), visible=t("visible"), means2D_grad=t("means2D_grad"),
             max_radii2D=t("before.max_radii2D"), after_max_radii2D=t("after.max_radii2D"))
    for n in NAMES:
        assert float(z[f"{name}.after.{n}.step"]) == c["steps"][n] + 1
    if single:
        c.update(accum=t("before.accum"), denom=t("before.denom"), after_accum=t("after.accum"), after_denom=t("after.denom"))
        c["config"] = dict(lock_head=sky, select="opacity_grad", clamp=(float(np.float32(z[f"{name}.clamp_threshold"])), 0))
    else:
        mask = torch.zeros(P, dtype=torch.uint8, device=device)
        mask[t("anchors")] = 1
        c["config"] = dict(lock_tail=sky, lock_mask=mask, select="all", clamp=None)
    return c


def raw_radii(P, visible, radii):
    """The rasterizer's raw [P] radii from the compacted pair render() returns."""
    raw = torch.zeros(P, dtype=torch.int32, device=radii.device)
    raw[visible] = radii.to(torch.int32)
    return raw


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300)) if b.numel() else 0.0


def child_bound_ok(got, ref):
    """f-8's child bound, element-wise: |got - ref| <= 1e-5 |ref| + 1e-6 max|ref|.  -> (ok, worst excess)."""
    if not ref.numel():
        return True, 0.0
    tol = 1e-5 * ref.abs() + 1e-6 * ref.abs().max()
    err = (got - ref).abs()
    return bool((err <= tol).all()), float((err - tol).max())


def clear_band(scaling, threshold):
    """Moves, IN PLACE, the rows whose max_k exp(scaling) lies within 2 % of ``threshold`` (in log space) down by 0.05:
    one Adam step of the test inputs moves a scaling by less than 0.01 (lr 5e-3; the seeded second moments are bounded
    below), so every row is still far outside the 1e-4 band afterwards -- which the tests assert on the reference's
    values.  -> the number of rows touched."""
    if not scaling.shape[0]:
        return 0
    m = scaling.double().max(dim=1).values
    bad = ((m - math.log(threshold)).abs() < 0.02).nonzero().flatten()
    scaling[bad] -= 0.05
    return int(bad.numel())


def band_distance(scaling, threshold):
    if not scaling.shape[0]:
        return float("inf")
    m = torch.exp(scaling.double()).max(dim=1).values
    return float(((m - threshold).abs() / threshold).min())


def make_model(P, K, seed, device, *, visible_fraction=0.3):
    """Seeded parameters, gradients (zero opacity gradient outside the visible rows, as the rasterizer leaves it) and
    the statistics' inputs; an hgs.optim.Adam over the parameters is built by the caller.  -> dict."""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    shapes = SHAPES(K)
    params = {n: rn(P, *s) for n, s in shapes.items()}
    params["scaling"] = params["scaling"] * 0.7 - 3.0
    if visible_fraction >= 1:
        vis = torch.ones(P, dtype=torch.bool, device=device)
    elif visible_fraction <= 0:
        vis = torch.zeros(P, dtype=torch.bool, device=device)
    else:
        vis = torch.rand(P, generator=g, device=device) < visible_fraction
    radii = torch.randint(1, 60, (P,), generator=g, device=device, dtype=torch.int32) * vis.to(torch.int32)
    grads = {n: rn(P, *s) * 0.01 * vis.reshape(P, *([1] * len(s))) for n, s in shapes.items()}
    means2D_grad = rn(P, 3) * vis.reshape(P, 1)
    return dict(P=P, K=K, params=params, grads=grads, radii=radii, visible=vis.nonzero().flatten(),
                means2D_grad=means2D_grad, max_radii2D=torch.rand(P, generator=g, device=device) * 40.0,
                accum=rn(P, 1).abs() * 0.5, denom=torch.randint(0, 5, (P, 1), generator=g, device=device).float())


def build(model, moments_seed=None):
    """-> (params as nn.Parameters with .grad set, an hgs.optim.Adam over them with the reference's groups and, if
    ``moments_seed`` is given, non-trivial seeded moments at step 2)."""
    from hgs.optim import Adam
    params = {n: torch.nn.Parameter(model["params"][n].clone()) for n in NAMES}
    opt = Adam([dict(params=[params[n]], lr=LRS[n], name=n) for n in NAMES], lr=0.0, eps=EPS)
    if moments_seed is not None:
        dev = params["xyz"].device
        g = torch.Generator(device=dev).manual_seed(moments_seed)
        for n in NAMES:
            p = params[n]
            opt.state[p] = dict(step=torch.tensor(2.), exp_avg=torch.randn(p.shape, generator=g, device=dev) * 1e-2,
                                exp_avg_sq=(torch.randn(p.shape, generator=g, device=dev).abs() + 0.5) * 1e-4)
    for n in NAMES:
        params[n].grad = model["grads"][n].clone()
    return params, opt


def state_of(params, opt):
    """-> dict name -> (param, exp_avg, exp_avg_sq) clones."""
    out = {}
    for n in NAMES:
        st = opt.state.get(params[n], {})
        out[n] = (params[n].detach().clone(), st["exp_avg"].clone() if "exp_avg" in st else None,
                  st["exp_avg_sq"].clone() if "exp_avg_sq" in st else None)
    return out
