"""Shared by tests/test_densify_cpu.py and tests/test_densify_gpu.py (a helper module, not a test): the golden cases of
tests/golden/ref_densify_golden.npz, seeded inputs whose rows all keep 1e-4 away from the four thresholds, and the one
comparison both suites use."""
import os

import numpy as np
import torch

from densify_spec import NAMES, threshold_distance

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_densify_golden.npz")
BAND = 1e-4          # tests keep every row this far (relative, float64) from every threshold; the contract's band is 1e-5


def golden_case_names():
    return [str(n) for n in np.load(GOLDEN)["case_names"]]


def load_case(name, device="cpu"):
    """-> dict(tensors, moments, accum, radii, F, max_grad, min_opacity, d, noise, out, out_m, distance)."""
    z = np.load(GOLDEN)
    t = lambda key: torch.from_numpy(z[key]).to(device)
    F, max_grad, min_opacity, percent_dense, extent, dist = (float(v) for v in z[f"{name}.scalars"])
    return dict(
        tensors={n: t(f"{name}.in.{n}") for n in NAMES},
        moments={n: (t(f"{name}.in.{n}.exp_avg"), t(f"{name}.in.{n}.exp_avg_sq")) for n in NAMES},
        accum=t(f"{name}.accum"), radii=t(f"{name}.radii"), F=None if F < 0 else int(F), max_grad=max_grad,
        min_opacity=min_opacity, d=percent_dense * extent, percent_dense=percent_dense, extent=extent,
        noise=t(f"{name}.z"), distance=dist,
        totals=tuple(int(v) for v in z[f"{name}.totals"]),
        steps={n: float(z[f"{name}.step.{n}"]) for n in NAMES},
        out={n: t(f"{name}.out.{n}") for n in NAMES},
        out_m={n: (t(f"{name}.out.{n}.exp_avg"), t(f"{name}.out.{n}.exp_avg_sq")) for n in NAMES})


def call_args(case):
    return (case["tensors"], case["moments"], case["accum"], case["radii"], case["F"], case["max_grad"],
            case["min_opacity"], case["d"])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_same_result(got, ref, where=""):
    """got / ref: (tensors, moments, totals).  Row count and totals exact; blocks 1 and 2 and every copied column bit
    for bit; moments bit for bit; the children's xyz / scaling within the project's element-wise rule
    1e-5 |ref| + 1e-6 max|ref|."""
    (gt, gm, gtot), (rt, rm, rtot) = got, ref
    assert tuple(int(v) for v in gtot) == tuple(int(v) for v in rtot), (where, gtot, rtot)
    n_orig, n_clone, S, n_kept = (int(v) for v in rtot)
    rows = n_orig + n_clone + 2 * n_kept
    copied = n_orig + n_clone
    for n in NAMES:
        a, b = gt[n], rt[n]
        assert a.shape == b.shape and a.shape[0] == rows, (where, n, tuple(a.shape), tuple(b.shape), rows)
        if n in ("xyz", "scaling"):
            assert same_bits(a[:copied], b[:copied]), (where, n, "blocks 1 and 2")
            ka, kb = a[copied:], b[copied:]
            if kb.numel():
                tol = 1e-5 * kb.abs() + 1e-6 * kb.abs().max()
                err = (ka - kb).abs()
                assert bool((err <= tol).all()), (where, n, "children", float((err - tol).max()))
        else:
            assert same_bits(a, b), (where, n)
        assert (gm[n] is None) == (rm[n] is None), (where, n, "moments present")
        if rm[n] is not None:
            for what, x, y in zip(("exp_avg", "exp_avg_sq"), gm[n], rm[n]):
                assert same_bits(x, y), (where, n, what)
                assert not bool(x[n_orig:].any()), (where, n, what, "moments of new rows")


def make_inputs(P, K, seed, device, *, with_moments=True, max_grad=4.0, min_opacity=0.1):
    """Seeded inputs with roughly the class shares of the general golden case.  -> dict like load_case's (no outputs)
    plus ``redrawn``: the share of rows that fell into the 1e-4 band (float64, on the host) and were drawn again."""
    g = torch.Generator().manual_seed(seed)
    shapes = dict(xyz=(3,), f_dc=(1, 3), f_rest=(K, 3), opacity=(1,), scaling=(3,), rotation=(4,))

    def draw(n):
        opacity = torch.randn(n, 1, generator=g) * 1.5
        scaling = torch.randn(n, 3, generator=g) * 0.7 - 3.0
        accum = torch.randn(n, 1, generator=g).abs() * 0.4
        accum[torch.rand(n, generator=g) < 0.05] *= -1.0
        accum[torch.rand(n, generator=g) < 0.04] = float("nan")
        radii = torch.rand(n, generator=g) * 60.0
        radii[torch.rand(n, generator=g) < 0.1] = 0.0
        return opacity, scaling, accum, radii

    opacity, scaling, accum, radii = draw(P)
    # the median row's own m is a row's value: d sits 1e-3 above it, outside the band
    d = float(torch.exp(scaling).max(dim=1).values.median()) * 1.001 if P else 0.05
    redrawn = 0
    for _ in range(20):
        bad = (threshold_distance(accum, radii, opacity, scaling, max_grad, min_opacity, d) < BAND).nonzero().flatten()
        if bad.numel() == 0:
            break
        redrawn += int(bad.numel())
        opacity[bad], scaling[bad], accum[bad], radii[bad] = draw(int(bad.numel()))
    else:
        raise AssertionError("rows keep falling into the threshold band")
    # everything that does not decide a class is drawn where it will live (180 M floats at 1 M rows of K = 15)
    dg = torch.Generator(device=device).manual_seed(seed + 1)
    big = lambda *s: torch.randn(*s, generator=dg, device=device)
    tensors = {n: big(P, *s) for n, s in shapes.items()}
    tensors["opacity"], tensors["scaling"] = opacity.to(device), scaling.to(device)
    moments = {n: (big(P, *s) * 1e-2, big(P, *s).abs() * 1e-4) for n, s in shapes.items()} if with_moments else {}
    return dict(tensors=tensors, moments=moments, accum=accum.to(device), radii=radii.to(device), max_grad=max_grad,
                min_opacity=min_opacity, d=d, redrawn=redrawn / max(P, 1), generator=g)


def clear_band(tensors, accum, radii, max_grad, min_opacity, d, generator):
    """Re-draws, IN PLACE, accumulator, radius, opacity and scaling of the rows inside the 1e-4 band of any threshold
    (tensors on any device; the test is made in float64 on the host).  -> the share of rows that were touched."""
    P = accum.shape[0]
    touched = torch.zeros(P, dtype=torch.bool)
    for _ in range(20):
        dist = threshold_distance(accum.cpu(), radii.cpu(), tensors["opacity"].cpu(), tensors["scaling"].cpu(), max_grad,
                                  min_opacity, d)
        bad = (dist < BAND).nonzero().flatten()
        if bad.numel() == 0:
            return float(touched.sum()) / max(P, 1)
        touched[bad] = True
        n = int(bad.numel())
        dev = accum.device
        accum.view(-1)[bad.to(dev)] = (torch.randn(n, generator=generator).abs() * 0.4).to(dev)
        radii[bad.to(dev)] = (torch.rand(n, generator=generator) * 60.0).to(dev)
        tensors["opacity"].data[bad.to(dev)] = (torch.randn(n, 1, generator=generator) * 1.5).to(dev)
        tensors["scaling"].data[bad.to(dev)] = (torch.randn(n, 3, generator=generator) * 0.7 - 3.0).to(dev)
    raise AssertionError("rows keep falling into the threshold band")
