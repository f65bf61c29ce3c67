#!/usr/bin/env python
"""Fused densify-and-prune figures, one JSON line per row count:

  fused_ms    hgs.densify.densify_and_prune_tensors: plan launch, one host wait for the four totals, apply launch
  spec_ms     tests/densify_spec.py, this project's whole-array torch statement of the same rule, on the same device
              and inputs.  It is NOT the reference's own method chain (which indexes by boolean mask per tensor in three
              passes and cannot be run here); it is the baseline because it is what can be run next to the kernels.
  Both contain host waits, so the figure is the HOST clock around a call that ends in a synchronise (the device events
  inside it are printed too); warm-up first, the two alternated over --reps repetitions: median, minimum, maximum.
  peak_bytes  torch.cuda.max_memory_allocated above the inputs during one call of each (the caller keeps the inputs, so
              both hold old + new); fused_model_peak_bytes: the same for hgs.densify.densify_and_prune on a model that
              owns the inputs, where every group's old tensors are released as soon as its new ones exist
  bytes       the traffic floor: E = 3 (14 + 3K) floats per row (parameters and both moments) read for P rows and
              written for P' rows, plus the plan's 24 B read and 8 B written per row
  bound_us    bytes over the measured HBM rate (6.29 TB/s, MI355X_MICROARCH: float4 copy); byte_bound_share = bound_us
              over the fused median

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (e.g. --reps 2 --only fused).

    python scripts/bench_densify.py [--rows 375000 1000000 8000000] [--K 15] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hgs import densify                             # noqa: E402
from densify_spec import classes, densify_and_prune_spec     # noqa: E402

HBM_BYTES_PER_S = 6.29e12
MAX_GRAD, MIN_OPACITY = 4.0, 0.1


def inputs(P, K, dev, seed=0):
    """The distributions of the general golden case (tests/golden/make_densify_golden.py): about 11 % of the rows are
    cloned, 10 % split and 4 % pruned."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    ru = lambda *s: torch.rand(*s, generator=g, device=dev)
    shapes = dict(xyz=(3,), f_dc=(1, 3), f_rest=(K, 3), opacity=(1,), scaling=(3,), rotation=(4,))
    tensors = {n: rn(P, *s) for n, s in shapes.items()}
    tensors["opacity"] *= 1.5
    tensors["scaling"] = tensors["scaling"] * 0.7 - 3.0
    moments = {n: (rn(P, *s) * 1e-2, rn(P, *s).abs() * 1e-4) for n, s in shapes.items()}
    accum = rn(P, 1).abs() * 0.4
    accum[ru(P) < 0.05] *= -1.0
    accum[ru(P) < 0.04] = float("nan")
    radii = ru(P) * 60.0
    radii[ru(P) < 0.1] = 0.0
    d = float(torch.exp(tensors["scaling"]).max(dim=1).values.median())
    S = int(classes(accum, radii, tensors["opacity"], tensors["scaling"], 0, MAX_GRAD, MIN_OPACITY, d)[1].sum())
    return (tensors, moments, accum, radii, 0, MAX_GRAD, MIN_OPACITY, d), rn(2 * S, 3)


def timed(fn, args, noise):
    """-> (host ms around call + synchronise, device ms between events inside it, totals)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn(*args, noise=noise)
    e1.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) * 1e3
    return host, e0.elapsed_time(e1), out[2]


def peak_above_inputs(fn, args, noise):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn(*args, noise=noise)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def model_peak(call_args, noise):
    """Peak above the inputs of the model-level call; CONSUMES call_args' tensors (the model owns them afterwards)."""
    import types
    tensors, moments, accum, radii, F, max_grad, min_opacity, d = call_args
    attrs = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
                 rotation="_rotation")
    params = {n: torch.nn.Parameter(t) for n, t in tensors.items()}
    opt = types.SimpleNamespace(
        param_groups=[dict(params=[params[n]], name=n) for n in densify.NAMES],
        state={params[n]: dict(step=torch.tensor(1.0), exp_avg=moments[n][0], exp_avg_sq=moments[n][1]) for n in params})
    model = types.SimpleNamespace(optimizer=opt, xyz_gradient_accum=accum, denom=torch.zeros_like(accum),
                                  max_radii2D=radii, percent_dense=0.01, scaffold_points=None,
                                  **{attrs[n]: params[n] for n in params})
    tensors.clear()
    moments.clear()
    del params, opt, tensors, moments, accum, radii, call_args
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    densify.densify_and_prune(model, max_grad, min_opacity, d / 0.01, noise=noise)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="+", type=int, default=[375_000, 1_000_000, 8_000_000])
    ap.add_argument("--K", type=int, default=15)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["fused", "spec"], default=None, help="time one side only (kernel traces)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_densify.py needs a GPU")
    dev = torch.device("cuda:0")
    sides = {"fused": densify.densify_and_prune_tensors, "spec": densify_and_prune_spec}
    if args.only:
        sides = {args.only: sides[args.only]}
    for P in args.rows:
        call_args, noise = inputs(P, args.K, dev)
        for _ in range(args.warmup):
            for fn in sides.values():
                fn(*call_args, noise=noise)
        host = {k: [] for k in sides}
        device = {k: [] for k in sides}
        totals = None
        for _ in range(args.reps):
            for k, fn in sides.items():
                h, dv, totals = timed(fn, call_args, noise)
                host[k].append(h)
                device[k].append(dv)
        peak = {k: peak_above_inputs(fn, call_args, noise) for k, fn in sides.items()}
        n_orig, n_clone, S, n_kept = totals
        P_new = n_orig + n_clone + 2 * n_kept
        E = 3 * (14 + 3 * args.K) * 4
        nbytes = E * P + E * P_new + (24 + 8) * P
        bound_us = nbytes / HBM_BYTES_PER_S * 1e6
        row = {"rows": P, "K": args.K, "rows_out": P_new, "totals": list(totals), "reps": args.reps, "bytes": nbytes,
               "bound_us": bound_us}
        for k in sides:
            row[f"{k}_ms"] = stats(host[k])
            row[f"{k}_device_ms"] = stats(device[k])
            row[f"{k}_peak_bytes"] = peak[k]
        if len(sides) == 2:
            row["speedup_median"] = row["spec_ms"]["median"] / row["fused_ms"]["median"]
            row["ranges_overlap"] = row["fused_ms"]["max"] >= row["spec_ms"]["min"]
        if "fused" in sides:
            row["byte_bound_share"] = bound_us / (row["fused_ms"]["median"] * 1e3)
        if "fused" in sides:
            row["fused_model_peak_bytes"] = model_peak(call_args, noise)
        print(json.dumps(row), flush=True)
        del call_args, noise
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
