#!/usr/bin/env python
"""Fused training-loss figures, one JSON line per shape, every contender forward + backward
with exposure (requires grad), alpha mask and depth term on, gradients to the rendered image, the exposure and the
inverse depth:

  fused_ms        (a) hgs.loss.photometric_loss (hgs_photo_fwd + reduction, hgs_photo_bwd + reduction)
  composed_ms     (b) the best composition without it: the reference's torch lines for exposure, clamp, mask, L1, the
                  lambda mix and the depth term (tests/photometric_spec.torch_formula) with hgs.loss.ssim for SSIM
  torch_ms        (c) the same lines with the torch SSIM formula (tests/train_loop.ssim), for information
  ssim_only_ms    hgs.loss.ssim forward + backward alone on the same image pair, for the ratio fused / ssim_only
  All on the same inputs in the same process, after warm-up, hipEvents around --iters calls, the contenders alternated
  over --reps repetitions: the median, the minimum and the maximum of the repetitions are printed.
  non_overlap     the acceptance criterion: (a)'s slowest repetition is faster than (b)'s fastest
  bytes           the traffic floor of (a): the forward reads r, gt (C planes each), the mask and three depth planes and
                  writes three maps of C planes; the backward reads the maps, r, gt, the mask and the depth planes and
                  writes the image gradient and one depth plane -- (11 C + 9) planes of float32
  bound_us        bytes over the measured HBM rate (6.29 TB/s, MI355X_MICROARCH: float4 copy); byte_bound_share =
                  bound_us over the fused median

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (e.g. --reps 2 --only fused).

    python scripts/bench_photometric.py [--shapes 3x1080x1920 3x2160x3840 8x3x1080x1920] [--iters 20] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hgs import loss                 # noqa: E402
import photometric_spec as spec      # noqa: E402
import train_loop                    # noqa: E402

HBM_BYTES_PER_S = 6.29e12
LAMBDA, DEPTH_WEIGHT = 0.2, 0.7


def inputs(shape, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g, device=dev)
    lead = shape[:-3]
    H, W = shape[-2:]
    r = (1.3 * rand(*shape) - 0.15).requires_grad_(True)
    gt = (0.8 * r.detach() + 0.2 * rand(*shape)).clamp(0, 1)
    E = (torch.eye(3, 4, device=dev).expand(*lead, 3, 4) + 0.05 * (rand(*lead, 3, 4) - 0.5)).contiguous().requires_grad_(True)
    mask = (rand(*lead, 1, H, W) > 0.1).float()
    d = (0.2 + 0.3 * rand(*lead, 1, H, W)).requires_grad_(True)
    mono = d.detach() + 0.05 * (rand(*lead, 1, H, W) - 0.5)
    md = (rand(*lead, 1, H, W) > 0.15).float()
    return dict(rendered=r, gt=gt, exposure=E, alpha_mask=mask, invdepth=d, mono_invdepth=mono, depth_mask=md)


def backward(value, t):
    return torch.autograd.grad(value, (t["rendered"], t["exposure"], t["invdepth"]))


def fused(t):
    return backward(loss.photometric_loss(lambda_dssim=LAMBDA, depth_weight=DEPTH_WEIGHT, **t).loss, t)


def composed(t):
    return backward(spec.torch_formula(ssim_fn=loss.ssim, lambda_dssim=LAMBDA, depth_weight=DEPTH_WEIGHT, **t)[0], t)


def all_torch(t):
    return backward(spec.torch_formula(ssim_fn=spec.planes_ssim(train_loop.ssim), lambda_dssim=LAMBDA,
                                       depth_weight=DEPTH_WEIGHT, **t)[0], t)


def ssim_only(t):
    return torch.autograd.grad(loss.ssim(t["rendered"], t["gt"]), t["rendered"])


CONTENDERS = dict(fused=fused, composed=composed, torch=all_torch, ssim_only=ssim_only)


def time_ms(fn, t, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(t)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["3x1080x1920", "3x2160x3840", "8x3x1080x1920"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", nargs="+", choices=list(CONTENDERS), default=list(CONTENDERS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photometric.py needs a GPU")
    dev = torch.device("cuda:0")
    for s in args.shapes:
        shape = tuple(int(v) for v in s.split("x"))
        t = inputs(shape, dev)
        for _ in range(args.warmup):
            for name in args.only:
                CONTENDERS[name](t)
        torch.cuda.synchronize(dev)
        times = {name: [] for name in args.only}
        for _ in range(args.reps):
            for name in args.only:
                times[name].append(time_ms(CONTENDERS[name], t, args.iters))
        C_, H, W = shape[-3:]
        N = shape[0] if len(shape) == 4 else 1
        nbytes = (11 * C_ + 9) * N * H * W * 4
        bound_us = nbytes / HBM_BYTES_PER_S * 1e6
        row = {"shape": list(shape), "iters": args.iters, "reps": args.reps, "bytes": nbytes, "bound_us": bound_us}
        for name in args.only:
            row[name + "_ms"] = stats(times[name])
        if "fused" in times:
            row["byte_bound_share"] = bound_us / (row["fused_ms"]["median"] * 1e3)
        if "fused" in times and "composed" in times:
            row["fused_over_composed"] = row["fused_ms"]["median"] / row["composed_ms"]["median"]
            row["non_overlap"] = row["fused_ms"]["max"] < row["composed_ms"]["min"]
        if "fused" in times and "ssim_only" in times:
            row["fused_over_ssim_only"] = row["fused_ms"]["median"] / row["ssim_only_ms"]["median"]
        print(json.dumps(row), flush=True)
        del t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
