#!/usr/bin/env python
"""Fused SSIM loss figures, one JSON line per shape:

  fused_ms    hgs.loss.ssim forward + backward (hgs_ssim_fwd + reduction + hgs_ssim_bwd)
  torch_ms    the reference's formula (tests/train_loop.ssim: five grouped 11x11 conv2d calls) forward + backward
              through autograd; a batch is passed as (N*C, H, W), the same per-channel planes and the same mean
  Both on the same inputs in the same process, after warm-up, hipEvents around --iters calls, the two alternated over
  --reps repetitions: the median, the minimum and the maximum of the repetitions are printed.
  bytes       the traffic floor: the forward reads two images and writes three per-pixel maps, the backward reads the
              maps and the two images and writes one gradient -- 11 images of float32
  bound_us    bytes over the measured HBM rate (6.29 TB/s, MI355X_MICROARCH: float4 copy); byte_bound_share = bound_us
              over the fused median

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (e.g. --reps 2).

    python scripts/bench_ssim.py [--shapes 3x1080x1920 3x2160x3840 8x3x1080x1920] [--iters 20] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hgs import loss   # noqa: E402
import train_loop      # noqa: E402

HBM_BYTES_PER_S = 6.29e12


def inputs(shape, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    x1 = torch.rand(shape, generator=g, device=dev)
    x2 = (0.8 * x1 + 0.2 * torch.rand(shape, generator=g, device=dev)).clamp(0, 1)
    return x1.requires_grad_(True), x2


def fused(x1, x2):
    v = loss.ssim(x1, x2)
    return torch.autograd.grad(v, x1)[0]


def torch_formula(x1, x2):
    a = x1 if x1.dim() == 3 else x1.reshape(-1, *x1.shape[-2:])
    b = x2 if x2.dim() == 3 else x2.reshape(-1, *x2.shape[-2:])
    v = train_loop.ssim(a, b)
    return torch.autograd.grad(v, x1)[0]


def time_ms(fn, x1, x2, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(x1, x2)
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim.py needs a GPU")
    dev = torch.device("cuda:0")
    for s in args.shapes:
        shape = tuple(int(v) for v in s.split("x"))
        x1, x2 = inputs(shape, dev)
        for _ in range(args.warmup):
            fused(x1, x2)
            torch_formula(x1, x2)
        torch.cuda.synchronize(dev)
        tf, tt = [], []
        for _ in range(args.reps):
            tf.append(time_ms(fused, x1, x2, args.iters))
            tt.append(time_ms(torch_formula, x1, x2, args.iters))
        numel = x1.numel()
        nbytes = 11 * numel * 4
        bound_us = nbytes / HBM_BYTES_PER_S * 1e6
        f, t = stats(tf), stats(tt)
        print(json.dumps({"shape": list(shape), "fused_ms": f, "torch_ms": t,
                          "speedup_median": t["median"] / f["median"], "bytes": nbytes, "bound_us": bound_us,
                          "byte_bound_share": bound_us / (f["median"] * 1e3), "iters": args.iters, "reps": args.reps}),
              flush=True)
        del x1, x2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
