#!/usr/bin/env python
"""Similarity transform figures, one JSON line per (size, mode):

  hierarchies     hgs.hierarchy.build_hierarchy_on_device, --sizes nodes each (16 SH coefficients: 236 bytes per row, 28 of
                  node record and 32 of box per node)
  transform       a general rotation, s = 1.7, t = (3, -2, 9)
  hip             hgs.hierarchy.transform_hierarchy_gpu (hgs_hier_transform), out of place and in place
  torch           this project's torch statement of the same rule on the same GPU (torch_transform below), out of place:
                  float64 as the rule asks, a matrix product for the means, an einsum per SH band, the quaternion product
                  written out, the box formula with the positive and negative parts of R; nodes and alpha cloned
  each            --reps alternated repetitions after one warm-up call of each, device events around the call: median,
                  min and max; the peak device memory of one call above what was allocated before it.  The outputs are
                  compared before anything is timed: the torch statement sums in another order, so not bit for bit but
                  within 2 float32 ulp of each row's largest entry (nodes and alpha bit for bit).
  floor_ms        the bytes the call cannot avoid, 2 (236 G + 32 N), at 8 TB/s; share = floor_ms / the HIP median

    python scripts/bench_transform.py [--sizes 1000000 10000000 50000000] [--reps 15] [--out profiles/f18_transform_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))

from hgs import hierarchy, synth   # noqa: E402

ARRAYS = ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes")
PEAK_BYTES_PER_MS = 8.0e9           # 8 TB/s


def torch_transform(h, sim, dev):
    """The rule in torch ops, float64, rounded once -> Hierarchy."""
    f64 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float64), device=dev)
    R, t, q = f64(sim.R), f64(sim.t), f64(sim.q_R)
    xyz = ((h.xyz.double() @ R.T) * sim.s + t).float()
    shs = h.shs.clone()
    for l, D in ((1, sim.D1), (2, sim.D2), (3, sim.D3)):
        o, n = l * l, 2 * l + 1
        if shs.shape[1] >= o + n:
            shs[:, o:o + n] = torch.einsum("mk,gkc->gmc", f64(D), h.shs[:, o:o + n].double()).float()
    ls = (h.log_scales.double() + sim.log_s).float()
    b = h.rots.double()
    b0, b1, b2, b3 = b.unbind(1)
    rots = torch.stack([q[0] * b0 - q[1] * b1 - q[2] * b2 - q[3] * b3, q[0] * b1 + q[1] * b0 + q[2] * b3 - q[3] * b2,
                        q[0] * b2 - q[1] * b3 + q[2] * b0 + q[3] * b1, q[0] * b3 + q[1] * b2 - q[2] * b1 + q[3] * b0], 1).float()
    lo, hi = h.boxes[:, 0, :3].double(), h.boxes[:, 1, :3].double()
    Rp, Rn = R.clamp(min=0).T, R.clamp(max=0).T
    boxes = h.boxes.clone()
    boxes[:, 0, :3] = ((lo @ Rp + hi @ Rn) * sim.s + t).float()
    boxes[:, 1, :3] = ((hi @ Rp + lo @ Rn) * sim.s + t).float()
    boxes[:, 0, 3] = (boxes[:, 1, :3] - boxes[:, 0, :3]).max(1).values
    return hierarchy.Hierarchy(xyz, shs, h.alpha.clone(), ls, rots, h.nodes.clone(), boxes)


def timed(fn, dev):
    """-> (result, ms from events, peak bytes above the allocation before the call)."""
    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1), torch.cuda.max_memory_allocated(dev) - base


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def close(a, b):
    """Within 2 float32 ulp of each row's largest entry."""
    a, b = a.reshape(a.shape[0], -1).double(), b.reshape(b.shape[0], -1).double()
    mag = torch.maximum(a.abs(), b.abs()).max(1, keepdim=True).values
    return bool(((a - b).abs() <= 2 * 2.0 ** -23 * mag).all())


def figures(h, sim, reps, dev):
    G, N, M = int(h.xyz.shape[0]), h.num_nodes, int(h.shs.shape[1])
    hip = lambda: hierarchy.transform_hierarchy_gpu(h, sim)
    ref = lambda: torch_transform(h, sim, dev)
    a, b = hip(), ref()
    for k in ("xyz", "shs", "log_scales", "rots"):
        assert close(getattr(a, k), getattr(b, k)), k
    assert close(a.boxes[:, :, :3].reshape(N, 6), b.boxes[:, :, :3].reshape(N, 6))
    assert torch.equal(a.nodes, b.nodes) and torch.equal(a.alpha.view(torch.int32), b.alpha.view(torch.int32))
    del a, b
    work = hierarchy.Hierarchy(*(getattr(h, k).clone() for k in ARRAYS))      # the in-place runs move this copy about
    inplace = lambda: hierarchy.transform_hierarchy_gpu(work, sim, inplace=True)
    inplace()
    ms = {"hip": [], "hip_inplace": [], "torch": []}
    peak = {k: 0 for k in ms}
    for _ in range(reps):                       # alternated
        for name, fn in (("hip", hip), ("hip_inplace", inplace), ("torch", ref)):
            out, t, p = timed(fn, dev)
            del out
            ms[name].append(t)
            peak[name] = max(peak[name], p)
    floor_ms = 2 * ((12 * M + 44) * G + 32 * N) / PEAK_BYTES_PER_MS
    med = {k: statistics.median(v) for k, v in ms.items()}
    return dict(nodes=N, rows=G, M=M, hip_ms=summary(ms["hip"]), hip_inplace_ms=summary(ms["hip_inplace"]),
                torch_ms=summary(ms["torch"]), ranges_apart=max(ms["hip"]) < min(ms["torch"]),
                speedup=round(med["torch"] / med["hip"], 2), floor_ms=round(floor_ms, 3),
                share=round(floor_ms / med["hip"], 3), share_inplace=round(floor_ms / med["hip_inplace"], 3),
                hip_peak_mb=round(peak["hip"] / 2**20, 1), hip_inplace_peak_mb=round(peak["hip_inplace"] / 2**20, 1),
                torch_peak_mb=round(peak["torch"] / 2**20, 1), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 10_000_000, 50_000_000])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cam = synth.make_camera(1920, 1080)
    q = np.array([0.83, 0.21, -0.43, 0.29])
    sim = hierarchy.similarity(quat=q, scale=1.7, translate=(3.0, -2.0, 9.0))
    for n in args.sizes:
        h = hierarchy.build_hierarchy_on_device((n + 1) // 2, cam, dev, seed=1)
        res = figures(h, sim, args.reps, dev)
        res["device"] = torch.cuda.get_device_name(dev)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del h
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
