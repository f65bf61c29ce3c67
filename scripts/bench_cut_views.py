#!/usr/bin/env python
"""Cut for several views: hgs.frustum.cut_views against V sequential
hgs.frustum.cut_view(nested=True) calls, one JSON line per measurement.

For every hierarchy size and every V: the V views are cameras at one place turned by 7 degrees from view to view, each
with a granularity of its own (log-uniform between 2 and 12 px, fixed seed), as the views of one training step or of a
viewer that also cuts for predicted cameras are.  Two places: "inside" (at (0, 0, 10), first view turned by 120
degrees: most of the scene is beside or behind every view) and "nocull" (the canonical camera in front of the scene with
planes that contain everything: nothing is culled, every view keeps its whole cut).

Before timing, the outputs of the two ways are compared (all five arrays of every view, bit for bit).  Then the two ways
ALTERNATE in one process after a warm-up; a host clock runs around each (each ends in its own host wait, and the
device is idle when the clock starts); --reps repetitions (>= 15): minimum, median, maximum.  Both ways write into
preallocated outputs.

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--sizes 50000000 --views 8 --reps 2
--out ''); this script only states the mark pass's bytes per node, from the shapes.

    python scripts/bench_cut_views.py [--sizes 1000000 10000000 50000000] [--views 2 4 8 16] [--reps 15] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))

from hgs import frustum, hierarchy, synth            # noqa: E402

W, H = 3840, 2160
ALL_INSIDE = torch.tensor([[0.0, 0.0, 1.0, 1e30]] * 5)
# the mark pass per node: 28 B record + 32 B box + 32 B parent's box + 16 B ball read once, 4 B per view written (the
# parent's ball, gathered by the nodes whose own ball is outside a plane, and the workgroup sums are not counted)
READ_BYTES = 28 + 32 + 32 + 16


def stats(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v))


def yaw_camera(center, yaw_deg):
    a = math.radians(yaw_deg)
    R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    return synth.make_camera(W, H, R=R, T=-R.T @ np.asarray(center, dtype=np.float64))


def views_of(place, V):
    """-> (taus [V], viewpoints [V,3], planes [V,5,4], radius scales [V]) on the host."""
    px = np.exp(np.random.default_rng(15).uniform(math.log(2.0), math.log(12.0), size=16))[:V]
    taus, vps, pls, rss = [], [], [], []
    for k in range(V):
        cam = yaw_camera((0.0, 0.0, 10.0), 120.0 + 7.0 * k) if place == "inside" else yaw_camera((0.0, 0.0, 0.0), 0.0 + 7.0 * k)
        planes, rs = frustum.frustum_planes(cam.world_view_transform, cam.tanfovx, cam.tanfovy, W, H)
        taus.append((2 * float(px[k]) + 1) * cam.tanfovx / (0.5 * W))
        vps.append(cam.camera_center.cpu())
        pls.append(ALL_INSIDE if place == "nocull" else planes)
        rss.append(float(rs))
    return taus, torch.stack(vps), torch.stack(pls), rss


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def measure(h, bounds, place, V, reps, warmup):
    dev = h.nodes.device
    G = int(h.nodes.shape[0])
    taus, vps, pls, rss = views_of(place, V)
    first = frustum.cut_views(h.nodes, h.boxes, bounds, taus, vps, pls, rss)
    needed = first[-1].render_indices.storage_offset() + first[-1].n
    packed = frustum.CutBuffers(max(needed, 1), dev)
    one = frustum.CutBuffers(max(max(c.n for c in first), 1), dev)
    del first

    def fused():
        return frustum.cut_views(h.nodes, h.boxes, bounds, taus, vps, pls, rss, out=packed)

    def sequential(keep=None):
        res = []
        for k in range(V):
            cv = frustum.cut_view(h.nodes, h.boxes, bounds, taus[k], vps[k], pls[k], rss[k], out=one, nested=True)
            res.append((cv.n, cv.n_unculled))
            if keep is not None:
                keep(k, cv)
        return res

    # the outputs are equal: every view, all five arrays, bit for bit
    cuts = fused()

    def same(k, cv):
        c = cuts[k]
        assert (c.n, c.n_unculled) == (cv.n, cv.n_unculled), (k, c.n, cv.n)
        for a, b in ((c.render_indices, cv.render_indices), (c.parent_indices, cv.parent_indices),
                     (c.node_indices, cv.node_indices), (c.kids, cv.kids), (c.weights.view(torch.int32), cv.weights.view(torch.int32))):
            assert torch.equal(a, b), k

    counts = sequential(keep=same)
    for _ in range(warmup):
        fused(); sequential()
    t = {"cut_views": [], "sequential": []}
    for _ in range(reps):
        t["cut_views"].append(clocked(fused)[0])
        t["sequential"].append(clocked(sequential)[0])
    nblk = (G + 255) // 256
    return {"part": "cut_views", "nodes": G, "place": place, "views": V, "reps": reps, "outputs_equal": True,
            "entries_kept": [c[0] for c in counts], "entries_unculled": [c[1] for c in counts],
            "cut_views_ms": stats(t["cut_views"]), "sequential_ms": stats(t["sequential"]),
            "ratio_median": statistics.median(t["cut_views"]) / statistics.median(t["sequential"]),
            "ranges_overlap": not (max(t["cut_views"]) < min(t["sequential"]) or max(t["sequential"]) < min(t["cut_views"])),
            "mark_bytes_per_node": READ_BYTES + 4 * V, "mark_bytes": G * (READ_BYTES + 4 * V) + nblk * 8 * V,
            "sequential_mark_bytes_per_node": V * (READ_BYTES + 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[1_000_000, 10_000_000, 50_000_000], help="nodes")
    ap.add_argument("--views", nargs="+", type=int, default=[2, 4, 8, 16])
    ap.add_argument("--places", nargs="+", default=["inside", "nocull"])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f15_cut_views_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cut_views.py needs a GPU")
    dev = torch.device("cuda:0")
    cam = synth.make_camera(W, H)
    lines = []
    for nodes in sorted(args.sizes):
        h = hierarchy.build_hierarchy_on_device((nodes + 1) // 2, cam, dev, seed=0)
        bounds = frustum.cull_bounds(h.nodes, h.xyz.contiguous(), torch.exp(h.log_scales).contiguous())
        for place in args.places:
            for V in args.views:
                row = measure(h, bounds, place, V, args.reps, args.warmup)
                print(json.dumps(row), flush=True)
                lines.append(json.dumps(row))
                torch.cuda.empty_cache()
        del h, bounds
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
