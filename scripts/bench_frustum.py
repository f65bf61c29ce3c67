#!/usr/bin/env python
"""Frustum-culled hierarchy cut figures, one JSON line per measurement.

  (a) cut    hgs.frustum.cut_view (cut + cull + weights + sibling counts, one call) against expand_to_size +
             get_interpolation_weights (hgs_expand_to_size_nested + hgs_interp_weights) on the same hierarchy, view and
             granularity, in the same run: hipEvents around the Python calls (both contain one host wait for the count),
             alternated over --reps repetitions after a warm-up: minimum, median, maximum.  Two views: "outside" (the
             canonical camera in front of the scene: little to cull) and "inside" (at (0, 0, 10), turned by 120 degrees).
  (b) fly    the 50 M-node fly-through of bench.py's config5_budgeted_6gb (3840x2160, 6 GB of rows on the GPU, forward
             0.08 units per frame, one 2-unit jump sideways, prefetch of the next view) with and without ``frustum=``:
             frames/s, frame times, the granularity the regulator settled at, budget occupancy, rows fetched.
  (c) bounds hgs.frustum.cull_bounds at the largest size.

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--parts a --sizes 50000000 --reps 2).

    python scripts/bench_frustum.py [--sizes 1000000 10000000 50000000] [--parts a b c] [--reps 7] [--out FILE]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hgs import frustum, hierarchy, synth            # noqa: E402

W, H = 3840, 2160


def stats(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def yaw_camera(center, yaw_deg):
    a = math.radians(yaw_deg)
    R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    return synth.make_camera(W, H, R=R, T=-R.T @ np.asarray(center, dtype=np.float64))


def planes_of(cam):
    return frustum.frustum_planes(cam.world_view_transform, cam.tanfovx, cam.tanfovy, W, H)


def part_cut(h, bounds, tau, reps, warmup):
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    dev = h.nodes.device
    G = int(h.nodes.shape[0])
    bufs = frustum.CutBuffers(G, dev)
    zero3 = torch.zeros(3)
    rows = []
    for view, cam in (("outside", synth.make_camera(W, H)), ("inside", yaw_camera((0.0, 0.0, 10.0), 120.0))):
        vp = cam.camera_center.cpu()
        planes, rs = planes_of(cam)

        def plain():
            n = expand_to_size(h.nodes, h.boxes, tau, vp, zero3, bufs.ri, bufs.pi, bufs.ni)
            get_interpolation_weights(bufs.ni[:n], tau, h.nodes, h.boxes, vp, zero3, bufs.w, bufs.ns)
            return n

        def culled():
            return frustum.cut_view(h.nodes, h.boxes, bounds, tau, vp, planes, rs, out=bufs)

        for _ in range(warmup):
            plain(); culled()
        t = {"plain": [], "cut_view": []}
        for _ in range(reps):
            ms, n_plain = timed(plain)
            t["plain"].append(ms)
            ms, cv = timed(culled)
            t["cut_view"].append(ms)
        assert cv.n_unculled == n_plain
        rows.append({"part": "cut", "nodes": G, "view": view, "tau": tau, "reps": reps, "entries_unculled": n_plain,
                     "entries_kept": cv.n, "plain_ms": stats(t["plain"]), "cut_view_ms": stats(t["cut_view"]),
                     "ratio_median": statistics.median(t["cut_view"]) / statistics.median(t["plain"]),
                     "ranges_overlap": not (max(t["cut_view"]) < min(t["plain"]) or max(t["plain"]) < min(t["cut_view"]))})
    return rows


def part_bounds(h, reps):
    means, scales = h.xyz.contiguous(), torch.exp(h.log_scales).contiguous()
    frustum.cull_bounds(h.nodes, means, scales)
    t = [timed(lambda: frustum.cull_bounds(h.nodes, means, scales))[0] for _ in range(reps)]
    G = int(h.nodes.shape[0])
    return [{"part": "bounds", "nodes": G, "reps": reps, "ms": stats(t), "bytes": G * (28 + 24 + 16)}]


def part_fly(h, tau_px, budget_mb, steps, warmup):
    import diff_gaussian_rasterization as dgr
    import parity as pa
    from gaussian_hierarchy import _C as ghC
    from hgs.residency import BudgetedHierarchy
    dev = h.nodes.device
    G = int(h.nodes.shape[0])
    cam0 = synth.make_camera(W, H)
    tau = (2 * tau_px + 1) * cam0.tanfovx / (0.5 * W)
    total, jump = warmup + steps, warmup + steps // 2
    cams = [synth.make_camera(W, H, T=np.array([-(2.0 if k >= jump else 0.0), 0.0, -0.08 * k])) for k in range(total)]
    vps = [(c.camera_center.to(dev), c.camera_center.cpu()) for c in cams]
    frs = [planes_of(c) for c in cams]
    kws = [pa.settings_kwargs(c, torch.zeros(3), 3, do_depth=False, device=dev) for c in cams]
    px = lambda t: (t * (0.5 * W) / cam0.tanfovx - 1) / 2
    rows = []
    prev_cache = ghC.set_viewpoint_cache(True)
    try:
        for mode in ("plain", "frustum"):
            bh = BudgetedHierarchy(h.xyz.cpu(), h.shs.cpu(), h.alpha.cpu(), torch.exp(h.log_scales).cpu(), h.rots.cpu(), dev,
                                   budget_mb=budget_mb)
            m2 = torch.zeros(bh.B, 3, device=dev)
            fkw = (lambda k: dict(frustum=frs[k])) if mode == "frustum" else (lambda k: {})
            sels, occ = [], []

            def frame(k):
                sel = bh.select(h.nodes, h.boxes, tau, vps[k][0], vps[k][1], **fkw(k))
                kw = dict(kws[k], interpolation_weights=sel.weights, num_node_kids=sel.kids,
                          render_indices=sel.render_indices, parent_indices=sel.parent_indices)
                with torch.no_grad():
                    color = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw))(
                        means3D=bh.means3D, means2D=m2, shs=bh.shs, opacities=bh.opacities, scales=bh.scales,
                        rotations=bh.rotations)[0]
                sels.append((sel.n, sel.tau, sel.misses, sel.attempts))
                if k + 1 < total:
                    bh.prefetch(h.nodes, h.boxes, tau, vps[k + 1][0], vps[k + 1][1], **fkw(k + 1))
                return color, sel

            for k in range(warmup):
                frame(k)
            torch.cuda.synchronize()
            sels.clear()
            f0, c0 = bh.stats["rows_fetched"], bh.stats["entries_culled"]
            ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            ends[0].record()
            t0 = time.perf_counter()
            for i in range(steps):
                _, sel = frame(warmup + i)
                ends[i + 1].record()
            torch.cuda.synchronize()
            elapsed = time.perf_counter() - t0
            ms = sorted(ends[i].elapsed_time(ends[i + 1]) for i in range(steps))
            used = int(torch.unique(torch.cat([sel.render_indices, sel.parent_indices])).numel())
            rows.append({"part": "fly", "mode": mode, "nodes": G, "budget_mb": budget_mb, "budget_rows": bh.B, "steps": steps,
                         "warmup": warmup, "requested_tau_px": tau_px, "frames_per_s": steps / elapsed,
                         "frame_ms": {"p50": ms[len(ms) // 2], "p99": ms[min(len(ms) - 1, int(0.99 * len(ms)))], "max": ms[-1]},
                         "rendered_tau_px": {"mean": sum(px(s[1]) for s in sels) / len(sels),
                                             "min": px(min(s[1] for s in sels)), "max": px(max(s[1] for s in sels))},
                         "mean_cut": sum(s[0] for s in sels) / len(sels),
                         "cuts_per_frame": sum(s[3] for s in sels) / len(sels),
                         "last_frame_occupancy": used / bh.B,
                         "rows_fetched_per_frame": (bh.stats["rows_fetched"] - f0) / steps,
                         "rows_select_still_fetched_max": max(s[2] for s in sels),
                         "entries_culled_per_frame": (bh.stats["entries_culled"] - c0) / steps,
                         "retries": bh.stats["retries"]})
            print(json.dumps(rows[-1]), flush=True)
            del bh, m2
            torch.cuda.empty_cache()
    finally:
        ghC.set_viewpoint_cache(prev_cache)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[1_000_000, 10_000_000, 50_000_000], help="nodes")
    ap.add_argument("--parts", nargs="+", default=["a", "b", "c"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tau-px", type=float, default=3.0)
    ap.add_argument("--budget-mb", type=float, default=6000.0)
    ap.add_argument("--fly-steps", type=int, default=32)
    ap.add_argument("--fly-warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f11_frustum_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frustum.py needs a GPU")
    dev = torch.device("cuda:0")
    cam = synth.make_camera(W, H)
    tau = (2 * args.tau_px + 1) * cam.tanfovx / (0.5 * W)
    lines = []
    for nodes in sorted(args.sizes):
        h = hierarchy.build_hierarchy_on_device((nodes + 1) // 2, cam, dev, seed=0)
        last = nodes == max(args.sizes)
        out = []
        if "a" in args.parts or ("c" in args.parts and last):
            bounds = frustum.cull_bounds(h.nodes, h.xyz.contiguous(), torch.exp(h.log_scales).contiguous())
        if "a" in args.parts:
            out += part_cut(h, bounds, tau, args.reps, args.warmup)
        if "c" in args.parts and last:
            out += part_bounds(h, args.reps)
        for r in out:
            print(json.dumps(r), flush=True)
        if "b" in args.parts and last:
            bounds = None
            out += part_fly(h, args.tau_px, args.budget_mb, args.fly_steps, args.fly_warmup)
        lines += [json.dumps(r) for r in out]
        del h
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
