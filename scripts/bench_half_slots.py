#!/usr/bin/env python
"""Half-precision residency slots, one JSON line per measurement.

  (a) fly  the 50 M-node fly-through of bench.py's config5_budgeted_6gb (3840x2160, 6 GB of rows on the GPU, forward 0.08
           units per frame, one 2-unit jump sideways, prefetch of the next view) with rows="half" and slots="float"
           against slots="half", under fit="budget" and under the regulator (fit="regulate"): four configurations,
           alternated --reps times in one run, each run on a fresh BudgetedHierarchy.  Per configuration: the granularity
           rendered per view (in pixels; the request is --tau-px), the budget in rows and its occupancy at the last frame,
           frames/s and the jump frame as minimum / median / maximum over the repetitions.  The comparison is
           slots="float" -- the path of the parent commit -- in the same run; no target is fixed.
  (k1) K1  one LOD cut of that scene (fit="budget" at the first view) rendered --k1-frames times from float slots and from
           half slots, alternated.  Meant to run under the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d DIR -o k1 -- python scripts/bench_half_slots.py --parts k1
               python scripts/rocprof_summary.py DIR/k1_results.db
           and to be read off the rows of preprocess_fwd_kernel<false, true, false> (float slots: 236 bytes per gathered
           row) and preprocess_fwd_lod_half_kernel (half slots: 124).  Without the profiler it prints the whole frame's time.

    python scripts/bench_half_slots.py [--parts a k1] [--nodes 50000000] [--reps 5] [--out FILE]"""
import argparse
import json
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

from hgs import hierarchy, synth                             # noqa: E402
from hgs.residency import BudgetedHierarchy                  # noqa: E402

W, H = 3840, 2160
KEYS = ("means3D", "shs", "opacities", "scales", "rotations")


def stats(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v))


def activated(h):
    """The rasterizer's five arrays of a hierarchy, on its device."""
    return dict(means3D=h.xyz.contiguous(), shs=h.shs.contiguous(), opacities=h.alpha.abs().reshape(-1, 1).contiguous(),
                scales=torch.exp(h.log_scales), rotations=torch.nn.functional.normalize(h.rots))


def render(dgr, kw, bh, m2, sel):
    kw = dict(kw, interpolation_weights=sel.weights, num_node_kids=sel.kids, render_indices=sel.render_indices,
              parent_indices=sel.parent_indices)
    with torch.no_grad():
        return dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw))(
            means3D=bh.means3D, means2D=m2, shs=bh.shs, opacities=bh.opacities, scales=bh.scales, rotations=bh.rotations)


# ---- (a) ----------------------------------------------------------------------------------------------------------
def fly_once(h, attrs, slots, fit, tau, budget_mb, steps, warmup, cams, vps, kws):
    import diff_gaussian_rasterization as dgr
    dev = h.nodes.device
    total = warmup + steps
    bh = BudgetedHierarchy.from_device_arrays(*[attrs[k] for k in KEYS], rows="half", slots=slots, budget_mb=budget_mb)
    m2 = torch.zeros(bh.B, 3, device=dev)
    sels = []

    def frame(k):
        sel = bh.select(h.nodes, h.boxes, tau, vps[k][0], vps[k][1], fit=fit)
        render(dgr, kws[k], bh, m2, sel)
        sels.append((sel.n, sel.tau, sel.misses, sel.attempts))
        if k + 1 < total:
            bh.prefetch(h.nodes, h.boxes, tau, vps[k + 1][0], vps[k + 1][1], fit=fit)
        return sel

    for k in range(warmup):
        frame(k)
    torch.cuda.synchronize()
    sels.clear()
    f0, b0, r0 = bh.stats["rows_fetched"], bh.stats["bytes_fetched"], bh.stats["retries"]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ends[0].record()
    t0 = time.perf_counter()
    for i in range(steps):
        sel = frame(warmup + i)
        ends[i + 1].record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    per_frame = [ends[i].elapsed_time(ends[i + 1]) for i in range(steps)]
    used = int(torch.unique(torch.cat([sel.render_indices, sel.parent_indices])).numel())
    out = dict(budget_rows=bh.B, row_bytes=bh.row_bytes, budget_bytes=bh.budget_bytes, frames_per_s=steps / elapsed,
               jump_frame_ms=per_frame[steps // 2], frame_before_jump_ms=per_frame[steps // 2 - 1],
               p50_ms=sorted(per_frame)[steps // 2], taus=[s[1] for s in sels], mean_cut=sum(s[0] for s in sels) / len(sels),
               cuts_per_frame=sum(s[3] for s in sels) / len(sels), last_frame_occupancy=used / bh.B,
               resident_rows=bh.resident_rows, rows_fetched_per_frame=(bh.stats["rows_fetched"] - f0) / steps,
               bytes_fetched_per_frame=(bh.stats["bytes_fetched"] - b0) / steps, retries=bh.stats["retries"] - r0)
    del bh, m2
    torch.cuda.empty_cache()
    return out


def part_fly(h, tau_px, budget_mb, steps, warmup, reps):
    import parity as pa
    from gaussian_hierarchy import _C as ghC
    dev = h.nodes.device
    cam0 = synth.make_camera(W, H)
    tau = (2 * tau_px + 1) * cam0.tanfovx / (0.5 * W)
    px = lambda t: (t * (0.5 * W) / cam0.tanfovx - 1) / 2
    total, jump = warmup + steps, warmup + steps // 2
    cams = [synth.make_camera(W, H, T=np.array([-(2.0 if k >= jump else 0.0), 0.0, -0.08 * k])) for k in range(total)]
    vps = [(c.camera_center.to(dev), c.camera_center.cpu()) for c in cams]
    kws = [pa.settings_kwargs(c, torch.zeros(3), 3, do_depth=False, device=dev) for c in cams]
    attrs = activated(h)
    configs = [(fit, slots) for fit in ("budget", "regulate") for slots in ("float", "half")]
    runs = {c: [] for c in configs}
    prev_cache = ghC.set_viewpoint_cache(True)
    try:
        for _ in range(reps):                                # alternated: every configuration once per repetition
            for c in configs:
                runs[c].append(fly_once(h, attrs, c[1], c[0], tau, budget_mb, steps, warmup, cams, vps, kws))
    finally:
        ghC.set_viewpoint_cache(prev_cache)
    rows = []
    for (fit, slots), rs in runs.items():
        last = rs[-1]
        taus_px = [round(px(t), 3) for t in last["taus"]]
        rows.append({"part": "fly", "fit": fit, "rows": "half", "slots": slots, "nodes": int(h.nodes.shape[0]),
                     "budget_mb": budget_mb, "budget_rows": last["budget_rows"], "row_bytes": last["row_bytes"],
                     "steps": steps, "warmup": warmup, "reps": reps, "requested_tau_px": tau_px,
                     "rendered_tau_px": taus_px, "rendered_tau_px_mean": sum(taus_px) / len(taus_px),
                     "rendered_tau_px_max": max(taus_px), "mean_cut": last["mean_cut"],
                     "last_frame_occupancy": last["last_frame_occupancy"], "resident_rows": last["resident_rows"],
                     "frames_per_s": stats([r["frames_per_s"] for r in rs]),
                     "jump_frame_ms": stats([r["jump_frame_ms"] for r in rs]),
                     "frame_before_jump_ms": stats([r["frame_before_jump_ms"] for r in rs]),
                     "p50_frame_ms": stats([r["p50_ms"] for r in rs]), "cuts_per_frame": last["cuts_per_frame"],
                     "rows_fetched_per_frame": last["rows_fetched_per_frame"],
                     "bytes_fetched_per_frame": last["bytes_fetched_per_frame"], "retries": last["retries"]})
        print(json.dumps(rows[-1]), flush=True)
    for fit in ("budget", "regulate"):
        f, g = (next(r for r in rows if r["fit"] == fit and r["slots"] == s) for s in ("float", "half"))
        fa, ha = f["frames_per_s"], g["frames_per_s"]
        rows.append({"part": "fly_compare", "fit": fit, "rows_ratio_half_over_float": g["budget_rows"] / f["budget_rows"],
                     "tau_px_mean_float": f["rendered_tau_px_mean"], "tau_px_mean_half": g["rendered_tau_px_mean"],
                     "frames_per_s_median_ratio": ha["median"] / fa["median"],
                     "frames_per_s_ranges_overlap": not (ha["max"] < fa["min"] or fa["max"] < ha["min"])})
        print(json.dumps(rows[-1]), flush=True)
    return rows


# ---- (k1) ---------------------------------------------------------------------------------------------------------
def part_k1(h, tau_px, budget_mb, frames):
    import diff_gaussian_rasterization as dgr
    import parity as pa
    dev = h.nodes.device
    cam = synth.make_camera(W, H)
    tau = (2 * tau_px + 1) * cam.tanfovx / (0.5 * W)
    vp = (cam.camera_center.to(dev), cam.camera_center.cpu())
    kw = pa.settings_kwargs(cam, torch.zeros(3), 3, do_depth=False, device=dev)
    attrs = activated(h)
    # both at the float-slot ROW budget: the same cut, the same rows -- only the bytes per gathered row differ
    rows_float = int(budget_mb * 1e6 // (4 * (3 * 16 + 11)))
    bhs = {s: BudgetedHierarchy.from_device_arrays(*[attrs[k] for k in KEYS], rows="half", slots=s, budget_rows=rows_float)
           for s in ("float", "half")}
    sels = {s: bh.select(h.nodes, h.boxes, tau, vp[0], vp[1], fit="budget") for s, bh in bhs.items()}
    assert sels["float"].n == sels["half"].n and sels["float"].tau == sels["half"].tau
    m2 = torch.zeros(rows_float, 3, device=dev)
    images, ms = {}, {"float": [], "half": []}
    for i in range(frames + 2):
        for s in ("float", "half"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            images[s] = render(dgr, kw, bhs[s], m2, sels[s])[0]
            e1.record()
            e1.synchronize()
            if i >= 2:
                ms[s].append(e0.elapsed_time(e1))
    w = sels["float"].weights[:sels["float"].n]
    row = {"part": "k1", "nodes": int(h.nodes.shape[0]), "budget_rows": rows_float, "cut_entries": sels["float"].n,
           "share_weight_1": float((w == 1.0).float().mean()), "frames": frames, "frame_ms_float_slots": stats(ms["float"]),
           "frame_ms_half_slots": stats(ms["half"]), "images_equal": bool(torch.equal(images["float"], images["half"])),
           "note": "whole frames by hipEvents; K1 alone comes from the rocprofv3 --kernel-trace --stats run of this part"}
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["a"], choices=["a", "k1"])
    ap.add_argument("--nodes", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tau-px", type=float, default=3.0)
    ap.add_argument("--budget-mb", type=float, default=6000.0)
    ap.add_argument("--fly-steps", type=int, default=32)
    ap.add_argument("--fly-warmup", type=int, default=8)
    ap.add_argument("--k1-frames", type=int, default=10)
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (the k1 part after part a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_half_slots_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_half_slots.py needs a GPU")
    dev = torch.device("cuda:0")
    h = hierarchy.build_hierarchy_on_device((args.nodes + 1) // 2, synth.make_camera(W, H), dev, seed=0)
    out = []
    if "k1" in args.parts:
        out += part_k1(h, args.tau_px, args.budget_mb, args.k1_frames)
    if "a" in args.parts:
        out += part_fly(h, args.tau_px, args.budget_mb, args.fly_steps, args.fly_warmup, args.reps)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(json.dumps(r) for r in out) + "\n")


if __name__ == "__main__":
    main()
