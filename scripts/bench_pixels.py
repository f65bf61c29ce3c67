#!/usr/bin/env python
"""Per-pixel readout figures, one JSON line per frame:

  pixels_all_ms     the readout call alone (hgs_raster_pixels, one kernel) with all eight planes, on the workspaces of
                    a forward that is NOT in the timed window
  pixels_front_ms   the same call with the ``front`` plane only: what the seven other plane stores cost
  contrib_ms        hgs_raster_contrib on the same forward: the same walk with per-instance records and a per-row sum
  forward_ms        the no-grad forward alone (a fresh one per repetition; the kept forward is not touched)

Nothing in the library computed these planes before the call, so there is no older route to time against.

Frames: ``metric`` (synth.make_scene, 1 M Gaussians, 1920 x 1080) and ``trained`` (synth.make_scene_trained_scale, 375 k
Gaussians, 10 M instances).  Device events around the calls, warm-up first, the sides alternated over --reps repetitions:
median, minimum, maximum.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--reps 3).
Before timing, the planes are checked against the forward's own words (alpha bits = 1 - final_T, count = 0 where
n_contrib = 0) and against the contribution call (equal pixel counts, equal largest weight).

    python scripts/bench_pixels.py [--frames metric trained] [--reps 15] [--only pixels_all|pixels_front|contrib|forward] [--out file.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))

import diff_gaussian_rasterization as dgr          # noqa: E402
from diff_gaussian_rasterization import _C         # noqa: E402
from hgs import synth                              # noqa: E402

W, H = 1920, 1080
FRAMES = {"metric": lambda cam: synth.make_scene(1_000_000, cam, seed=0),
          "trained": lambda cam: synth.make_scene_trained_scale(375_000, cam, seed=0)}
SIDES = ("pixels_all", "pixels_front", "contrib", "forward")


def settings(cam, dev):
    e_i, e_f = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, device=dev)
    return dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=dev),
        scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
        sh_degree=3, campos=cam.camera_center.to(dev), prefiltered=False, debug=False, render_indices=e_i,
        parent_indices=e_i, interpolation_weights=e_f, num_node_kids=e_i, do_depth=False)


def forward(rs, s, colors):
    """The no-grad forward with colors_precomp -> its call (the readout does not depend on the colours)."""
    with torch.no_grad():
        return _C.rasterize_gaussians(rs.bg, s.means3D, colors, s.opacities, s.scales, s.rotations, 1.0, None, rs.viewmatrix,
                                      rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, None, 3, rs.campos, False, False,
                                      rs.render_indices, rs.parent_indices, rs.interpolation_weights, rs.num_node_kids,
                                      False)[-1]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", nargs="+", default=list(FRAMES), choices=list(FRAMES))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=list(SIDES), default=None, help="time one side only (kernel traces)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pixels.py needs a GPU")
    dev = torch.device("cuda:0")
    cam = synth.make_camera(W, H)
    for name in args.frames:
        s = FRAMES[name](cam).to(dev)
        P = s.P
        rs = settings(cam, dev)
        colors = torch.rand(P, 3, device=dev)
        wmax = torch.zeros(P, device=dev)
        wsum = torch.zeros(P, dtype=torch.float64, device=dev)
        count = torch.zeros(P, dtype=torch.int64, device=dev)
        kept = forward(rs, s, colors)             # the forward whose workspaces the timed calls read
        sides = {"pixels_all": lambda: _C.raster_pixels(kept),
                 "pixels_front": lambda: _C.raster_pixels(kept, want=("front",)),
                 "contrib": lambda: _C.raster_contributions(kept, wmax, wsum, count),
                 "forward": lambda: forward(rs, s, colors)}
        # the same decisions first: the planes against K6's own words and against the contribution call
        planes = sides["pixels_all"]()
        sides["contrib"]()
        v = _C.raster_views(kept)
        torch.cuda.synchronize()
        checks = {
            "alpha_bits_equal_one_minus_final_T": bool(torch.equal(planes["alpha"].view(torch.int32),
                                                                   (1.0 - v["final_T"]).view(torch.int32))),
            "count_zero_where_n_contrib_zero": bool(torch.equal(planes["count"] == 0, v["n_contrib"] == 0)),
            "count_sum_equals_contrib": int(planes["count"].sum()) == int(count.sum()),
            "largest_wmax_bits_equal_contrib": bool(torch.equal(planes["wmax"].max().view(torch.int32),
                                                                wmax.max().view(torch.int32)))}
        covered, halved = int((planes["count"] > 0).sum()), int((planes["median"] != -1).sum())
        mean_rows = float(planes["count"].float().mean())
        wmax.zero_(); wsum.zero_(); count.zero_()
        del planes, v
        if args.only:
            sides = {args.only: sides[args.only]}
        for _ in range(args.warmup):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        for _ in range(args.reps):
            for k, fn in sides.items():
                ms[k].append(timed(fn)[0])
        row = {"frame": name, "gaussians": P, "width": W, "height": H, "instances": int(kept.L), "reps": args.reps,
               "checks": checks, "pixels_with_a_row": covered, "pixels_with_a_median": halved,
               "mean_rows_per_pixel": mean_rows, "plane_bytes_all": 8 * 4 * W * H}
        for k in sides:
            row[f"{k}_ms"] = stats(ms[k])
        for k in ("pixels_all", "pixels_front"):
            if k in sides and "contrib" in sides:
                row[f"{k}_over_contrib_median"] = row[f"{k}_ms"]["median"] / row["contrib_ms"]["median"]
                row[f"{k}_contrib_ranges_overlap"] = (row[f"{k}_ms"]["min"] <= row["contrib_ms"]["max"] and
                                                      row["contrib_ms"]["min"] <= row[f"{k}_ms"]["max"])
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fo:
                fo.write(line + "\n")
        if not all(checks.values()):
            raise SystemExit(f"bench_pixels.py: the planes disagree with the forward on the {name} frame: {checks}")
        del s, kept, colors, wmax, wsum, count
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
