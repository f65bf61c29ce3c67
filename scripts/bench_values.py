#!/usr/bin/env python
"""Value painting figures, one JSON line per frame:

  values_c1_ms      the painting call alone (hgs_raster_values, one kernel) with one channel, on the workspaces of a
                    forward that is NOT in the timed window
  values_c3_ms      the same call with three channels;  values_c4_ms: with four;  values_c4_wsum_ms: four and the weight sum
  pixels_all_ms     hgs_raster_pixels with all eight planes on the same forward: the same walk with id planes
  forward_ms        the no-grad forward alone with colors_precomp (a fresh one per repetition; the kept forward is not
                    touched): the only way to get such an image before this call -- three channels, no slot map

Frames: ``metric`` (synth.make_scene, 1 M Gaussians, 1920 x 1080) and ``trained`` (synth.make_scene_trained_scale, 375 k
Gaussians, 10 M instances).  Device events around the calls, warm-up first, the sides alternated over --reps repetitions:
median, minimum, maximum.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--reps 3).
Before timing, the call is checked against the forward itself: the colour words of K1's records, painted, must give the
bits of the forward's image, a channel of ones the bits of the weight sum, and the weight sum must be zero exactly
where the readout counts no row.

    python scripts/bench_values.py [--frames metric trained] [--reps 15] [--only values_c1|...|forward] [--out file.jsonl]"""
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
SIDES = ("values_c1", "values_c3", "values_c4", "values_c4_wsum", "pixels_all", "forward")


def settings(cam, dev):
    e_i, e_f = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, device=dev)
    return dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=dev),
        scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
        sh_degree=3, campos=cam.camera_center.to(dev), prefiltered=False, debug=False, render_indices=e_i,
        parent_indices=e_i, interpolation_weights=e_f, num_node_kids=e_i, do_depth=False)


def forward(rs, s, colors):
    """The no-grad forward with colors_precomp -> (its image, its call)."""
    with torch.no_grad():
        res = _C.rasterize_gaussians(rs.bg, s.means3D, colors, s.opacities, s.scales, s.rotations, 1.0, None, rs.viewmatrix,
                                     rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, None, 3, rs.campos, False, False,
                                     rs.render_indices, rs.parent_indices, rs.interpolation_weights, rs.num_node_kids,
                                     False)
    return res[1], res[-1]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def bits(t):
    return t.contiguous().view(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", nargs="+", default=list(FRAMES), choices=list(FRAMES))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=list(SIDES), default=None, help="time one side only (kernel traces)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_values.py needs a GPU")
    dev = torch.device("cuda:0")
    cam = synth.make_camera(W, H)
    for name in args.frames:
        s = FRAMES[name](cam).to(dev)
        P = s.P
        rs = settings(cam, dev)
        colors = torch.rand(P, 3, device=dev)
        table = torch.randn(P, 4, device=dev)
        image, kept = forward(rs, s, colors)      # the forward whose workspaces the timed calls read
        image = image.clone()
        sides = {"values_c1": lambda: _C.raster_values(kept, table[:, :1]),
                 "values_c3": lambda: _C.raster_values(kept, table[:, :3]),
                 "values_c4": lambda: _C.raster_values(kept, table),
                 "values_c4_wsum": lambda: _C.raster_values(kept, table, want_wsum=True),
                 "pixels_all": lambda: _C.raster_pixels(kept),
                 "forward": lambda: forward(rs, s, colors)}
        # the same blend first: the forward's own colour words painted, a channel of ones, the readout's count
        words = _C.raster_views(kept)["records"][:, 6:9]
        painted = _C.raster_values(kept, words)
        ones, wsum = _C.raster_values(kept, torch.ones(P, device=dev), want_wsum=True)
        count = _C.raster_pixels(kept, want=("count",))["count"]
        torch.cuda.synchronize()
        checks = {"record_colours_paint_the_forwards_image_bits": bool(torch.equal(bits(painted), bits(image))),
                  "ones_channel_bits_equal_wsum": bool(torch.equal(bits(ones[0]), bits(wsum))),
                  "wsum_zero_exactly_where_count_zero": bool(torch.equal(wsum == 0, count == 0))}
        covered = int((count > 0).sum())
        mean_rows = float(count.float().mean())
        del painted, ones, wsum, count, words, image
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
               "checks": checks, "pixels_with_a_row": covered, "mean_rows_per_pixel": mean_rows}
        for k in sides:
            row[f"{k}_ms"] = stats(ms[k])
        for k in ("values_c1", "values_c3", "values_c4", "values_c4_wsum"):
            for other in ("forward", "pixels_all"):
                if k in sides and other in sides:
                    row[f"{k}_over_{other}_median"] = row[f"{k}_ms"]["median"] / row[f"{other}_ms"]["median"]
                    row[f"{k}_{other}_ranges_overlap"] = (row[f"{k}_ms"]["min"] <= row[f"{other}_ms"]["max"] and
                                                          row[f"{other}_ms"]["min"] <= row[f"{k}_ms"]["max"])
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fo:
                fo.write(line + "\n")
        if not all(checks.values()):
            raise SystemExit(f"bench_values.py: the painted image disagrees with the forward on the {name} frame: {checks}")
        del s, kept, colors, table
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
