#!/usr/bin/env python
"""Image-attribution figures, one JSON line per frame:

  attr1_ms / attr3_ms   the attribution call alone (hgs_raster_attribute: tile kernel + per-Gaussian sum) with C = 1 and
                        C = 3 on the workspaces of a forward that is NOT in the timed window
  contrib_ms            (a) hgs_raster_contrib on the same forward: what the extra channels cost
  trick_ms              (b) the only route to these numbers without the call: a forward with colors_precomp that requires
                        a gradient, then the backward seeded with the image f, whose dL/dcolors is A (three channels in
                        one pass); trick_bwd_ms is its backward alone

Frames: ``metric`` (synth.make_scene, 1 M Gaussians, 1920 x 1080) and ``trained`` (synth.make_scene_trained_scale, 375 k
Gaussians, 10 M instances).  Device events around the calls, warm-up first, the sides alternated over --reps repetitions:
median, minimum, maximum.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--reps 3).
Before timing, the call's sums are compared with the trick's on the same frame (they must agree to float32 rounding).

    python scripts/bench_attribute.py [--frames metric trained] [--reps 15] [--only attr1|attr3|contrib|trick] [--out file.jsonl]"""
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
SIDES = ("attr1", "attr3", "contrib", "trick")


def settings(cam, dev):
    e_i, e_f = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, device=dev)
    return dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=dev),
        scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
        sh_degree=3, campos=cam.camera_center.to(dev), prefiltered=False, debug=False, render_indices=e_i,
        parent_indices=e_i, interpolation_weights=e_f, num_node_kids=e_i, do_depth=False)


def forward(rs, s, colors):
    """The no-grad forward with colors_precomp -> its call (the weights do not depend on the colours)."""
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
        raise SystemExit("bench_attribute.py needs a GPU")
    dev = torch.device("cuda:0")
    cam = synth.make_camera(W, H)
    for name in args.frames:
        s = FRAMES[name](cam).to(dev)
        P = s.P
        rs = settings(cam, dev)
        colors = torch.rand(P, 3, device=dev)
        rast = dgr.GaussianRasterizer(rs)
        m2 = torch.zeros(P, 3, device=dev)
        f = torch.randn(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        f1 = f[:1].contiguous()
        out1 = torch.zeros(P, 1, dtype=torch.float64, device=dev)
        out3 = torch.zeros(P, 3, dtype=torch.float64, device=dev)
        ws = torch.zeros(P, dtype=torch.float64, device=dev)
        wmax = torch.zeros(P, device=dev)
        wsum = torch.zeros(P, dtype=torch.float64, device=dev)
        count = torch.zeros(P, dtype=torch.int64, device=dev)

        def trick_fwd():
            c = colors.detach().requires_grad_(True)
            color, _, _ = rast(means3D=s.means3D, means2D=m2, colors_precomp=c, opacities=s.opacities, scales=s.scales,
                               rotations=s.rotations)
            return c, color

        def trick():
            c, color = trick_fwd()
            color.backward(f)
            return c.grad

        kept = forward(rs, s, colors)             # the forward whose workspaces the timed calls read
        sides = {"attr1": lambda: _C.raster_attribute(kept, f1, out1, wsum=ws),
                 "attr3": lambda: _C.raster_attribute(kept, f, out3, wsum=ws),
                 "contrib": lambda: _C.raster_contributions(kept, wmax, wsum, count),
                 "trick": trick}
        # same numbers first: the call's sums against the trick's colour gradient, in units of the fold of |f|
        sides["attr3"]()
        absf = torch.zeros(P, 3, dtype=torch.float64, device=dev)
        _C.raster_attribute(kept, f.abs(), absf)
        ref = trick().double()
        torch.cuda.synchronize()
        err = float(((out3 - ref).abs() / (absf + 1e-6 * absf.max())).max())
        blended = int((ws > 0).sum())
        if args.only:
            sides = {args.only: sides[args.only]}
        for _ in range(args.warmup):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        bwd = []
        for _ in range(args.reps):
            for k, fn in sides.items():
                if k == "trick":                  # also its backward alone
                    t_f, (c, color) = timed(trick_fwd)
                    t_b, _ = timed(lambda: color.backward(f))
                    ms[k].append(t_f + t_b)
                    bwd.append(t_b)
                else:
                    ms[k].append(timed(fn)[0])
        row = {"frame": name, "gaussians": P, "width": W, "height": H, "instances": int(kept.L), "reps": args.reps,
               "attr3_vs_trick_max_err_over_abs_fold": err, "blended_rows": blended}
        for k in sides:
            row[f"{k}_ms"] = stats(ms[k])
        if bwd:
            row["trick_bwd_ms"] = stats(bwd)
        for k in ("attr1", "attr3"):
            if k in sides and "trick" in sides:
                row[f"trick_over_{k}_median"] = row["trick_ms"]["median"] / row[f"{k}_ms"]["median"]
                row[f"{k}_trick_ranges_overlap"] = row[f"{k}_ms"]["max"] >= row["trick_ms"]["min"]
            if k in sides and "contrib" in sides:
                row[f"{k}_over_contrib_median"] = row[f"{k}_ms"]["median"] / row["contrib_ms"]["median"]
                row[f"{k}_contrib_ranges_overlap"] = (row[f"{k}_ms"]["min"] <= row["contrib_ms"]["max"] and
                                                      row["contrib_ms"]["min"] <= row[f"{k}_ms"]["max"])
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fo:
                fo.write(line + "\n")
        del s, kept, colors, out1, out3, ws, wmax, wsum, count, f, f1, m2, absf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
