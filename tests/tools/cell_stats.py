#!/usr/bin/env python
"""Work model of the compositing kernels' unit of work (csrc/render.hip), computed on the CPU from the float64 geometry
of a scene (test infrastructure; imports oracle/).  One wave composites a 16x16 tile; the tile is cut into UNITS, each
with its own list of the batch's instances, and one iteration of the inner loop serves the next instance of every
unit's list at once.  A batch therefore costs the length of its longest list.  Units compared:
  quad8x8   four 8x8 quadrants, one 16-lane row each (the layout before the 4x4 cells)
  oct8x4    eight 8x4 octants
  cell4x4   sixteen 4x4 cells, one 4-lane quad each (K6's layout; K7 keeps the quadrants)
Per unit, what decides that an instance enters its list:
  live      some pixel of the unit passes alpha >= 1/255 (the per-pixel test itself: the model's floor)
  box       K1's alpha >= 1/255 box (ext_x, ext_y) against the unit's pixel range, separably by column and row bands
  box_quad  box AND the exact rectangle test of the unit's 8x8 quadrant (what K6 stages: the quadrant's test is
            computed anyway, the cell's own bands cost eight compares)
  box_cell  box AND the exact rectangle test of the unit itself (16 edge maximisations per staged instance)
"rectangle test": the maximum of the Gaussian's exponent over the unit's continuous pixel rectangle reaches the skip
threshold.  Reported per instance: iterations at the batch sizes of the kernels and the (instance, unit) pairs.
`gain_kept` (cells): how much of the floor's gain over the quadrants a test keeps, (quad8x8 box_quad - test) /
(quad8x8 box_quad - live) in iterations.  Early termination is ignored.
    python tests/tools/cell_stats.py [heavy]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "hierarchical-3d-gaussians_amd")):
    sys.path.insert(0, p)
from hgs import synth                       # noqa: E402
from oracle import raster_oracle as ro      # noqa: E402

UNITS = {"quad8x8": (8, 8), "oct8x4": (8, 4), "cell4x4": (4, 4)}
TESTS = ("live", "box", "box_quad", "box_cell")
BATCHES = (64, 48, 32)


def rect_max(A, B, C, lx, hx, ly, hy):
    """max of -0.5 (A dx^2 + C dy^2) - B dx dy over dx in [lx, hx], dy in [ly, hy] (A, C > 0, AC > B^2)"""
    inside = (lx <= 0) & (hx >= 0) & (ly <= 0) & (hy >= 0)
    best = np.full(np.broadcast(A, lx, ly).shape, -np.inf)
    for dx in (lx, hx):                     # vertical edges: maximise over dy
        dy = np.clip(-B * dx / C, ly, hy)
        best = np.maximum(best, -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy)
    for dy in (ly, hy):
        dx = np.clip(-B * dy / A, lx, hx)
        best = np.maximum(best, -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy)
    return np.where(inside, 0.0, best)


def unit_masks(x, y, ex, ey, A, B, C, thr, live_px, uw, uh):
    """(instances, units) hit masks of every test for units of uw x uh pixels; x, y: tile-relative centres"""
    nx, ny = 16 // uw, 16 // uh
    out = {t: [] for t in TESTS}
    for cy in range(ny):
        for cx in range(nx):
            x0, y0 = cx * uw, cy * uh
            x1, y1 = x0 + uw - 1, y0 + uh - 1
            box = (x - ex <= x1) & (x + ex >= x0) & (y - ey <= y1) & (y + ey >= y0)
            qx0, qy0 = (x0 // 8) * 8, (y0 // 8) * 8
            quad = rect_max(A, B, C, x - (qx0 + 7), x - qx0, y - (qy0 + 7), y - qy0) >= thr
            cell = rect_max(A, B, C, x - x1, x - x0, y - y1, y - y0) >= thr
            out["live"].append(live_px[:, y0:y1 + 1, x0:x1 + 1].any((1, 2)))
            out["box"].append(box)
            out["box_quad"].append(box & quad)
            out["box_cell"].append(box & cell)
    return {t: np.stack(v, 1) for t, v in out.items()}


def main(P=1_000_000, W=1920, H=1080, n_tiles=300, s_px=(0.5, 4.0)):
    cam = synth.make_camera(W, H)
    scene = synth.make_scene(P, cam, seed=0, s_px=s_px)
    geom = ro.geometry_spec(scene.means3D.numpy(), scene.scales.numpy(), scene.rotations.numpy(), None,
                            cam.world_view_transform.numpy(), cam.full_proj_transform.numpy(), W, H,
                            float(np.float32(cam.tanfovx)), float(np.float32(cam.tanfovy)), 1.0)
    b = ro.binning_spec(geom)
    gx = geom.grid[0]
    tiles = np.random.default_rng(0).choice(gx * geom.grid[1], size=n_tiles, replace=False)
    op = scene.opacities.numpy().reshape(-1).astype(np.float64)
    A, B, C = (geom.conic[:, i].astype(np.float64) for i in range(3))
    thr_all = np.log(1.0 / (255.0 * np.maximum(op, 1e-300)))              # power >= thr  <=>  o exp(power) >= 1/255
    T2 = 2.0 * (np.log(np.maximum(255.0 * op, 1e-300)) + 1e-3 * 0.6931471805599453)
    det = A * C - B * B
    ok = (T2 > 0) & (det > 0)
    ex = np.where(ok, np.sqrt(np.maximum(T2 * C / np.where(ok, det, 1), 0)) * 1.0001 + 5e-3, -1.0)
    ey = np.where(ok, np.sqrt(np.maximum(T2 * A / np.where(ok, det, 1), 0)) * 1.0001 + 5e-3, -1.0)
    pix = np.arange(16, dtype=np.float64)
    it = {(u, t, bs): 0 for u in UNITS for t in TESTS for bs in BATCHES}
    pairs = {(u, t): 0 for u in UNITS for t in TESTS}
    n_inst = live_px_total = 0
    for t in tiles:
        s, e = b.ranges[t]
        if e <= s:
            continue
        ids = b.point_list[s:e]
        x = geom.px[ids].astype(np.float64) - (t % gx) * 16
        y = geom.py[ids].astype(np.float64) - (t // gx) * 16
        a, bb, c, thr = A[ids], B[ids], C[ids], thr_all[ids]
        dx = x[:, None, None] - pix[None, None, :]
        dy = y[:, None, None] - pix[None, :, None]
        power = -0.5 * (a[:, None, None] * dx * dx + c[:, None, None] * dy * dy) - bb[:, None, None] * dx * dy
        live_px = np.minimum(op[ids][:, None, None] * np.exp(np.minimum(power, 0.0)), 0.99) >= 1.0 / 255.0
        n_inst += len(ids)
        live_px_total += int(live_px.sum())
        for u, (uw, uh) in UNITS.items():
            masks = unit_masks(x, y, ex[ids], ey[ids], a, bb, c, thr, live_px, uw, uh)
            for tname, m in masks.items():
                pairs[(u, tname)] += int(m.sum())
                for bs in BATCHES:
                    for b0 in range(0, len(ids), bs):
                        it[(u, tname, bs)] += int(m[b0:b0 + bs].sum(0).max())
    res = {}
    floor = {bs: it[("quad8x8", "box_quad", bs)] for bs in BATCHES}
    for u in UNITS:
        for tname in TESTS:
            row = {f"iterations_per_instance_b{bs}": round(it[(u, tname, bs)] / n_inst, 4) for bs in BATCHES}
            row["pairs_per_instance"] = round(pairs[(u, tname)] / n_inst, 3)
            if u == "cell4x4" and tname != "live":
                row["gain_kept_b64"] = round((floor[64] - it[(u, tname, 64)]) / max(floor[64] - it[(u, "live", 64)], 1), 3)
                row["gain_kept_b32"] = round((floor[32] - it[(u, tname, 32)]) / max(floor[32] - it[(u, "live", 32)], 1), 3)
            res[f"{u}/{tname}"] = row
    print(json.dumps(dict(scene=f"{P} Gaussians, {W}x{H}, s_px {s_px}", tiles=n_tiles, instances=n_inst,
                          live_pixels_per_instance=round(live_px_total / n_inst, 2), units=res), indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "heavy":
        main(s_px=(1.0, 8.0))
    else:
        main()
