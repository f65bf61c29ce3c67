#!/usr/bin/env python
"""Budget-exact hierarchy cut figures, one JSON line per measurement.

  (a) cut   hgs.frustum.cut_to_budget at a budget of a quarter of the cut at the request (rows cost, with the cull and
            without) against hgs.frustum.cut_view at the tau* it returned, on the same hierarchy and view, in the same
            run: hipEvents around the Python calls (each contains one host wait), alternated over --reps repetitions
            after a warm-up: minimum, median, maximum.  The two views of scripts/bench_frustum.py.  The target is
            cut_to_budget < 2 cut_view calls (what the regulator pays at the least when a request does not fit), with
            ranges that do not overlap.
  (b) fly   the 50 M-node, 6 GB fly-through of scripts/bench_frustum.py with fit="budget" against fit="regulate", each
            with and without ``frustum=``: frames/s, p50 / p99, tau per frame, occupancy, cuts per frame, retries.

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--parts a --sizes 50000000 --reps 2).

    python scripts/bench_budget_cut.py [--sizes 1000000 10000000 50000000] [--parts a b] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_frustum import H, ROOT, W, planes_of, stats, timed, yaw_camera      # noqa: E402  (sets sys.path for hgs)

from hgs import frustum, hierarchy, synth            # noqa: E402


def part_cut(h, bounds, tau, reps, warmup):
    dev = h.nodes.device
    G = int(h.nodes.shape[0])
    bufs = frustum.CutBuffers(G, dev)
    rows = []
    for view, cam in (("outside", synth.make_camera(W, H)), ("inside", yaw_camera((0.0, 0.0, 10.0), 120.0))):
        vp = cam.camera_center.cpu()
        planes, rs = planes_of(cam)
        for culled in (True, False):
            pl, r, bnd = (planes, rs, bounds) if culled else (None, 1.0, None)
            all_in = torch.tensor([[0.0, 0.0, 1.0, 1e30]] * 5)
            at_request = frustum.cut_view(h.nodes, h.boxes, bounds, tau, vp, planes if culled else all_in, rs, out=bufs)
            budget = max(at_request.n // 4, 1)

            def exact():
                return frustum.cut_to_budget(h.nodes, h.boxes, bnd, budget, vp, pl, r, tau_min=tau, cost="rows", out=bufs)

            star = exact().tau

            def one_cut():
                return frustum.cut_view(h.nodes, h.boxes, bounds, star, vp, planes if culled else all_in, rs, out=bufs)

            for _ in range(warmup):
                exact(); one_cut()
            t = {"budget": [], "cut_view": []}
            for _ in range(reps):
                ms, bc = timed(exact)
                t["budget"].append(ms)
                ms, cv = timed(one_cut)
                t["cut_view"].append(ms)
            assert (bc.n, bc.n_unculled, bc.tau) == (cv.n, cv.n_unculled, star)
            rows.append({"part": "cut", "nodes": G, "view": view, "culled": culled, "request_tau": tau, "budget_rows": budget,
                         "entries_at_request": at_request.n, "tau_star": star, "entries": bc.n, "cost_rows": bc.cost,
                         "reps": reps, "cut_to_budget_ms": stats(t["budget"]), "cut_view_ms": stats(t["cut_view"]),
                         "ratio_median": stats(t["budget"])["median"] / stats(t["cut_view"])["median"],
                         "below_two_cuts_ranges_apart": max(t["budget"]) < 2 * min(t["cut_view"])})
    return rows


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
        for fit in ("regulate", "budget"):
            for culled in (False, True):
                bh = BudgetedHierarchy(h.xyz.cpu(), h.shs.cpu(), h.alpha.cpu(), torch.exp(h.log_scales).cpu(), h.rots.cpu(),
                                       dev, budget_mb=budget_mb)
                m2 = torch.zeros(bh.B, 3, device=dev)
                fkw = (lambda k: dict(frustum=frs[k], fit=fit)) if culled else (lambda k: dict(fit=fit))
                sels = []

                def frame(k):
                    sel = bh.select(h.nodes, h.boxes, tau, vps[k][0], vps[k][1], **fkw(k))
                    kw = dict(kws[k], interpolation_weights=sel.weights, num_node_kids=sel.kids,
                              render_indices=sel.render_indices, parent_indices=sel.parent_indices)
                    with torch.no_grad():
                        dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw))(
                            means3D=bh.means3D, means2D=m2, shs=bh.shs, opacities=bh.opacities, scales=bh.scales,
                            rotations=bh.rotations)
                    sels.append((sel.n, sel.tau, sel.misses, sel.attempts))
                    if k + 1 < total:
                        bh.prefetch(h.nodes, h.boxes, tau, vps[k + 1][0], vps[k + 1][1], **fkw(k + 1))
                    return sel

                for k in range(warmup):
                    frame(k)
                torch.cuda.synchronize()
                sels.clear()
                f0, r0 = bh.stats["rows_fetched"], bh.stats["retries"]
                ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
                ends[0].record()
                t0 = time.perf_counter()
                for i in range(steps):
                    sel = frame(warmup + i)
                    ends[i + 1].record()
                torch.cuda.synchronize()
                elapsed = time.perf_counter() - t0
                ms = sorted(ends[i].elapsed_time(ends[i + 1]) for i in range(steps))
                used = int(torch.unique(torch.cat([sel.render_indices, sel.parent_indices])).numel())
                rows.append({"part": "fly", "fit": fit, "frustum": culled, "nodes": G, "budget_mb": budget_mb,
                             "budget_rows": bh.B, "steps": steps, "warmup": warmup, "requested_tau_px": tau_px,
                             "frames_per_s": steps / elapsed,
                             "frame_ms": {"p50": ms[len(ms) // 2], "p99": ms[min(len(ms) - 1, int(0.99 * len(ms)))], "max": ms[-1]},
                             "rendered_tau_px": [round(px(s[1]), 3) for s in sels],
                             "mean_cut": sum(s[0] for s in sels) / len(sels),
                             "cuts_per_frame": sum(s[3] for s in sels) / len(sels),
                             "last_frame_occupancy": used / bh.B,
                             "rows_fetched_per_frame": (bh.stats["rows_fetched"] - f0) / steps,
                             "retries": bh.stats["retries"] - r0, "retries_with_warmup": bh.stats["retries"]})
                print(json.dumps(rows[-1]), flush=True)
                if fit == "budget":
                    assert bh.stats["retries"] == 0, "fit='budget' retried a cut"
                del bh, m2
                torch.cuda.empty_cache()
    finally:
        ghC.set_viewpoint_cache(prev_cache)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[1_000_000, 10_000_000, 50_000_000], help="nodes")
    ap.add_argument("--parts", nargs="+", default=["a", "b"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tau-px", type=float, default=3.0)
    ap.add_argument("--budget-mb", type=float, default=6000.0)
    ap.add_argument("--fly-steps", type=int, default=32)
    ap.add_argument("--fly-warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f12_budget_cut_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_budget_cut.py needs a GPU")
    dev = torch.device("cuda:0")
    cam = synth.make_camera(W, H)
    tau = (2 * args.tau_px + 1) * cam.tanfovx / (0.5 * W)
    lines = []
    for nodes in sorted(args.sizes):
        h = hierarchy.build_hierarchy_on_device((nodes + 1) // 2, cam, dev, seed=0)
        out = []
        if "a" in args.parts:
            bounds = frustum.cull_bounds(h.nodes, h.xyz.contiguous(), torch.exp(h.log_scales).contiguous())
            out += part_cut(h, bounds, tau, args.reps, args.warmup)
            del bounds
            for r in out:
                print(json.dumps(r), flush=True)
        if "b" in args.parts and nodes == max(args.sizes):
            out += part_fly(h, args.tau_px, args.budget_mb, args.fly_steps, args.fly_warmup)
        lines += [json.dumps(r) for r in out]
        del h
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
