#!/usr/bin/env python
"""Half-precision hierarchy rows, one JSON line per measurement.

  (a) fetch  one sorted miss list of m rows (every fourth host row) at M = 16 through hgs_resid_fetch_half (128-byte
             host rows) and hgs_resid_fetch (256-byte host rows) into the same slot arrays, alternated in one run:
             hipEvents around the C call, --reps repetitions after a warm-up, minimum / median / maximum, and whether
             the two ranges overlap.  The expectation from the bytes is about half at the largest size; it is reported,
             not asserted.
  (b) fly    the 50 M-node fly-through of bench.py's config5_budgeted_6gb (3840x2160, 6 GB of rows on the GPU, forward
             0.08 units per frame, one 2-unit jump sideways, prefetch of the next view) with rows="float" and with
             rows="half": frames/s, p50 / p99 / max frame time, rows and bytes fetched per frame.  The jump frame (p99,
             max) is the number of interest.
  (c) setup  BudgetedHierarchy.from_device_arrays against the CPU constructor at the same size, both formats: seconds
             and the process's peak resident set.  Each of the four runs is its own child process (ru_maxrss is a
             high-water mark).
  (d) psnr   rows="half" against rows="float" (the unrounded attributes): PSNR of the in-op LOD render at tau = 3 px on
             the tests' 2 000-leaf scene and on a 20 000-leaf trained-like scene.  No bar is set for it.

    python scripts/bench_half_rows.py [--parts a b c d] [--fetch-rows 10000 250000 1400000] [--nodes 50000000]
                                      [--reps 7] [--out FILE]"""
import argparse
import ctypes as C
import json
import math
import os
import resource
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hgs import _lib, hierarchy, residency, synth            # noqa: E402
from hgs.residency import BudgetedHierarchy                  # noqa: E402

W, H = 3840, 2160
KEYS = ("means3D", "shs", "opacities", "scales", "rotations")


def stats(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v))


def activated(h):
    """The rasterizer's five arrays of a hierarchy, on its device."""
    return dict(means3D=h.xyz.contiguous(), shs=h.shs.contiguous(), opacities=h.alpha.abs().reshape(-1, 1).contiguous(),
                scales=torch.exp(h.log_scales), rotations=torch.nn.functional.normalize(h.rots))


# ---- (a) ----------------------------------------------------------------------------------------------------------
def part_fetch(dev, sizes, reps, warmup):
    lib, p, M = _lib.lib(), _lib.ptr, 16
    m_max = max(sizes)
    G = 4 * m_max
    rng = np.random.default_rng(0)
    hosts = {}
    for fmt, width in (("float", 256), ("half", 128)):
        arr, ptr = residency._host_array((G, width), np.uint8)
        tile = rng.integers(0, 0x3C, (4096, width), dtype=np.uint8)      # (small positive halves / floats: no NaN, no inf)
        for a in range(0, G, 4096):
            arr[a:a + 4096] = tile[:min(4096, G - a)]
        hosts[fmt] = (arr, ptr)
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    slots = [torch.zeros(m_max, 3, **f32), torch.zeros(m_max, M, 3, **f32), torch.zeros(m_max, 1, **f32),
             torch.zeros(m_max, 3, **f32), torch.zeros(m_max, 4, **f32)]
    slot_rows = _lib.ResidRows(*[C.c_void_p(t.data_ptr()) for t in slots])
    slot_of, id_of_slot = torch.full((G,), -1, **i32), torch.full((m_max,), -1, **i32)
    stamp, free_list = torch.zeros(m_max, **i32), torch.arange(m_max - 1, -1, -1, **i32)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    calls = {"float": lib.hgs_resid_fetch, "half": lib.hgs_resid_fetch_half}
    rows = []
    for m in sorted(sizes):
        miss = (torch.arange(m, **i32) * 4 + 1).contiguous()             # sorted, every fourth row
        t = {"float": [], "half": []}

        def run(fmt):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(calls[fmt](p(miss), m, p(free_list), m_max, p(slot_of), p(id_of_slot), p(stamp), 1,
                                  C.c_void_p(hosts[fmt][1]), C.byref(slot_rows), M, stream, dev.index or 0), fmt)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(warmup):
            run("float"); run("half")
        for _ in range(reps):
            t["float"].append(run("float"))
            t["half"].append(run("half"))
        rows.append({"part": "fetch", "rows": m, "M": M, "host_rows": G, "reps": reps, "float_ms": stats(t["float"]),
                     "half_ms": stats(t["half"]), "ratio_median": statistics.median(t["half"]) / statistics.median(t["float"]),
                     "float_GBps": m * 256 / statistics.median(t["float"]) / 1e6,
                     "half_GBps": m * 128 / statistics.median(t["half"]) / 1e6,
                     "ranges_overlap": not (max(t["half"]) < min(t["float"]) or max(t["float"]) < min(t["half"]))})
        print(json.dumps(rows[-1]), flush=True)
    torch.cuda.synchronize()
    for arr, ptr in hosts.values():
        lib.hgs_host_free(C.c_void_p(ptr))
    return rows


# ---- (b) ----------------------------------------------------------------------------------------------------------
def part_fly(h, tau_px, budget_mb, steps, warmup):
    import diff_gaussian_rasterization as dgr
    import parity as pa
    from gaussian_hierarchy import _C as ghC
    dev = h.nodes.device
    G = int(h.nodes.shape[0])
    cam0 = synth.make_camera(W, H)
    tau = (2 * tau_px + 1) * cam0.tanfovx / (0.5 * W)
    total, jump = warmup + steps, warmup + steps // 2
    cams = [synth.make_camera(W, H, T=np.array([-(2.0 if k >= jump else 0.0), 0.0, -0.08 * k])) for k in range(total)]
    vps = [(c.camera_center.to(dev), c.camera_center.cpu()) for c in cams]
    kws = [pa.settings_kwargs(c, torch.zeros(3), 3, do_depth=False, device=dev) for c in cams]
    px = lambda t: (t * (0.5 * W) / cam0.tanfovx - 1) / 2
    attrs = activated(h)
    rows = []
    prev_cache = ghC.set_viewpoint_cache(True)
    try:
        for fmt in ("float", "half"):
            bh = BudgetedHierarchy.from_device_arrays(*[attrs[k] for k in KEYS], rows=fmt, budget_mb=budget_mb)
            m2 = torch.zeros(bh.B, 3, device=dev)
            sels = []

            def frame(k):
                sel = bh.select(h.nodes, h.boxes, tau, vps[k][0], vps[k][1])
                kw = dict(kws[k], interpolation_weights=sel.weights, num_node_kids=sel.kids,
                          render_indices=sel.render_indices, parent_indices=sel.parent_indices)
                with torch.no_grad():
                    dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw))(
                        means3D=bh.means3D, means2D=m2, shs=bh.shs, opacities=bh.opacities, scales=bh.scales,
                        rotations=bh.rotations)
                sels.append((sel.n, sel.tau, sel.misses, sel.attempts))
                if k + 1 < total:
                    bh.prefetch(h.nodes, h.boxes, tau, vps[k + 1][0], vps[k + 1][1])

            for k in range(warmup):
                frame(k)
            torch.cuda.synchronize()
            sels.clear()
            f0, b0 = bh.stats["rows_fetched"], bh.stats["bytes_fetched"]
            ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            ends[0].record()
            t0 = time.perf_counter()
            for i in range(steps):
                frame(warmup + i)
                ends[i + 1].record()
            torch.cuda.synchronize()
            elapsed = time.perf_counter() - t0
            per_frame = [ends[i].elapsed_time(ends[i + 1]) for i in range(steps)]
            ms = sorted(per_frame)
            rows.append({"part": "fly", "rows": fmt, "nodes": G, "budget_mb": budget_mb, "budget_rows": bh.B, "steps": steps,
                         "warmup": warmup, "requested_tau_px": tau_px, "frames_per_s": steps / elapsed,
                         "frame_ms": {"p50": ms[len(ms) // 2], "p99": ms[min(len(ms) - 1, int(0.99 * len(ms)))], "max": ms[-1]},
                         "jump_frame_ms": per_frame[steps // 2], "frame_before_jump_ms": per_frame[steps // 2 - 1],
                         "rendered_tau_px_mean": sum(px(s[1]) for s in sels) / len(sels),
                         "rows_fetched_per_frame": (bh.stats["rows_fetched"] - f0) / steps,
                         "bytes_fetched_per_frame": (bh.stats["bytes_fetched"] - b0) / steps,
                         "pinned_host_bytes": int(bh._rows.nbytes), "retries": bh.stats["retries"]})
            print(json.dumps(rows[-1]), flush=True)
            del bh, m2
            torch.cuda.empty_cache()
    finally:
        ghC.set_viewpoint_cache(prev_cache)
    return rows


# ---- (c) ----------------------------------------------------------------------------------------------------------
def setup_child(nodes, how, fmt):
    """One constructor in this process: seconds and the peak resident set (the hierarchy is built on the device; the CPU
    constructor's input copies are made before the clock starts, as bench.py's budgeted loop makes them)."""
    dev = torch.device("cuda:0")
    h = hierarchy.build_hierarchy_on_device((nodes + 1) // 2, synth.make_camera(W, H), dev, seed=0)
    attrs = activated(h)
    base = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    if how == "cpu":
        host = [attrs[k].cpu() for k in KEYS]
        t0 = time.perf_counter()
        bh = BudgetedHierarchy(*host, dev, budget_mb=6000.0, rows=fmt)
    else:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bh = BudgetedHierarchy.from_device_arrays(*[attrs[k] for k in KEYS], rows=fmt, budget_mb=6000.0)
    seconds = time.perf_counter() - t0
    peak = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    print(json.dumps({"part": "setup", "constructor": how, "rows": fmt, "nodes": int(h.nodes.shape[0]), "seconds": seconds,
                      "pinned_host_bytes": int(bh._rows.nbytes), "peak_rss_kb": peak, "rss_before_kb": base}), flush=True)


def part_setup(nodes):
    rows = []
    for how in ("device", "cpu"):
        for fmt in ("float", "half"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--setup-child", how, fmt, "--nodes", str(nodes)],
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"setup child ({how}, {fmt}) failed with status {r.returncode}:\n{r.stderr[-2000:]}")
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[-1]), flush=True)
    return rows


# ---- (d) ----------------------------------------------------------------------------------------------------------
def part_psnr(dev, tau_px):
    import diff_gaussian_rasterization as dgr
    import parity as pa
    w, hh = 320, 200
    cam = synth.make_camera(w, hh)
    tau = (2 * tau_px + 1) * cam.tanfovx / (0.5 * w)
    scenes = [("make_scene, 2 000 leaves, seed 8", synth.make_scene(2_000, cam, seed=8)),
              ("make_scene_trained_like, 20 000 leaves, seed 4", synth.make_scene_trained_like(20_000, cam, seed=4))]
    rows = []
    for name, scene in scenes:
        h = hierarchy.build_hierarchy(scene)
        attrs = {k: v.cpu() for k, v in activated(h).items()}
        nodes, boxes = h.nodes.to(dev), h.boxes.to(dev)
        G = int(attrs["means3D"].shape[0])
        views = [synth.orbit_camera(w, hh, j, 6, radius=0.4, tilt=0.05) for j in range(6)]
        images = {}
        for fmt in ("float", "half"):
            bh = BudgetedHierarchy(*[attrs[k] for k in KEYS], dev, budget_rows=G, rows=fmt)
            images[fmt] = []
            for c in views:
                sel = bh.select(nodes, boxes, tau, c.camera_center.to(dev), c.camera_center.cpu())
                kw = pa.settings_kwargs(c, torch.zeros(3), 3, do_depth=False, device=dev, interpolation_weights=sel.weights,
                                        num_node_kids=sel.kids)
                kw.update(render_indices=sel.render_indices, parent_indices=sel.parent_indices)
                with torch.no_grad():
                    color = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw))(
                        means3D=bh.means3D, means2D=torch.zeros(bh.B, 3, device=dev), shs=bh.shs, opacities=bh.opacities,
                        scales=bh.scales, rotations=bh.rotations)[0]
                images[fmt].append(color.double().cpu())
        psnr, maxabs = [], []
        for a, b in zip(images["half"], images["float"]):
            mse = float(((a - b) ** 2).mean())
            psnr.append(None if mse == 0.0 else 10.0 * math.log10(1.0 / mse))
            maxabs.append(float((a - b).abs().max()))
        scales = attrs["scales"]
        rows.append({"part": "psnr", "scene": name, "rows_G": G, "tau_px": tau_px, "width": w, "height": hh, "views": len(views),
                     "psnr_db": psnr, "psnr_db_min": min(p for p in psnr if p is not None), "max_abs_diff": max(maxabs),
                     "image_max": max(float(a.max()) for a in images["float"]),
                     "share_of_scales_below_2^-14": float((scales < 2.0 ** -14).double().mean()),
                     "sh_abs_max": float(attrs["shs"].abs().max())})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["a", "b", "c", "d"])
    ap.add_argument("--fetch-rows", nargs="+", type=int, default=[10_000, 250_000, 1_400_000])
    ap.add_argument("--nodes", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tau-px", type=float, default=3.0)
    ap.add_argument("--budget-mb", type=float, default=6000.0)
    ap.add_argument("--fly-steps", type=int, default=32)
    ap.add_argument("--fly-warmup", type=int, default=8)
    ap.add_argument("--setup-child", nargs=2, metavar=("CONSTRUCTOR", "ROWS"), help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f14_half_rows_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_half_rows.py needs a GPU")
    if args.setup_child:
        setup_child(args.nodes, *args.setup_child)
        return
    dev = torch.device("cuda:0")
    out = []
    if "d" in args.parts:
        out += part_psnr(dev, args.tau_px)
    if "a" in args.parts:
        out += part_fetch(dev, args.fetch_rows, args.reps, args.warmup)
    if "c" in args.parts:
        out += part_setup(args.nodes)            # (child processes: before this process holds the large hierarchy)
    if "b" in args.parts:
        h = hierarchy.build_hierarchy_on_device((args.nodes + 1) // 2, synth.make_camera(W, H), dev, seed=0)
        out += part_fly(h, args.tau_px, args.budget_mb, args.fly_steps, args.fly_warmup)
        del h
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in out) + "\n")


if __name__ == "__main__":
    main()
