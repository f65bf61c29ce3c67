#!/usr/bin/env python
"""Hierarchy construction figures, one JSON line:

  build_ms        device build (hgs.hierarchy.build_hierarchy_gpu) per leaf count, hipEvents around one build after one
                  warm-up build, leaves from hgs.synth.make_scene
  numpy_1m_s      the float64 numpy spec (hgs.hierarchy.build_hierarchy) at 1 M leaves, one run
  command         python -m hgs.create_hierarchy on a PLY of --e2e-rows rows in the save_ply layout (written to a
                  temporary directory first): read + select, build, write, seconds each

    python scripts/bench_hier_build.py [--sizes 1000000 10000000 30000000] [--e2e-rows 10000000] [--no-numpy]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))

from hgs import create_hierarchy, hierarchy, synth   # noqa: E402


def device_build_ms(P, cam, dev):
    sc = synth.make_scene(P, cam, seed=1).to(dev)
    hierarchy.build_hierarchy_gpu(sc, dev)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    h = hierarchy.build_hierarchy_gpu(sc, dev)
    e1.record()
    e1.synchronize()
    del h, sc
    torch.cuda.empty_cache()
    return e0.elapsed_time(e1)


def write_ply(path, P, seed=0):
    """save_ply layout (scene/gaussian_model.py:491-508), M = 16, raw parameters; written in row blocks."""
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(45)] + \
        ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        f.write(("\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {P}"] +
                           [f"property float {n}" for n in names] + ["end_header"]) + "\n").encode())
        for b0 in range(0, P, 1 << 20):
            n = min(1 << 20, P - b0)
            a = rng.standard_normal((n, len(names)), dtype=np.float32)
            a[:, 0:3] *= 10.0
            a[:, 3:6] = 0.0
            a[:, 55:58] = rng.uniform(-6.0, -2.0, (n, 3)).astype(np.float32)
            f.write(a.astype("<f4").tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 10_000_000, 30_000_000])
    ap.add_argument("--e2e-rows", type=int, default=10_000_000)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cam = synth.make_camera(1920, 1080)
    res = {"build_ms": {str(P): round(device_build_ms(P, cam, dev), 3) for P in args.sizes}}
    if not args.no_numpy:
        sc = synth.make_scene(1_000_000, cam, seed=1)
        t0 = time.perf_counter()
        hierarchy.build_hierarchy(sc)
        res["numpy_1m_s"] = round(time.perf_counter() - t0, 2)
    if args.e2e_rows > 0:
        with tempfile.TemporaryDirectory() as tmp:
            ply_path = os.path.join(tmp, "point_cloud.ply")
            write_ply(ply_path, args.e2e_rows)
            r = create_hierarchy.run(ply_path, tmp, os.path.join(tmp, "out"))
            res["command"] = dict(rows=r["rows_kept"], nodes=r["nodes"], read_s=round(r["read_s"], 2),
                                  build_ms=round(r["build_ms"], 2), write_s=round(r["write_s"], 2),
                                  hier_bytes=os.path.getsize(r["path"]))
    res["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
