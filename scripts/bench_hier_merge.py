#!/usr/bin/env python
"""Hierarchy consolidation figures, one JSON line:

  merge           per merged size: hgs.hierarchy.merge_hierarchies_gpu against the torch spec merge_hierarchies on the
                  same device-resident chunks (hgs.hierarchy.build_hierarchy_on_device), hipEvents around one call after
                  one warm-up call of each, and the peak device memory of each call above what was allocated before it
                  (the chunks themselves not counted); device_ms is the sum of the events around the placements and the
                  root inside merge_hierarchies_gpu
  command         python -m hgs.merge_hierarchies on --e2e-chunks chunk files of --e2e-leaves leaves each (written to a
                  temporary directory first, with skybox tails): read, device merge, write, seconds each

    python scripts/bench_hier_merge.py [--sizes 10000000 50000000] [--chunks 4 10] [--e2e-chunks 4]
                                       [--e2e-leaves 1000000]"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))

from hgs import hierarchy, merge_hierarchies, synth   # noqa: E402


def timed(fn, dev):
    """-> (result, ms from events, peak bytes above the allocation before the call)."""
    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1), torch.cuda.max_memory_allocated(dev) - base


def merge_figures(n_nodes, k, cam, dev):
    P = (n_nodes // k + 1) // 2
    chunks = [hierarchy.build_hierarchy_on_device(P, cam, dev, seed=i) for i in range(k)]
    N = hierarchy.merge_layout([c.num_nodes for c in chunks])[1]
    hierarchy.merge_hierarchies_gpu(chunks, dev)
    stats = {}
    h, gpu_ms, gpu_peak = timed(lambda: hierarchy.merge_hierarchies_gpu(chunks, dev, stats), dev)
    del h
    hierarchy.merge_hierarchies(chunks[:1])
    h, spec_ms, spec_peak = timed(lambda: hierarchy.merge_hierarchies(chunks), dev)
    del h, chunks
    torch.cuda.empty_cache()
    return dict(chunks=k, nodes=N, gpu_ms=round(gpu_ms, 2), device_ms=round(stats["merge_ms"], 2),
                gpu_peak_mb=round(gpu_peak / 2**20, 1), spec_ms=round(spec_ms, 2),
                spec_peak_mb=round(spec_peak / 2**20, 1))


def command_figures(k, P, cam, dev):
    from gaussian_hierarchy._C import write_hierarchy
    names = [f"{i}_0" for i in range(k)]
    with tempfile.TemporaryDirectory() as tmp:
        for i, n in enumerate(names):
            h = hierarchy.build_hierarchy_on_device(P, cam, dev, seed=100 + i)
            tail = 10_000
            g = torch.Generator(device=dev).manual_seed(i)
            r = lambda *s: torch.randn(*s, generator=g, device=dev)
            d = os.path.join(tmp, "trained_chunks", n)
            os.makedirs(d)
            write_hierarchy(os.path.join(d, "hierarchy.hier_opt"), torch.cat([h.xyz, r(tail, 3)]),
                            torch.cat([h.shs, r(tail, 16, 3)]), torch.cat([h.alpha, r(tail, 1).abs()]),
                            torch.cat([h.log_scales, r(tail, 3)]), torch.cat([h.rots, r(tail, 4)]), h.nodes, h.boxes)
            del h
        out = os.path.join(tmp, "merged.hier")
        r = merge_hierarchies.run(os.path.join(tmp, "trained_chunks"), os.path.join(tmp, "chunks"), out, names)
        return dict(chunks=k, merged_nodes=r["merged"], read_s=round(r["read_s"], 2), merge_ms=round(r["merge_ms"], 2),
                    merge_s=round(r["merge_s"], 2), write_s=round(r["write_s"], 2), hier_bytes=os.path.getsize(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[10_000_000, 50_000_000])
    ap.add_argument("--chunks", type=int, nargs="*", default=[4, 10])
    ap.add_argument("--e2e-chunks", type=int, default=4)
    ap.add_argument("--e2e-leaves", type=int, default=1_000_000)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cam = synth.make_camera(1920, 1080)
    res = {"merge": {str(n): merge_figures(n, k, cam, dev) for n, k in zip(args.sizes, args.chunks)}}
    if args.e2e_chunks > 0:
        res["command"] = command_figures(args.e2e_chunks, args.e2e_leaves, cam, dev)
    res["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
