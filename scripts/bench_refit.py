#!/usr/bin/env python
"""Box refit figures, one JSON line per size:

  hierarchies     hgs.hierarchy.build_hierarchy_on_device, --sizes nodes each (balanced binary, BFS numbering)
  hip             hgs.hierarchy.refit_boxes_gpu (hgs_hier_refit): leaf rules "cube" and "keep", out of place and in place
  torch           this project's torch statement of the same rule on the same GPU (torch_refit below), out of place: the
                  leaf formula in float64, one stable sort of the depth column and a bincount (one host read, as the
                  HIP call has one), then per level a scatter_reduce amin / amax of the level's boxes into their parents
  each            --reps alternated repetitions after one warm-up call of each, device events around the whole call (the
                  HIP call's host wait included): median, min and max.  The outputs are compared before anything is
                  timed: kept leaves and their unions bit for bit, cube leaves and their unions within 1 float32 ulp
                  (torch's float64 exp against the device library's).
  floor_ms        the bytes the rule cannot avoid -- per node the 28-byte record, one box read and one box written, and on
                  the leaves (half the nodes) the 40 bytes of mean, log-scales and rotation: 28 + 64 + 20 = 112 bytes
                  ("cube" does not read the rotations and "keep" reads no row: the one figure is used for all) -- at
                  8 TB/s; share = floor_ms / the HIP median

    python scripts/bench_refit.py [--sizes 1000000 10000000 50000000] [--reps 15] [--out profiles/f19_refit_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))

from hgs import hierarchy, synth   # noqa: E402

PEAK_BYTES_PER_MS = 8.0e9           # 8 TB/s
FLOOR_BYTES_PER_NODE = 112


def torch_refit(h, leaf):
    """The rule in torch ops -> boxes [N,2,4]."""
    N = h.num_nodes
    nodes = h.nodes
    depth, parent, is_leaf = nodes[:, 0].long(), nodes[:, 1].long(), nodes[:, 6] == 0
    inf = float("inf")
    if leaf == "keep":
        lo = torch.where(is_leaf[:, None], h.boxes[:, 0, :3], torch.full_like(h.boxes[:, 0, :3], inf))
        hi = torch.where(is_leaf[:, None], h.boxes[:, 1, :3], torch.full_like(h.boxes[:, 1, :3], -inf))
    else:
        x = h.xyz[:N].double()
        e = 3.0 * torch.exp(h.log_scales[:N].double()).max(1, keepdim=True).values
        lo = torch.where(is_leaf[:, None], (x - e).float(), torch.full((N, 3), inf, device=x.device))
        hi = torch.where(is_leaf[:, None], (x + e).float(), torch.full((N, 3), -inf, device=x.device))
    order = torch.sort(depth, stable=True).indices
    counts = torch.bincount(depth).tolist()                    # the one host read
    first = N
    for d in range(len(counts) - 1, 0, -1):                    # children before parents
        first -= counts[d]
        ids = order[first:first + counts[d]]
        p = parent[ids][:, None].expand(-1, 3)
        lo.scatter_reduce_(0, p, lo[ids], "amin", include_self=True)
        hi.scatter_reduce_(0, p, hi[ids], "amax", include_self=True)
    boxes = h.boxes.clone()
    boxes[:, 0, :3], boxes[:, 1, :3] = lo, hi
    ext = (hi - lo).max(1).values
    boxes[:, 0, 3] = torch.where(is_leaf, h.boxes[:, 0, 3], ext) if leaf == "keep" else ext
    return boxes


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1)


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def ulps(a, b):
    o = lambda t: (lambda i: torch.where(i < 0, -(i & 0x7FFFFFFF), i))(t.contiguous().view(torch.int32).long())
    return (o(a) - o(b)).abs()


def figures(h, reps, dev):
    N = h.num_nodes
    work = hierarchy.Hierarchy(h.xyz, h.shs, h.alpha, h.log_scales, h.rots, h.nodes, h.boxes.clone())   # the in-place runs
    calls = {}
    for leaf in ("cube", "keep"):
        calls[f"hip_{leaf}"] = lambda leaf=leaf: hierarchy.refit_boxes_gpu(h, leaf).boxes
        calls[f"hip_{leaf}_inplace"] = lambda leaf=leaf: hierarchy.refit_boxes_gpu(work, leaf, inplace=True).boxes
        calls[f"torch_{leaf}"] = lambda leaf=leaf: torch_refit(h, leaf)
    # ---- the outputs agree (and every call has run once)
    worst = {}
    for leaf in ("cube", "keep"):
        work.boxes.copy_(h.boxes)                # (the last in-place run left its own output there)
        a, b, c = calls[f"hip_{leaf}"](), calls[f"torch_{leaf}"](), calls[f"hip_{leaf}_inplace"]().clone()
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), "in place differs from out of place"
        worst[leaf] = int(ulps(a, b).max())
        assert worst[leaf] <= (0 if leaf == "keep" else 1), (leaf, worst[leaf])
        del a, b, c
    stats = {}
    hierarchy.refit_boxes_gpu(h, "cube", stats=stats)
    ms = {k: [] for k in calls}
    for _ in range(reps):                       # alternated
        for name, fn in calls.items():
            ms[name].append(timed(fn, dev))
    floor_ms = FLOOR_BYTES_PER_NODE * N / PEAK_BYTES_PER_MS
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = dict(nodes=N, levels=stats["levels"], leaves=stats["leaves"], reps=reps, floor_ms=round(floor_ms, 3),
               cube_ulp_vs_torch=worst["cube"])
    for k, v in ms.items():
        res[k + "_ms"] = summary(v)
    for leaf in ("cube", "keep"):
        res[f"speedup_{leaf}"] = round(med[f"torch_{leaf}"] / med[f"hip_{leaf}"], 2)
        res[f"ranges_apart_{leaf}"] = max(ms[f"hip_{leaf}"]) < min(ms[f"torch_{leaf}"])
        res[f"share_{leaf}"] = round(floor_ms / med[f"hip_{leaf}"], 3)
        res[f"share_{leaf}_inplace"] = round(floor_ms / med[f"hip_{leaf}_inplace"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 10_000_000, 50_000_000])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cam = synth.make_camera(1920, 1080)
    for n in args.sizes:
        h = hierarchy.build_hierarchy_on_device((n + 1) // 2, cam, dev, seed=1)
        res = figures(h, args.reps, dev)
        res["device"] = torch.cuda.get_device_name(dev)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del h
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
