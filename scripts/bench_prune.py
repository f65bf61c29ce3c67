#!/usr/bin/env python
"""Leaf-removal figures, one JSON line per (size, case):

  hierarchies     hgs.hierarchy.build_hierarchy_on_device, --sizes nodes each (16 SH coefficients: 296 bytes per node)
  cases           box: one remove box about the centre of the leaves, its size bisected until about a tenth of the leaves
                  lie in it (few dirty nodes); opacity: the opacity floor at the leaves' 10 % quantile (a tenth of the
                  leaves, scattered: many dirty nodes); second: every second leaf by a mask (nearly every interior dirty)
  hip             hgs.hierarchy.prune_hierarchy_gpu, remerge="dirty" (hgs_hier_prune_plan, the allocation,
                  hgs_hier_prune_apply); for the box case also remerge="none"
  identity_trim   hgs.hierarchy.trim_hierarchy_gpu with no floor: the identity copy of the same hierarchy, the bytes a
                  prune must at least move
  torch           (box case) this project's torch statement of the TOPOLOGY of the rule on the same GPU (torch_prune
                  below): the removal test, alive bottom-up with one index_reduce per depth, a cumulative sum,
                  index_select per tensor, the record rewrite; no checks, no box unions, no re-merge: it is to be read
                  against the remerge="none" figure
  each            --reps alternated repetitions after one warm-up call of each, device events around the call: median,
                  min and max.  The torch statement's records and maps are compared with the HIP call's before timing.

    python scripts/bench_prune.py [--sizes 1000000 10000000 50000000] [--reps 15] [--out profiles/f21_prune_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))

from hgs import hierarchy, synth   # noqa: E402

ARRAYS = ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes")


def torch_prune(h, lo, hi):
    """The topology of the rule for one remove box in torch ops -> (nodes int32 [N',7], old_of_new, new_of_old, rows)."""
    nodes = h.nodes
    N = nodes.shape[0]
    depth, parent, sc, cc = nodes[:, 0].long(), nodes[:, 1].long(), nodes[:, 5].long(), nodes[:, 6]
    leaf = cc == 0
    inside = ((h.xyz[:N] >= lo) & (h.xyz[:N] <= hi)).all(1)
    alive = (leaf & ~inside).to(torch.float32)
    order = torch.argsort(depth, stable=True)
    counts = torch.bincount(depth).tolist()
    end = N
    for d in range(len(counts) - 1, 0, -1):                  # children before parents: alive[parent] |= alive[node]
        ids = order[end - counts[d]:end]
        end -= counts[d]
        alive.index_reduce_(0, parent[ids], alive[ids], "amax", include_self=True)
    keep = alive.bool()
    new_of_old = torch.where(keep, torch.cumsum(keep, 0, dtype=torch.int32) - 1, -1).to(torch.int32)
    old = keep.nonzero().flatten()
    # surviving children: a count and the first one per parent
    surviving = torch.zeros(N, dtype=torch.float32, device=nodes.device).index_add_(0, parent[old[1:]], alive[old[1:]])
    first = torch.full((N,), float(N), dtype=torch.float64, device=nodes.device).index_reduce_(0, parent[old[1:]], old[1:].double(), "amin").long()
    nd = nodes.index_select(0, old)
    inner = nd[:, 6] > 0
    nd[:, 1] = torch.where(old == 0, -1, new_of_old[nd[:, 1].clamp_min(0).long()])
    nd[:, 2] = torch.arange(old.numel(), dtype=torch.int32, device=old.device)
    nd[:, 5] = torch.where(inner, new_of_old[first[old].clamp_max(N - 1)], nd[:, 5])
    nd[:, 6] = torch.where(inner, surviving[old].to(torch.int32), nd[:, 6])
    rows = [getattr(h, k).index_select(0, old) for k in ("xyz", "shs", "alpha", "log_scales", "rots", "boxes")]
    return nd, old.to(torch.int32), new_of_old, rows


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    out = fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]), out


def summary(ms):
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3))


def tenth_box(xyz_leaves):
    """A box about the leaves' median whose half size is bisected until about a tenth of the leaves lie in it."""
    c = xyz_leaves.median(0).values
    span = (xyz_leaves.max(0).values - xyz_leaves.min(0).values)
    a, b = 0.0, 0.5
    for _ in range(30):
        m = 0.5 * (a + b)
        share = float(((xyz_leaves >= c - m * span) & (xyz_leaves <= c + m * span)).all(1).float().mean())
        a, b = (m, b) if share < 0.1 else (a, m)
    m = 0.5 * (a + b)
    return c - m * span, c + m * span


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000, 50_000_000])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f21_prune_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cam = synth.make_camera(256, 160)
    lines = []
    for size in a.sizes:
        h = hierarchy.build_hierarchy_on_device((size + 1) // 2, cam, dev, seed=0)
        N = h.num_nodes
        leaf = h.nodes[:, 6] == 0
        lo, hi = tenth_box(h.xyz[:N][leaf])
        floor = float(torch.quantile(h.alpha[:N].reshape(-1)[leaf][:4_000_000].float(), 0.1))
        ids = leaf.nonzero().flatten()
        second = torch.zeros(N, dtype=torch.uint8, device=dev)
        second[ids[::2]] = 1
        box = [(lo.cpu().numpy(), hi.cpu().numpy())]
        calls = {
            "box": lambda st: hierarchy.prune_hierarchy_gpu(h, remove_boxes=box, stats=st),
            "box_none": lambda st: hierarchy.prune_hierarchy_gpu(h, remove_boxes=box, remerge="none", stats=st),
            "opacity": lambda st: hierarchy.prune_hierarchy_gpu(h, min_opacity=floor, stats=st),
            "second": lambda st: hierarchy.prune_hierarchy_gpu(h, remove=second, stats=st),
            "identity_trim": lambda st: hierarchy.trim_hierarchy_gpu(h, stats=st),
            "torch_box": lambda st: torch_prune(h, lo, hi),
        }
        # the torch statement against the HIP call: records and maps
        r = calls["box_none"]({})
        try:
            nd, old, new_of_old, _ = calls["torch_box"]({})
            assert torch.equal(nd, r.hierarchy.nodes) and torch.equal(old, r.old_of_new) and torch.equal(new_of_old, r.new_of_old)
            del nd, old, new_of_old
        except (RuntimeError, AssertionError) as e:          # said in the output, and the comparator is left out
            print(json.dumps(dict(nodes=N, case="torch_box", not_measured=f"{type(e).__name__}: {str(e)[:200]}")), flush=True)
            del calls["torch_box"]
            torch.cuda.empty_cache()
        del r
        ms = {k: [] for k in calls}
        parts = {k: {"plan_ms": [], "apply_ms": []} for k in calls}
        info = {}
        for rep in range(a.reps + 1):
            for k, fn in calls.items():                   # alternated
                st = {}
                t, out = timed(lambda: fn(st))
                if rep == 0:
                    if k in ("box", "opacity", "second"):
                        info[k] = dict(kept=out.hierarchy.num_nodes, removed_leaves=out.removed_leaves, dead=out.dead,
                                       dirty=out.dirty, single_child=out.single_child, levels=st["levels"])
                    continue
                ms[k].append(t)
                for p in parts[k]:
                    if p in st:
                        parts[k][p].append(st[p])
                del out
        for k in calls:
            line = dict(nodes=N, case=k, reps=a.reps, ms=summary(ms[k]), **info.get(k, {}))
            for p, v in parts[k].items():
                if v:
                    line[p] = summary(v)
            lines.append(line)
            print(json.dumps(line), flush=True)
        del h, second
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
