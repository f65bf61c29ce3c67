#!/usr/bin/env python
"""Hierarchy trimming figures, one JSON line per (size, mode):

  hierarchies     hgs.hierarchy.build_hierarchy_on_device, --sizes nodes each (16 SH coefficients: 296 bytes per node)
  modes           floor: the median extent of the nodes with children (about half of the nodes stay); region: a box
                  about the root box's centre, its size bisected until about a tenth of the nodes stay; identity
  hip             hgs.hierarchy.trim_hierarchy_gpu (hgs_hier_trim_plan, the allocation, hgs_hier_trim_apply)
  torch           this project's torch statement of the same rule on the same GPU (torch_trim below): a boolean mask, a
                  cumulative sum, index_select per tensor, the node rewrite; without the four checks the HIP call makes
  each            --reps alternated repetitions after one warm-up call of each, device events around the call: median,
                  min and max; the peak device memory of one call above what was allocated before it (the input not
                  counted, the outputs counted).  The outputs of the two are compared bit for bit before anything is timed.
  floor_ms        the bytes the apply step cannot avoid -- the kept rows read and written, 60 bytes of node record and
                  box per node scanned -- at 8 TB/s; apply_share = floor_ms / the median apply_ms of the HIP call

    python scripts/bench_trim.py [--sizes 1000000 10000000 50000000] [--reps 15] [--out profiles/f17_trim_bench.jsonl]"""
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
PEAK_BYTES_PER_MS = 8.0e9           # 8 TB/s


def node_test(boxes, e, roi):
    t = boxes[:, 0, 3] >= e
    if roi is not None:
        lo, hi = roi
        t = t & (boxes[:, 0, :3] <= hi).all(1) & (boxes[:, 1, :3] >= lo).all(1)
    return t


def torch_trim(h, e, roi):
    """The rule in torch ops -> (Hierarchy, old_of_new int32, new_of_old int32)."""
    nodes, boxes = h.nodes, h.boxes
    test = node_test(boxes, e, roi)
    keep = test[nodes[:, 1].clamp_min(0).long()]
    keep[0] = True
    new_of_old = torch.where(keep, torch.cumsum(keep, 0, dtype=torch.int32) - 1, -1).to(torch.int32)
    old = keep.nonzero().flatten()
    rows = [getattr(h, k).index_select(0, old) for k in ARRAYS[:5]]
    nd = nodes.index_select(0, old)
    cc = nd[:, 6]
    own = test.index_select(0, old)
    stub, inner = (cc > 0) & ~own, (cc > 0) & own
    nd[:, 1] = torch.where(old == 0, -1, new_of_old[nd[:, 1].clamp_min(0).long()])
    nd[:, 2] = torch.arange(old.numel(), dtype=torch.int32, device=old.device)
    nd[:, 5] = torch.where(inner, new_of_old[nd[:, 5].long()], nd[:, 5])
    leaf = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=old.device)
    nd[:, 3:7] = torch.where(stub[:, None], leaf, nd[:, 3:7])
    return hierarchy.Hierarchy(*rows, nd, boxes.index_select(0, old)), old.to(torch.int32), new_of_old


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


def region_for(h, share):
    """A box about the root box's centre whose size is bisected until about `share` of the nodes stay."""
    lo, hi = h.boxes[0, 0, :3], h.boxes[0, 1, :3]
    c, half = (lo + hi) / 2, (hi - lo) / 2
    parent = h.nodes[:, 1].clamp_min(0).long()
    a, b = 0.0, 1.0
    for _ in range(16):
        f = (a + b) / 2
        kept = int(node_test(h.boxes, float("-inf"), (c - f * half, c + f * half))[parent].sum())
        a, b = (f, b) if kept < share * h.num_nodes else (a, f)
    f = (a + b) / 2
    return (c - f * half).cpu().numpy(), (c + f * half).cpu().numpy()


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def figures(h, mode, e, roi, reps, dev):
    roi_dev = None if roi is None else tuple(torch.from_numpy(r).to(dev) for r in roi)
    hip = lambda st=None: hierarchy.trim_hierarchy_gpu(h, e, roi, stats=st)
    ref = lambda: torch_trim(h, e, roi_dev)
    # ---- warm-up of each, and the comparison
    r, (th, old, new) = hip(), ref()
    for k in ARRAYS:
        assert torch.equal(getattr(r.hierarchy, k).view(torch.int32), getattr(th, k).view(torch.int32)), (mode, k)
    assert torch.equal(r.old_of_new, old) and torch.equal(r.new_of_old, new), mode
    kept, stubs, M = r.hierarchy.num_nodes, r.stubs, int(h.shs.shape[1])
    del r, th, old, new
    hip_ms, ref_ms, plan_ms, apply_ms, hip_peak, ref_peak = [], [], [], [], 0, 0
    for _ in range(reps):                       # alternated
        st = {}
        out, ms, peak = timed(lambda: hip(st), dev)
        del out
        hip_ms.append(ms); plan_ms.append(st["plan_ms"]); apply_ms.append(st["apply_ms"]); hip_peak = max(hip_peak, peak)
        out, ms, peak = timed(ref, dev)
        del out
        ref_ms.append(ms); ref_peak = max(ref_peak, peak)
    row = 12 * M + 104                          # attributes, node record, box
    floor_ms = (2 * kept * row + 60 * h.num_nodes) / PEAK_BYTES_PER_MS
    return dict(nodes=h.num_nodes, mode=mode, kept=kept, stubs=stubs, min_extent=e, hip_ms=summary(hip_ms),
                plan_ms=summary(plan_ms), apply_ms=summary(apply_ms), torch_ms=summary(ref_ms),
                ranges_apart=max(hip_ms) < min(ref_ms), speedup=round(statistics.median(ref_ms) / statistics.median(hip_ms), 2),
                hip_peak_mb=round(hip_peak / 2**20, 1), torch_peak_mb=round(ref_peak / 2**20, 1),
                out_mb=round((kept * (row + 4) + 4 * h.num_nodes) / 2**20, 1), floor_ms=round(floor_ms, 3),
                apply_share=round(floor_ms / statistics.median(apply_ms), 3), reps=reps)


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
        inner = h.boxes[:, 0, 3][h.nodes[:, 6] > 0]
        med = float(inner.median()) if inner.numel() else 0.0
        roi = region_for(h, 0.1)
        for mode, e, r in (("floor", med, None), ("region", 0.0, roi), ("identity", 0.0, None)):
            res = figures(h, mode, e, r, args.reps, dev)
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
