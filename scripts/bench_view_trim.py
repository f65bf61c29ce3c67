#!/usr/bin/env python
"""View-dependent trimming figures, one JSON line per (size, views):

  hierarchies     hgs.hierarchy.build_hierarchy_on_device, --sizes nodes each (16 SH coefficients: 296 bytes per node)
  views           --views point views on a straight path through the scene: along x through the centre of the root box,
                  from one face to the other; tau = the renderer's granularity for --tau-px pixels at this camera
  hip             hgs.hierarchy.trim_to_views_gpu (hgs_hier_reach, hgs_hier_trim_plan_keyed, the allocation,
                  hgs_hier_trim_apply)
  torch           this project's torch statement of the same rule on the same GPU: d2 over region chunks with a running
                  minimum (torch_reach below), then bench_trim.py's torch statement on the keyed test; no checks
  each            --reps alternated repetitions after one warm-up call of each, device events around the whole call:
                  median, min and max.  The reach and the outputs of the two are compared bit for bit before anything is
                  timed: reach_bits_differ counts the nodes whose reach differs (torch's own sqrt and division decide
                  that), outputs_equal says whether all seven tensors and the map agree; equal reach with unequal
                  outputs stops the run.
  valu_share      pairs x the reach kernel's vector instructions per pair (13.5: the unrolled loop in the ISA), in wave64
                  instructions, over the median reach_ms, over the issue rate scripts/microbench/valu_issue.hip measured
                  (v_fma_f32 at 8 waves per SIMD: 891.7 G wave-instructions/s)

    python scripts/bench_view_trim.py [--sizes 1000000 10000000 50000000] [--views 64 1024 4096] [--reps 15]
                                      [--out profiles/f20_view_trim_bench.jsonl]"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_trim import ARRAYS, summary, timed   # noqa: E402
from hgs import hierarchy, synth   # noqa: E402

VALU_PER_PAIR = 13.5                 # 6 sub, 3 max3, 1 mul + 1 pk_mul, 2 add, half a min3
VALU_WAVE_INST_PER_MS = 891.7e6      # profiles/r02_microbench_valu_issue.txt
FLT_MAX = 3.4028234663852886e38
CHUNK_PAIRS = 1 << 28                # (node, region) pairs per chunk of the torch statement: 1 GiB per float temporary


def torch_reach(boxes, lo, hi):
    """The rule in torch ops -> float32 [N].  (torch does not contract across ops: the device's operation order.)"""
    mn, mx, ext = boxes[:, None, 0, :3], boxes[:, None, 1, :3], boxes[:, 0, 3]
    N, step = boxes.shape[0], max(1, CHUNK_PAIRS // boxes.shape[0])
    best = torch.full((N,), float("inf"), device=boxes.device)
    zero = torch.zeros((), device=boxes.device)
    for c0 in range(0, lo.shape[0], step):
        d = torch.fmax(torch.fmax(mn - hi[None, c0:c0 + step], lo[None, c0:c0 + step] - mx), zero)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        best = torch.fmin(best, d2.min(1).values)
    return torch.where(best > 0, ext / best.sqrt(), torch.full_like(best, FLT_MAX))


def torch_view_trim(h, lo, hi, tau):
    """reach, then the trim rule of bench_trim.torch_trim on test = reach >= tau."""
    nodes, boxes = h.nodes, h.boxes
    test = torch_reach(boxes, lo, hi) >= tau
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


def path_through(h, count):
    """``count`` point views along x through the centre of the root box, face to face."""
    mn, mx = h.boxes[0, 0, :3].cpu().numpy().astype(np.float64), h.boxes[0, 1, :3].cpu().numpy().astype(np.float64)
    c = (mn + mx) / 2
    return hierarchy.view_regions(points=[(x, c[1], c[2]) for x in np.linspace(mn[0], mx[0], count)])


def figures(h, regions, tau, reps, dev):
    lo, hi = (torch.from_numpy(r).to(dev) for r in regions)
    hip = lambda st=None: hierarchy.trim_to_views_gpu(h, regions, tau, stats=st)
    ref = lambda: torch_view_trim(h, lo, hi, float(np.float32(tau)))
    # ---- warm-up of each, and the comparison
    differ = int((hierarchy.view_reach_gpu(h, regions).view(torch.int32) != torch_reach(h.boxes, lo, hi).view(torch.int32)).sum())
    r, (th, old, new) = hip(), ref()
    same = r.hierarchy.num_nodes == th.num_nodes and torch.equal(r.new_of_old, new) and all(
        torch.equal(getattr(r.hierarchy, k).view(torch.int32), getattr(th, k).view(torch.int32)) for k in ARRAYS)
    assert same or differ, "the torch statement's reach has the HIP call's bits, its trim has not"
    kept, stubs = r.hierarchy.num_nodes, r.stubs
    del r, th, old, new
    hip_ms, ref_ms, parts = [], [], dict(reach_ms=[], plan_ms=[], apply_ms=[])
    for _ in range(reps):                       # alternated
        st = {}
        out, ms, _ = timed(lambda: hip(st), dev)
        del out
        hip_ms.append(ms)
        for k in parts:
            parts[k].append(st[k])
        out, ms, _ = timed(ref, dev)
        del out
        ref_ms.append(ms)
    pairs = h.num_nodes * regions[0].shape[0]
    share = pairs / 64 * VALU_PER_PAIR / statistics.median(parts["reach_ms"]) / VALU_WAVE_INST_PER_MS
    return dict(nodes=h.num_nodes, views=int(regions[0].shape[0]), tau=float(np.float32(tau)), kept=kept, stubs=stubs,
                hip_ms=summary(hip_ms), **{k: summary(v) for k, v in parts.items()}, torch_ms=summary(ref_ms),
                ranges_apart=max(hip_ms) < min(ref_ms), speedup=round(statistics.median(ref_ms) / statistics.median(hip_ms), 2),
                valu_share=round(share, 3), reach_bits_differ=differ, outputs_equal=bool(same), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 10_000_000, 50_000_000])
    ap.add_argument("--views", type=int, nargs="*", default=[64, 1024, 4096])
    ap.add_argument("--tau-px", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    width, height = 1920, 1080
    cam = synth.make_camera(width, height)
    tanfovx = width / (2.0 * (height / (2.0 * math.tan(math.radians(60.0) / 2))))
    tau = (2.0 * (args.tau_px + 0.5)) * tanfovx / (0.5 * width)
    for n in args.sizes:
        h = hierarchy.build_hierarchy_on_device((n + 1) // 2, cam, dev, seed=1)
        for count in args.views:
            res = figures(h, path_through(h, count), tau, args.reps, dev)
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
