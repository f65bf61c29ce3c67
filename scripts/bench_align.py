#!/usr/bin/env python
"""Rotation-alignment figures, one JSON line per hierarchy:

  builder         hgs.hierarchy.build_hierarchy_gpu output over --leaves leaves of hgs.synth.make_scene (N = 2 P - 1
                  nodes, BFS numbering); build_ms = hipEvents around one build after one warm-up build
  merged          --merged-chunks chunks of hgs.hierarchy.build_hierarchy_on_device joined by merge_hierarchies_gpu to
                  about --merged-nodes nodes (chunks side by side: not level by level), every rotation replaced by a
                  random unit quaternion so that interior rows move too (the generator's interior frames are all the
                  identity); merge_ms = the device time of the merge

per hierarchy: align_ms = hipEvents around one hgs.hierarchy.align_hierarchy_gpu call (the host wait for the level sizes
included) on a fresh copy of the unaligned rows, after one warm-up call on another copy; realign_ms = the same call on
the aligned result (nothing left to write); torch_ms = tests/align_spec.py's torch statement of the rule on the same
GPU, same protocol, and whether it wrote the same bits; rows_changed; below_before / below_after = the share of non-root
nodes whose normalised dot with the parent is below (2 + sqrt 2) / 4.
floor: bytes the passes must move per node at the least -- check 16 (depth, parent, the parent's depth, the key out),
8-bit sort 16 (keys read twice, keys and ids out), level pass 80 (id, parent column, 7 floats in, the parent's
quaternion, 7 floats out) = 112 B -- over the measured float4-copy rate of the HBM, 6.29 TB/s; floor_share = floor_ms /
align_ms.

    python scripts/bench_align.py [--leaves 500000 5000000] [--merged-nodes 50000000] [--merged-chunks 10]
                                  [--out profiles/f13_align_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import align_spec                                   # noqa: E402
from hgs import hierarchy, synth                    # noqa: E402

FLOOR_BYTES_PER_NODE = 16 + 16 + 80
HBM_COPY_BYTES_PER_S = 6.29e12


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def fresh(h, ls, rots):
    return hierarchy.Hierarchy(h.xyz, h.shs, h.alpha, ls.clone(), rots.clone(), h.nodes, h.boxes)


def below(h, chunk=1 << 24):
    """Share of the non-root nodes below the bound, on the device (float64, in slices of the node list)."""
    N = h.num_nodes
    bad = 0
    for a in range(0, N, chunk):
        nd = h.nodes[a:a + chunk]
        q = torch.nn.functional.normalize(h.rots[a:a + chunk].double(), dim=1)
        p = torch.nn.functional.normalize(h.rots[nd[:, 1].clamp_min(0).long()].double(), dim=1)
        bad += int((((q * p).sum(1).abs() < hierarchy.ALIGN_BOUND) & (nd[:, 0] > 0)).sum())
    return bad / max(N - 1, 1)


def align_figures(h):
    ls0, r0 = h.log_scales.clone(), h.rots.clone()
    N = h.num_nodes
    res = dict(nodes=N, levels=int(h.nodes[:, 0].max()) + 1, below_before=round(below(h), 4))
    hierarchy.align_hierarchy_gpu(fresh(h, ls0, r0))                                # warm-up
    a, res["align_ms"] = events(lambda: hierarchy.align_hierarchy_gpu(fresh(h, ls0, r0)))
    # (the two clones inside the timed window copy 28 B per node: subtracted below from a timing of their own)
    _, clone_ms = events(lambda: fresh(h, ls0, r0))
    res["align_ms"] = round(res["align_ms"] - clone_ms, 3)
    _, realign_ms = events(lambda: hierarchy.align_hierarchy_gpu(a))
    res["realign_ms"] = round(realign_ms, 3)
    changed = ((a.rots.view(torch.int32) != r0.view(torch.int32)).any(1) |
               (a.log_scales.view(torch.int32) != ls0.view(torch.int32)).any(1))
    res["rows_changed"] = int(changed[:N].sum())
    res["below_after"] = round(below(a), 4)
    try:
        align_spec.align_torch(fresh(h, ls0, r0))                                   # warm-up
        t, torch_ms = events(lambda: align_spec.align_torch(fresh(h, ls0, r0)))
        res["torch_ms"] = round(torch_ms - clone_ms, 3)
        res["torch_same_bits"] = bool(torch.equal(t.rots.view(torch.int32), a.rots.view(torch.int32)) and
                                      torch.equal(t.log_scales.view(torch.int32), a.log_scales.view(torch.int32)))
        del t
    except torch.cuda.OutOfMemoryError:             # 24 float64 candidates per node of the widest level
        res["torch_ms"] = res["torch_same_bits"] = None
    torch.cuda.empty_cache()
    floor_ms = N * FLOOR_BYTES_PER_NODE / HBM_COPY_BYTES_PER_S * 1e3
    res["floor_ms"] = round(floor_ms, 3)
    res["floor_share"] = round(floor_ms / res["align_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, nargs="*", default=[500_000, 5_000_000])
    ap.add_argument("--merged-nodes", type=int, default=50_000_000)
    ap.add_argument("--merged-chunks", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cam = synth.make_camera(1920, 1080)
    lines = []

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(dev)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for P in args.leaves:
        sc = synth.make_scene(P, cam, seed=1).to(dev)
        hierarchy.build_hierarchy_gpu(sc, dev)
        h, build_ms = events(lambda: hierarchy.build_hierarchy_gpu(sc, dev))
        del sc
        emit(dict(kind="builder", leaves=P, build_ms=round(build_ms, 3), **align_figures(h)))
        del h
        torch.cuda.empty_cache()
    if args.merged_nodes > 0:
        k = args.merged_chunks
        P = (args.merged_nodes // k + 1) // 2
        chunks = [hierarchy.build_hierarchy_on_device(P, cam, dev, seed=i) for i in range(k)]
        stats = {}
        h = hierarchy.merge_hierarchies_gpu(chunks, dev, stats)
        del chunks
        torch.cuda.empty_cache()
        g = torch.Generator(device=dev).manual_seed(7)
        h.rots[1:] = torch.nn.functional.normalize(torch.randn(h.num_nodes - 1, 4, generator=g, device=dev), dim=1)
        emit(dict(kind="merged", chunks=k, merge_ms=round(stats["merge_ms"], 3), **align_figures(h)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
