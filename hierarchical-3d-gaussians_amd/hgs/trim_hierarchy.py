"""Trimmer for an existing hierarchy file: ``<in.hier>`` -> a smaller ``<out.hier>``.

    python -m hgs.trim_hierarchy <in.hier> <out.hier> [--min-extent E] [--max-nodes K] [--roi x0 y0 z0 x1 y1 z1]

A detail floor (nodes whose parent's extent is below E go), a node budget (the floor at which at most K nodes stay) and
a region (nodes whose parent's box misses the closed box go), alone or together; at least one option is required.  Steps:

  1. read the file (load_hierarchy: any of the layouts it accepts);
  2. ``hgs.hierarchy.trim_hierarchy_gpu`` on the N node rows: the N' kept nodes in their old order,
     rows and boxes bit for bit, node records renumbered, kept nodes that lost their children turned into leaves
     (stubs).  Rows behind the node rows (the skybox tail save_hier appends) are carried through unchanged, behind the
     N' kept rows;
  3. write the result (write_hierarchy).

Printed: N -> N' and the stub count, the floor that was used, the tail rows carried, the device time, read and write
seconds.  A hierarchy that fails a check is named with the check and the node, nothing is written, exit status 1.
``anchors.bin`` and ``exposure.json`` beside the input are neither copied nor remapped (said so when they exist)."""
from __future__ import annotations

import os
import sys
import time

import torch

USAGE = ("usage: python -m hgs.trim_hierarchy <in.hier> <out.hier> [--min-extent E] [--max-nodes K] "
         "[--roi x0 y0 z0 x1 y1 z1]   (at least one option)")
SIDE_FILES = ("anchors.bin", "exposure.json")


def parse_args(argv):
    """-> (in_path, out_path, min_extent, max_nodes, roi) or None for a usage error (no option at all included)."""
    pos, min_extent, max_nodes, roi = [], None, None, None
    i = 0
    try:
        while i < len(argv):
            a = argv[i]
            if a == "--min-extent":
                min_extent = float(argv[i + 1])
                i += 2
            elif a == "--max-nodes":
                max_nodes = int(argv[i + 1])
                i += 2
            elif a == "--roi":
                vals = argv[i + 1:i + 7]
                if len(vals) != 6:
                    return None
                v = [float(x) for x in vals]
                roi = (tuple(v[:3]), tuple(v[3:]))
                i += 7
            elif a.startswith("--"):
                return None
            else:
                pos.append(a)
                i += 1
    except (IndexError, ValueError):
        return None
    if len(pos) != 2 or (min_extent is None and max_nodes is None and roi is None):
        return None
    if (min_extent is not None and min_extent != min_extent) or (max_nodes is not None and max_nodes < 1):
        return None
    if roi is not None and any(x != x for r in roi for x in r):
        return None
    return pos[0], pos[1], 0.0 if min_extent is None else min_extent, max_nodes, roi


def run(in_path, out_path, min_extent=0.0, max_nodes=None, roi=None) -> dict:
    """Read, trim, write; -> figures of the run."""
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from .hierarchy import Hierarchy, trim_hierarchy_gpu
    if not torch.cuda.is_available():
        raise RuntimeError("hgs.trim_hierarchy trims on the GPU; no GPU is visible")
    t0 = time.perf_counter()
    host = Hierarchy(*load_hierarchy(in_path))
    t_read = time.perf_counter() - t0
    N, G = host.num_nodes, int(host.xyz.shape[0])
    if N < 1 or G < N:
        raise ValueError(f"{in_path}: G = {G} rows, N = {N} nodes; 1 <= N <= G expected")
    dev = torch.device("cuda", torch.cuda.current_device())
    names = ("xyz", "shs", "alpha", "log_scales", "rots")
    h = Hierarchy(*(getattr(host, k)[:N].to(dev).contiguous() for k in names), host.nodes.to(dev).contiguous(),
                  host.boxes.to(dev).contiguous())
    stats = {}
    r = trim_hierarchy_gpu(h, min_extent, roi, max_nodes, stats)
    rows = [torch.cat([getattr(r.hierarchy, k).cpu(), getattr(host, k)[N:]]) for k in names]
    t1 = time.perf_counter()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    write_hierarchy(out_path, *rows, r.hierarchy.nodes.cpu(), r.hierarchy.boxes.cpu())
    beside = [f for f in SIDE_FILES if os.path.exists(os.path.join(os.path.dirname(os.path.abspath(in_path)), f))]
    return dict(nodes=N, kept=r.hierarchy.num_nodes, stubs=r.stubs, min_extent=r.min_extent, tail=G - N,
                trim_ms=stats["trim_ms"], read_s=t_read, write_s=time.perf_counter() - t1, beside=beside, path=out_path)


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    parsed = parse_args(argv)
    if parsed is None:
        print(USAGE, file=sys.stderr)
        return 2
    if not os.path.exists(parsed[0]):
        print(f"trim_hierarchy: {parsed[0]} does not exist\n{USAGE}", file=sys.stderr)
        return 2
    from .hierarchy import HierarchyTrimError
    try:
        r = run(*parsed)
    except HierarchyTrimError as e:
        print(f"trim_hierarchy: {parsed[0]}: {e.check} (node {e.node}): {e}; nothing written", file=sys.stderr)
        return 1
    print(f"trim_hierarchy: N = {r['nodes']} -> {r['kept']} nodes ({r['stubs']} stubs), min_extent {r['min_extent']:.9g} "
          f"used, {r['tail']} rows behind the nodes carried through, trim {r['trim_ms']:.2f} ms on the device (read "
          f"{r['read_s']:.2f} s, write {r['write_s']:.2f} s) -> {r['path']}", flush=True)
    for f in r["beside"]:
        print(f"trim_hierarchy: {f} beside the input is not copied or remapped", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
