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

import sys

from ._hier_command import (check_exit, missing_path, read_input, side_files_beside, upload, usage_exit, walk_args,
                            with_tail, write_output)

USAGE = ("usage: python -m hgs.trim_hierarchy <in.hier> <out.hier> [--min-extent E] [--max-nodes K] "
         "[--roi x0 y0 z0 x1 y1 z1]   (at least one option)")
OPTIONS = {"--min-extent": 1, "--max-nodes": 1, "--roi": 6}


def parse_args(argv):
    """-> (in_path, out_path, min_extent, max_nodes, roi) or None for a usage error (no option at all included).  The
    last occurrence of an option wins."""
    walked = walk_args(argv, OPTIONS)
    if walked is None:
        return None
    pos, seen = walked
    # every occurrence is converted (a bad one is a usage error even when a later one replaces it); absent: None(s)
    last = lambda name, conv: ([[conv(x) for x in vals] for vals in seen[name]] or [[None] * OPTIONS[name]])[-1]
    try:
        (min_extent,), (max_nodes,), roi = last("--min-extent", float), last("--max-nodes", int), last("--roi", float)
    except ValueError:
        return None
    roi = None if roi[0] is None else (tuple(roi[:3]), tuple(roi[3:]))
    if len(pos) != 2 or (min_extent is None and max_nodes is None and roi is None):
        return None
    if (min_extent is not None and min_extent != min_extent) or (max_nodes is not None and max_nodes < 1):
        return None
    if roi is not None and any(x != x for r in roi for x in r):
        return None
    return pos[0], pos[1], 0.0 if min_extent is None else min_extent, max_nodes, roi


def run(in_path, out_path, min_extent=0.0, max_nodes=None, roi=None) -> dict:
    """Read, trim, write; -> figures of the run."""
    from .hierarchy import trim_hierarchy_gpu
    host, N, G, read_s = read_input("trim_hierarchy", in_path)
    stats = {}
    r = trim_hierarchy_gpu(upload(host, rows=N), min_extent, roi, max_nodes, stats)
    write_s = write_output(out_path, with_tail(r.hierarchy, host, N) + [r.hierarchy.nodes, r.hierarchy.boxes])
    return dict(nodes=N, kept=r.hierarchy.num_nodes, stubs=r.stubs, min_extent=r.min_extent, tail=G - N,
                trim_ms=stats["trim_ms"], read_s=read_s, write_s=write_s, beside=side_files_beside(in_path),
                path=out_path)


def main(argv=None) -> int:
    parsed = parse_args(sys.argv[1:] if argv is None else list(argv))
    if parsed is None or missing_path("trim_hierarchy", parsed[0]):
        return usage_exit(USAGE)
    from .hierarchy import HierarchyTrimError
    try:
        r = run(*parsed)
    except HierarchyTrimError as e:
        return check_exit("trim_hierarchy", f"{parsed[0]}: {e.check} (node {e.node}): {e}")
    print(f"trim_hierarchy: N = {r['nodes']} -> {r['kept']} nodes ({r['stubs']} stubs), min_extent {r['min_extent']:.9g} "
          f"used, {r['tail']} rows behind the nodes carried through, trim {r['trim_ms']:.2f} ms on the device (read "
          f"{r['read_s']:.2f} s, write {r['write_s']:.2f} s) -> {r['path']}", flush=True)
    for f in r["beside"]:
        print(f"trim_hierarchy: {f} beside the input is not copied or remapped", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
