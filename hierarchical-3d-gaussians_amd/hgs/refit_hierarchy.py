"""Box refit for an existing hierarchy file: ``<in.hier>`` -> ``<out.hier>`` with every box derived again from the rows.

    python -m hgs.refit_hierarchy <in.hier> <out.hier> [--leaf cube|ellipsoid|keep] [--half]

For a hierarchy whose rows moved after its boxes were made (``train_post.py`` writes the optimised rows back with the
boxes it loaded), whose boxes grew under a general rotation (``python -m hgs.transform_hierarchy``), or whose boxes do
not nest (the budgeted and the multi-view cut refuse it, the plain cut walks it level by level).  Steps:

  1. read the file (load_hierarchy: any of the layouts it accepts);
  2. ``hgs.hierarchy.refit_boxes_gpu`` in place on the device: a leaf gets the cube of 3 times its
     largest scale around its mean (``--leaf cube``, the default: the builder's rule), the box of its 3 sigma ellipsoid
     (``--leaf ellipsoid``) or keeps its box (``--leaf keep``); every node with children gets the union of its
     children's boxes, children first.  No row and no node record changes; rows behind the node rows (the skybox tail)
     are not touched;
  3. write the result (write_hierarchy; ``--half``: its half-precision variant).

Printed: N, the level and leaf counts, whether the input's boxes nested and that the output's do, the device time, read
and write seconds.  A hierarchy that fails a check is named with the check and the node, nothing is written, exit
status 1.  ``anchors.bin`` and ``exposure.json`` beside the input hold indices and per-image data, which new boxes do
not touch: they are copied beside the output (said so when they exist)."""
from __future__ import annotations

import dataclasses
import sys

from ._hier_command import (carry_side_files, check_exit, missing_path, read_input, upload, usage_exit, walk_args,
                            write_output)

USAGE = "usage: python -m hgs.refit_hierarchy <in.hier> <out.hier> [--leaf cube|ellipsoid|keep] [--half]"
LEAF_MODES = ("cube", "ellipsoid", "keep")
OPTIONS = {"--leaf": 1, "--half": 0}


def parse_args(argv):
    """-> (in_path, out_path, leaf, half) or None for a usage error.  The last --leaf wins."""
    walked = walk_args(argv, OPTIONS)
    if walked is None:
        return None
    pos, seen = walked
    leaves = [v[0] for v in seen["--leaf"]]
    if len(pos) != 2 or any(v not in LEAF_MODES for v in leaves):
        return None
    return pos[0], pos[1], leaves[-1] if leaves else "cube", bool(seen["--half"])


def run(in_path, out_path, leaf="cube", half=False) -> dict:
    """Read, refit, write; -> figures of the run."""
    from gaussian_hierarchy._C import _boxes_nested
    from .hierarchy import refit_boxes_gpu
    host, N, G, read_s = read_input("refit_hierarchy", in_path)
    h = upload(host)
    nested_in = _boxes_nested(h.nodes, h.boxes)
    stats = {}
    refit_boxes_gpu(h, leaf, inplace=True, stats=stats)
    nested_out = _boxes_nested(h.nodes, h.boxes)
    write_s = write_output(out_path, dataclasses.replace(host, boxes=h.boxes), half)
    beside, same_dir = carry_side_files(in_path, out_path)
    return dict(nodes=N, tail=G - N, leaf=leaf, levels=stats["levels"], leaves=stats["leaves"], nested_in=nested_in,
                nested_out=nested_out, refit_ms=stats["refit_ms"], read_s=read_s, write_s=write_s, beside=beside,
                same_dir=same_dir, path=out_path)


def main(argv=None) -> int:
    parsed = parse_args(sys.argv[1:] if argv is None else list(argv))
    if parsed is None or missing_path("refit_hierarchy", parsed[0]):
        return usage_exit(USAGE)
    from .hierarchy import HierarchyRefitError
    try:
        r = run(*parsed)
    except HierarchyRefitError as e:
        return check_exit("refit_hierarchy", f"{parsed[0]}: {e.check} (node {e.node}): {e}")
    yes = lambda b: "nested" if b else "did NOT nest"
    print(f"refit_hierarchy: N = {r['nodes']} nodes on {r['levels']} levels, {r['leaves']} leaves (--leaf {r['leaf']}), "
          f"{r['tail']} rows behind the nodes left alone; the input's boxes {yes(r['nested_in'])}, the output's "
          f"{'nest' if r['nested_out'] else 'do NOT nest'}; refit {r['refit_ms']:.2f} ms on the device (read "
          f"{r['read_s']:.2f} s, write {r['write_s']:.2f} s) -> {r['path']}", flush=True)
    for f in r["beside"]:
        how = "stays valid beside the output" if r["same_dir"] else "copied beside the output"
        print(f"refit_hierarchy: {f} holds indices / per-image data, which new boxes do not touch: {how}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
