"""Rotation aligner for an existing hierarchy file: ``<in.hier>`` -> ``<out.hier>``.

    python -m hgs.align_hierarchy <in.hier> <out.hier>

For hierarchies written without ``--align`` (hgs.create_hierarchy, hgs.merge_hierarchies) and for what
``train_post.py`` leaves behind (``hierarchy.hier_opt``: the optimiser moves rotations and scales freely).  Steps:

  1. read the file (load_hierarchy: any of the layouts it accepts);
  2. ``hgs.hierarchy.align_hierarchy_gpu`` on the N node rows: every node's rotation and scales re-parametrised to the
     one of its 24 equivalent frames that lies closest to its parent's; the Gaussians, xyz, shs,
     alpha, nodes and boxes do not change.  Rows behind the node rows (the skybox tail save_hier appends) are carried
     through untouched;
  3. write the result (write_hierarchy).

Printed: the node count, the rows changed, the share of non-root nodes whose normalised quaternion dot with the parent
is below (2 + sqrt 2) / 4 before and after, and the device time of the align call."""
from __future__ import annotations

import dataclasses
import sys

import torch

from ._hier_command import check_exit, missing_path, read_input, upload, usage_exit, write_output

USAGE = "usage: python -m hgs.align_hierarchy <in.hier> <out.hier>"


def run(in_path, out_path) -> dict:
    """Read, align, write; -> figures of the run."""
    from .hierarchy import ALIGN_BOUND, align_hierarchy_gpu, alignment_dots
    host, N, G, read_s = read_input("align_hierarchy", in_path)
    h = upload(host, ("log_scales", "rots", "nodes"))
    stats = {}
    align_hierarchy_gpu(h, stats)
    out = dataclasses.replace(host, log_scales=h.log_scales.cpu(), rots=h.rots.cpu())
    bits = lambda t: t.contiguous().view(torch.int32)
    changed = (bits(out.rots) != bits(host.rots)).any(1) | (bits(out.log_scales) != bits(host.log_scales)).any(1)
    below = lambda x: float((alignment_dots(x) < ALIGN_BOUND).mean()) if N > 1 else 0.0
    write_s = write_output(out_path, out)
    return dict(nodes=N, tail=G - N, changed=int(changed.sum()), below_before=below(host), below_after=below(out),
                align_ms=stats["align_ms"], read_s=read_s, write_s=write_s, path=out_path)


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) != 2 or missing_path("align_hierarchy", argv[0]):
        return usage_exit(USAGE)
    from .hierarchy import HierarchyAlignError
    try:
        r = run(*argv)
    except HierarchyAlignError as e:
        return check_exit("align_hierarchy", f"{argv[0]}: {e}")
    print(f"align_hierarchy: N = {r['nodes']} nodes ({r['tail']} rows behind them carried through), {r['changed']} rows "
          f"changed, below the bound {100 * r['below_before']:.1f} % -> {100 * r['below_after']:.1f} % of the non-root "
          f"nodes, align {r['align_ms']:.2f} ms on the device (read {r['read_s']:.2f} s, write {r['write_s']:.2f} s) -> "
          f"{r['path']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
