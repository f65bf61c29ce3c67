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

import os
import sys
import time

import torch

USAGE = "usage: python -m hgs.align_hierarchy <in.hier> <out.hier>"


def run(in_path, out_path) -> dict:
    """Read, align, write; -> figures of the run."""
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from .hierarchy import ALIGN_BOUND, Hierarchy, align_hierarchy_gpu, alignment_dots
    if not torch.cuda.is_available():
        raise RuntimeError("hgs.align_hierarchy aligns on the GPU; no GPU is visible")
    t0 = time.perf_counter()
    host = Hierarchy(*load_hierarchy(in_path))
    t_read = time.perf_counter() - t0
    N = host.num_nodes
    if N < 1 or host.xyz.shape[0] < N:
        raise ValueError(f"{in_path}: G = {host.xyz.shape[0]} rows, N = {N} nodes; 1 <= N <= G expected")
    dev = torch.device("cuda", torch.cuda.current_device())
    h = Hierarchy(host.xyz, host.shs, host.alpha, host.log_scales.to(dev), host.rots.to(dev), host.nodes.to(dev),
                  host.boxes)
    stats = {}
    align_hierarchy_gpu(h, stats)
    out = Hierarchy(host.xyz, host.shs, host.alpha, h.log_scales.cpu(), h.rots.cpu(), host.nodes, host.boxes)
    bits = lambda t: t.contiguous().view(torch.int32)
    changed = (bits(out.rots) != bits(host.rots)).any(1) | (bits(out.log_scales) != bits(host.log_scales)).any(1)
    below = lambda x: float((alignment_dots(x) < ALIGN_BOUND).mean()) if N > 1 else 0.0
    t1 = time.perf_counter()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    write_hierarchy(out_path, out.xyz, out.shs, out.alpha, out.log_scales, out.rots, out.nodes, out.boxes)
    return dict(nodes=N, tail=int(host.xyz.shape[0]) - N, changed=int(changed.sum()), below_before=below(host),
                below_after=below(out), align_ms=stats["align_ms"], read_s=t_read, write_s=time.perf_counter() - t1,
                path=out_path)


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) != 2:
        print(USAGE, file=sys.stderr)
        return 2
    if not os.path.exists(argv[0]):
        print(f"align_hierarchy: {argv[0]} does not exist\n{USAGE}", file=sys.stderr)
        return 2
    from .hierarchy import HierarchyAlignError
    try:
        r = run(*argv)
    except HierarchyAlignError as e:
        print(f"align_hierarchy: {argv[0]}: {e}; nothing written", file=sys.stderr)
        return 1
    print(f"align_hierarchy: N = {r['nodes']} nodes ({r['tail']} rows behind them carried through), {r['changed']} rows "
          f"changed, below the bound {100 * r['below_before']:.1f} % -> {100 * r['below_after']:.1f} % of the non-root "
          f"nodes, align {r['align_ms']:.2f} ms on the device (read {r['read_s']:.2f} s, write {r['write_s']:.2f} s) -> "
          f"{r['path']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
