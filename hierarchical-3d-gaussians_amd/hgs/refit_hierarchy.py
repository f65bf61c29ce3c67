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

import os
import shutil
import sys
import time

import torch

USAGE = "usage: python -m hgs.refit_hierarchy <in.hier> <out.hier> [--leaf cube|ellipsoid|keep] [--half]"
SIDE_FILES = ("anchors.bin", "exposure.json")
LEAF_MODES = ("cube", "ellipsoid", "keep")


def parse_args(argv):
    """-> (in_path, out_path, leaf, half) or None for a usage error."""
    pos, leaf, half = [], "cube", False
    i = 0
    while i < len(argv):
        a = argv[i]
        if a == "--leaf":
            if i + 1 >= len(argv) or argv[i + 1] not in LEAF_MODES:
                return None
            leaf, i = argv[i + 1], i + 2
        elif a == "--half":
            half, i = True, i + 1
        elif a.startswith("--"):
            return None
        else:
            pos.append(a)
            i += 1
    if len(pos) != 2:
        return None
    return pos[0], pos[1], leaf, half


def run(in_path, out_path, leaf="cube", half=False) -> dict:
    """Read, refit, write; -> figures of the run."""
    from gaussian_hierarchy._C import _boxes_nested, load_hierarchy, write_hierarchy
    from .hierarchy import Hierarchy, refit_boxes_gpu
    if not torch.cuda.is_available():
        raise RuntimeError("hgs.refit_hierarchy refits on the GPU; no GPU is visible")
    t0 = time.perf_counter()
    host = Hierarchy(*load_hierarchy(in_path))
    t_read = time.perf_counter() - t0
    N, G = host.num_nodes, int(host.xyz.shape[0])
    if N < 1 or G < N:
        raise ValueError(f"{in_path}: G = {G} rows, N = {N} nodes; 1 <= N <= G expected")
    dev = torch.device("cuda", torch.cuda.current_device())
    names = ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes")
    h = Hierarchy(*(getattr(host, k).to(dev).contiguous() for k in names))
    nested_in = _boxes_nested(h.nodes, h.boxes)
    stats = {}
    refit_boxes_gpu(h, leaf, inplace=True, stats=stats)
    nested_out = _boxes_nested(h.nodes, h.boxes)
    t1 = time.perf_counter()
    out_dir = os.path.dirname(os.path.abspath(out_path))
    os.makedirs(out_dir, exist_ok=True)
    write_hierarchy(out_path, *(getattr(host, k) for k in names[:6]), h.boxes.cpu(), half=half)
    in_dir = os.path.dirname(os.path.abspath(in_path))
    beside = [f for f in SIDE_FILES if os.path.exists(os.path.join(in_dir, f))]
    for f in beside:
        if in_dir != out_dir:
            shutil.copyfile(os.path.join(in_dir, f), os.path.join(out_dir, f))
    return dict(nodes=N, tail=G - N, leaf=leaf, levels=stats["levels"], leaves=stats["leaves"], nested_in=nested_in,
                nested_out=nested_out, refit_ms=stats["refit_ms"], read_s=t_read, write_s=time.perf_counter() - t1,
                beside=beside, same_dir=in_dir == out_dir, path=out_path)


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    parsed = parse_args(argv)
    if parsed is None:
        print(USAGE, file=sys.stderr)
        return 2
    if not os.path.exists(parsed[0]):
        print(f"refit_hierarchy: {parsed[0]} does not exist\n{USAGE}", file=sys.stderr)
        return 2
    from .hierarchy import HierarchyRefitError
    try:
        r = run(*parsed)
    except HierarchyRefitError as e:
        print(f"refit_hierarchy: {parsed[0]}: {e.check} (node {e.node}): {e}; nothing written", file=sys.stderr)
        return 1
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
