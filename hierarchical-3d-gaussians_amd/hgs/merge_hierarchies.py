"""Hierarchy consolidation: every trained chunk's hierarchy -> one ``merged.hier``.

    python -m hgs.merge_hierarchies [--align] <trained chunks dir> <root type> <chunks dir> <output .hier> <chunk name> [...]

The positional form of the reference's consolidation call (scripts/full_train.py:240-250), so only the executable
changes; the output is what ``render_hierarchy.py`` and the viewer load.  Steps:

  1. per chunk name, read ``<trained chunks dir>/<name>/hierarchy.hier_opt`` (what train_post.py writes), else
     ``hierarchy.hier`` (said so in the output);
  2. merge with ``hgs.hierarchy.merge_hierarchies_gpu``: a new root over the chunk roots, every chunk's nodes behind
     them, rows and boxes unchanged.  Rows behind a chunk's N node rows (the scaffold's skybox, appended by save_hier)
     are dropped; render_hierarchy.py / train_post.py append the scaffold's skybox again when they load the result;
  3. with ``--align`` (opt-in, anywhere among the arguments): ``hgs.hierarchy.align_hierarchy_gpu`` on the merged
     hierarchy -- the chunk roots against the new axis-aligned root, and every chunk's nodes below them (DESIGN.md
     section 4).  Without the flag the output is byte for byte what it was before the flag existed;
  4. write the merged hierarchy (write_hierarchy).

Root type 0 (what full_train.py passes) is the only one.  ``<chunks dir>/<name>/center.txt`` / ``extent.txt`` serve a
report only: the leaves whose means lie outside their chunk's square (create_hierarchy.select_rows' float32 test),
having drifted there during post-optimisation.  No pruning or rebalancing.

This project's merge rule, not a restatement of the reference's merger."""
from __future__ import annotations

import os
import sys
import time

import torch

from ._hier_command import check_exit, require_gpu, usage_exit, write_output
from .create_hierarchy import read_chunk_bounds, select_rows, split_flags

USAGE = ("usage: python -m hgs.merge_hierarchies [--align] <trained chunks dir> <root type> <chunks dir> <output .hier> "
         "<chunk name> [<chunk name> ...]")


def chunk_file(trained_dir, name):
    """-> (path, fallback): ``hierarchy.hier_opt`` of the chunk, else ``hierarchy.hier`` (fallback True), else None."""
    d = os.path.join(trained_dir, name)
    for fname, fallback in (("hierarchy.hier_opt", False), ("hierarchy.hier", True)):
        if os.path.exists(os.path.join(d, fname)):
            return os.path.join(d, fname), fallback
    return None, False


def count_drifted(h, node_counts, bounds):
    """Leaves (count_children == 0) of each chunk whose means lie outside the chunk's square, in the merged hierarchy
    ``h``; ``bounds[c]`` = (center, extent) or None (not counted)."""
    from .hierarchy import merge_layout
    bases, _ = merge_layout(node_counts)
    total = 0
    for c, (n, b) in enumerate(zip(node_counts, bounds)):
        if b is None:
            continue
        for lo, hi in ((1 + c, 2 + c), (bases[c], bases[c] + n - 1)):
            leaf = h.nodes[lo:hi, 6] == 0
            xyz = h.xyz[lo:hi][leaf].cpu()
            total += int(xyz.shape[0]) - int(select_rows(xyz, 0, b).numel())
    return total


def run(trained_dir, chunks_dir, out_path, names, align=False) -> dict:
    """Read, merge, (align,) write; -> figures of the run."""
    from .hierarchy import merge_hierarchies_gpu, read_hier_header
    require_gpu("merge_hierarchies")
    paths = [chunk_file(trained_dir, n)[0] for n in names]
    headers = [read_hier_header(p) for p in paths]
    bounds = [read_chunk_bounds(os.path.join(chunks_dir, n)) for n in names]
    dev = torch.device("cuda", torch.cuda.current_device())
    stats = {}
    t0 = time.perf_counter()
    h = merge_hierarchies_gpu(paths, dev, stats, align=align)
    t_merge = time.perf_counter() - t0
    node_counts = [hd[1] for hd in headers]
    drifted = count_drifted(h, node_counts, bounds)
    write_s = write_output(out_path, h)
    return dict(chunks=len(names), nodes=node_counts, merged=h.num_nodes,
                skybox_dropped=sum(hd[0] - hd[1] for hd in headers), drifted=drifted,
                bounded=sum(b is not None for b in bounds), merge_ms=stats["merge_ms"], align_ms=stats.get("align_ms"),
                read_s=stats["read_s"], merge_s=t_merge, write_s=write_s, path=out_path)


def main(argv=None) -> int:
    argv, flags = split_flags(sys.argv[1:] if argv is None else list(argv))
    if len(argv) < 5:
        return usage_exit(USAGE)
    trained_dir, root_type, chunks_dir, out_path, names = argv[0], argv[1], argv[2], argv[3], argv[4:]
    if root_type != "0":
        return usage_exit(USAGE, f"merge_hierarchies: root type {root_type!r} is not supported (0 only, what "
                                 f"full_train.py passes)")
    missing = [n for n in names if chunk_file(trained_dir, n)[0] is None]
    if missing:
        print(f"merge_hierarchies: no hierarchy.hier_opt or hierarchy.hier under {trained_dir} for chunk(s) "
              f"{', '.join(missing)}", file=sys.stderr)
        return 2
    for n in names:
        if chunk_file(trained_dir, n)[1]:
            print(f"merge_hierarchies: {n}: no hierarchy.hier_opt, merging its hierarchy.hier", flush=True)
    from .hierarchy import ChunkValidationError
    try:
        r = run(trained_dir, chunks_dir, out_path, names, align="--align" in flags)
    except ChunkValidationError as e:
        return check_exit("merge_hierarchies", e)
    aligned = f", align {r['align_ms']:.2f} ms" if r["align_ms"] is not None else ""
    print(f"merge_hierarchies: {r['chunks']} chunks of {'/'.join(str(n) for n in r['nodes'])} nodes, merged N = "
          f"{r['merged']} nodes, dropped {r['skybox_dropped']} skybox rows, {r['drifted']} leaves outside their chunk "
          f"({r['bounded']} chunks with bounds), merge {r['merge_ms']:.2f} ms{aligned} on the device (read {r['read_s']:.2f} s, "
          f"write {r['write_s']:.2f} s) -> {r['path']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
