"""Leaf removal for an existing hierarchy file: ``<in.hier>`` -> ``<out.hier>`` without the removed leaves.

    python -m hgs.prune_hierarchy <in.hier> <out.hier> [--remove-box x0 y0 z0 x1 y1 z1]... [--keep-box x0 y0 z0 x1 y1 z1]
                                  [--min-opacity A] [--max-scale S] [--mask <file.npy>] [--remerge dirty|all|none]
                                  [--align] [--half]

Crop a scene to a site boundary, delete a floater or a parked car: a leaf goes when its mean lies in one of up to 16
closed ``--remove-box``es, outside the ``--keep-box``, when its opacity is below A, when one of its scales exceeds S, or
when ``--mask`` (a ``.npy`` array with one entry per node) is nonzero at it; at least one criterion is required.  This
project's own rule ("Removing leaves (f-21)").  Steps:

  1. read the file (load_hierarchy: any of the layouts it accepts);
  2. ``hgs.hierarchy.prune_hierarchy_gpu`` on the N node rows: nodes all of whose leaves went are dropped, the N' others
     keep their order, records renumbered; the ancestors of what went get the union of their surviving children's boxes
     and, by ``--remerge``, a re-merged row (``dirty``, the default: only they; ``all``: every node with children;
     ``none``: no row changes); everything else is copied bit for bit.  Rows behind the node rows (the skybox tail
     save_hier appends) are carried through unchanged, behind the N' rows.  ``--align`` then re-expresses the rows in
     the frames closest to their parents' (``hgs.hierarchy.align_hierarchy_gpu``);
  3. write the result (write_hierarchy; ``--half``: half-precision rows).

Beside the input, ``anchors.bin`` (an int32 count and that many int32 node indices) is remapped to the new numbering --
anchors at dropped nodes go, the count is rewritten, the order stays -- and written beside the output; ``exposure.json``
is copied.  Printed: one sentence with the counts.  A hierarchy that fails a check, or all of whose leaves would go, is
named with the check and the node, nothing is written, exit status 1."""
from __future__ import annotations

import os
import shutil
import sys

import numpy as np

from ._hier_command import check_exit, missing_path, read_input, upload, usage_exit, walk_args, with_tail, write_output

USAGE = ("usage: python -m hgs.prune_hierarchy <in.hier> <out.hier> [--remove-box x0 y0 z0 x1 y1 z1]... "
         "[--keep-box x0 y0 z0 x1 y1 z1] [--min-opacity A] [--max-scale S] [--mask <file.npy>] "
         "[--remerge dirty|all|none] [--align] [--half]   (at least one criterion; at most 16 remove boxes)")
OPTIONS = {"--remove-box": 6, "--keep-box": 6, "--min-opacity": 1, "--max-scale": 1, "--mask": 1, "--remerge": 1,
           "--align": 0, "--half": 0}
REMERGE = ("dirty", "all", "none")
MAX_BOXES = 16


def parse_args(argv):
    """-> dict(in_path, out_path, remove_boxes, keep_box, min_opacity, max_scale, mask, remerge, align, half) or None
    for a usage error (no criterion at all included).  Every --remove-box counts; of the others the last one wins."""
    walked = walk_args(argv, OPTIONS)
    if walked is None:
        return None
    pos, seen = walked
    try:
        nums = {name: [[float(x) for x in vals] for vals in seen[name]]
                for name in ("--remove-box", "--keep-box", "--min-opacity", "--max-scale")}
    except ValueError:
        return None
    if any(x != x for lists in nums.values() for vals in lists for x in vals):
        return None
    box = lambda v: (tuple(v[:3]), tuple(v[3:]))
    remove_boxes = [box(v) for v in nums["--remove-box"]]
    keep_box = box(nums["--keep-box"][-1]) if nums["--keep-box"] else None
    min_opacity = nums["--min-opacity"][-1][0] if nums["--min-opacity"] else None
    max_scale = nums["--max-scale"][-1][0] if nums["--max-scale"] else None
    mask = seen["--mask"][-1][0] if seen["--mask"] else None
    modes = [v[0] for v in seen["--remerge"]]
    if len(pos) != 2 or len(remove_boxes) > MAX_BOXES or any(m not in REMERGE for m in modes):
        return None
    if max_scale is not None and not max_scale > 0.0:
        return None
    if not remove_boxes and keep_box is None and min_opacity is None and max_scale is None and mask is None:
        return None
    return dict(in_path=pos[0], out_path=pos[1], remove_boxes=remove_boxes, keep_box=keep_box, min_opacity=min_opacity,
                max_scale=max_scale, mask=mask, remerge=modes[-1] if modes else "dirty", align=bool(seen["--align"]),
                half=bool(seen["--half"]))


def remap_anchors(anchors, new_of_old):
    """``anchors`` (node indices, any integer array) through ``new_of_old`` (-1 at dropped nodes) -> (int32 array of the
    surviving anchors in their old order and new numbering, how many were dropped).  An index outside the map counts as
    dropped."""
    a = np.asarray(anchors, dtype=np.int64).reshape(-1)
    m = np.asarray(new_of_old, dtype=np.int64).reshape(-1)
    ok = (a >= 0) & (a < m.shape[0])
    new = np.where(ok, m[np.where(ok, a, 0)], -1)
    kept = new[new >= 0].astype(np.int32)
    return kept, int(a.shape[0] - kept.shape[0])


def read_anchors(path):
    """anchors.bin -> its int32 indices (the leading int32 count is not trusted: what follows it is the list)."""
    raw = open(path, "rb").read()
    return np.frombuffer(raw[4:len(raw) - (len(raw) - 4) % 4], dtype="<i4").copy()


def write_anchors(path, anchors):
    a = np.asarray(anchors, dtype="<i4").reshape(-1)
    with open(path, "wb") as f:
        f.write(np.array([a.shape[0]], dtype="<i4").tobytes())
        f.write(a.tobytes())


def carry_side_files(in_path, out_path, new_of_old) -> dict:
    """anchors.bin beside the input -> remapped beside the output; exposure.json -> copied (unless the directory is the
    same).  -> dict(anchors=(before, dropped) or None, exposure=bool)."""
    in_dir, out_dir = (os.path.dirname(os.path.abspath(p)) for p in (in_path, out_path))
    done = dict(anchors=None, exposure=False)
    src = os.path.join(in_dir, "anchors.bin")
    if os.path.exists(src):
        old = read_anchors(src)
        kept, dropped = remap_anchors(old, new_of_old)
        write_anchors(os.path.join(out_dir, "anchors.bin"), kept)
        done["anchors"] = (int(old.shape[0]), dropped)
    src = os.path.join(in_dir, "exposure.json")
    if os.path.exists(src):
        if in_dir != out_dir:
            shutil.copyfile(src, os.path.join(out_dir, "exposure.json"))
        done["exposure"] = True
    return done


def run(in_path, out_path, remove_boxes=(), keep_box=None, min_opacity=None, max_scale=None, mask=None, remerge="dirty",
        align=False, half=False) -> dict:
    """Read, prune, write; -> figures of the run."""
    from .hierarchy import prune_hierarchy_gpu
    host, N, G, read_s = read_input("prune_hierarchy", in_path)
    remove = None
    if mask is not None:
        remove = np.load(mask, allow_pickle=False).reshape(-1)
        if remove.shape[0] != N:
            raise ValueError(f"{mask}: {remove.shape[0]} entries; one per node (N = {N}) expected")
    stats = {}
    r = prune_hierarchy_gpu(upload(host, rows=N), remove_boxes=list(remove_boxes), keep_box=keep_box, min_opacity=min_opacity,
                            max_scale=max_scale, remove=remove, remerge=remerge, align=align, stats=stats)
    write_s = write_output(out_path, with_tail(r.hierarchy, host, N) + [r.hierarchy.nodes, r.hierarchy.boxes], half)
    side = carry_side_files(in_path, out_path, r.new_of_old.cpu().numpy())
    return dict(nodes=N, kept=r.hierarchy.num_nodes, removed=r.removed_leaves, dead=r.dead, dirty=r.dirty,
                single=r.single_child, remerge=remerge, align=align, tail=G - N, prune_ms=stats["prune_ms"], read_s=read_s,
                write_s=write_s, side=side, path=out_path)


def main(argv=None) -> int:
    parsed = parse_args(sys.argv[1:] if argv is None else list(argv))
    if parsed is None or missing_path("prune_hierarchy", parsed["in_path"], parsed["mask"]):
        return usage_exit(USAGE)
    from .hierarchy import HierarchyPruneError
    try:
        r = run(**parsed)
    except HierarchyPruneError as e:
        return check_exit("prune_hierarchy", f"{parsed['in_path']}: {e.check} (node {e.node}): {e}")
    rows = {"dirty": f"{r['dirty']} ancestors re-merged", "all": f"every node with children re-merged ({r['dirty']} got new boxes)",
            "none": f"{r['dirty']} ancestors got new boxes, no row re-merged"}[r["remerge"]]
    anchors = "no anchors.bin beside the input"
    if r["side"]["anchors"] is not None:
        before, dropped = r["side"]["anchors"]
        anchors = f"anchors.bin remapped, {dropped} of {before} anchors dropped"
    print(f"prune_hierarchy: N = {r['nodes']} -> {r['kept']} nodes: {r['removed']} leaves removed, {r['dead']} nodes dropped "
          f"in all, {rows}, {r['single']} nodes left with a single child{', frames aligned' if r['align'] else ''}, "
          f"{r['tail']} rows behind the nodes carried through, {anchors}"
          f"{', exposure.json copied' if r['side']['exposure'] else ''}; prune {r['prune_ms']:.2f} ms on the device (read "
          f"{r['read_s']:.2f} s, write {r['write_s']:.2f} s) -> {r['path']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
