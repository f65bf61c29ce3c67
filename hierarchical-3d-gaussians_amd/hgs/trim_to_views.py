"""Trimmer for an existing hierarchy file under a set of views: ``<in.hier>`` -> a smaller ``<out.hier>``.

    python -m hgs.trim_to_views <in.hier> <out.hier>
        (--cameras <cameras.json> | --view x y z ... | --view-box x0 y0 z0 x1 y1 z1 ...) [--pad R]
        (--tau T | --tau-px PX --tanfovx X --width W) [--min-extent E] [--max-nodes K] [--roi x0 y0 z0 x1 y1 z1]

The view set is where the cameras may stand: the ``"position"`` of every entry of a ``cameras.json`` (the file a
training run writes beside its model), single positions (``--view``, repeatable) and closed boxes of positions
(``--view-box``, repeatable), each position widened by ``--pad`` on every side.  The granularity is given directly
(``--tau``) or in pixels as the renderer takes it (``--tau-px`` with the camera's tan(fovx / 2) and image width:
tau = (2 (PX + 0.5)) tanfovx / (0.5 width)).  Nodes go whose parent no view of the set can see at a size >= tau
(DESIGN.md section 4): for every viewpoint inside the set and every granularity >= tau the cut of the output is the
input's.  ``--min-extent``, ``--roi`` and ``--max-nodes`` as for ``hgs.trim_hierarchy``, except that a node budget
resolves to a granularity, not an extent.  Steps:

  1. read the file (load_hierarchy: any of the layouts it accepts);
  2. ``hgs.hierarchy.trim_to_views_gpu`` on the N node rows; rows behind them (the skybox tail save_hier appends) are
     carried through unchanged, behind the N' kept rows;
  3. write the result (write_hierarchy).

Printed: N -> N' and the stub count, the number of view regions, the tau that was used, reach / plan / apply in ms, read
and write seconds.  A hierarchy that fails a check is named with the check and the node, nothing is written, exit status
1; usage errors exit with 2.  ``anchors.bin`` and ``exposure.json`` beside the input are neither copied nor remapped
(said so when they exist)."""
from __future__ import annotations

import json
import sys

from ._hier_command import (check_exit, missing_path, read_input, side_files_beside, upload, usage_exit, walk_args,
                            with_tail, write_output)

USAGE = ("usage: python -m hgs.trim_to_views <in.hier> <out.hier> (--cameras <cameras.json> | --view x y z ... | "
         "--view-box x0 y0 z0 x1 y1 z1 ...) [--pad R] (--tau T | --tau-px PX --tanfovx X --width W) [--min-extent E] "
         "[--max-nodes K] [--roi x0 y0 z0 x1 y1 z1]")
SINGLE = ("--cameras", "--pad", "--tau", "--tau-px", "--tanfovx", "--width", "--min-extent", "--max-nodes")
OPTIONS = {**dict.fromkeys(SINGLE, 1), "--view": 3, "--view-box": 6, "--roi": 6}     # SINGLE and --roi: refused twice


def tau_from_pixels(px, tanfovx, width):
    """The renderer's granularity for a target of ``px`` pixels: (2 (px + 0.5)) tanfovx / (0.5 width)."""
    return (2.0 * (px + 0.5)) * tanfovx / (0.5 * width)


def read_camera_positions(path):
    """The ``"position"`` of every entry of a cameras.json -> a list of [x, y, z] (floats); ValueError naming the entry
    that has none, or a file that is no list of entries."""
    with open(path) as f:
        data = json.load(f)
    if not isinstance(data, list) or not data:
        raise ValueError(f"{path}: a non-empty list of cameras expected")
    out = []
    for k, cam in enumerate(data):
        pos = cam.get("position") if isinstance(cam, dict) else None
        if not isinstance(pos, (list, tuple)) or len(pos) != 3 or not all(isinstance(x, (int, float)) and
                                                                           not isinstance(x, bool) for x in pos):
            raise ValueError(f"{path}: camera {k} has no \"position\" of three numbers")
        out.append([float(x) for x in pos])
    return out


def parse_args(argv):
    """-> dict(in_path, out_path, cameras, views, view_boxes, pad, tau, min_extent, max_nodes, roi) or None for a usage
    error.  ``tau`` is resolved from --tau-px here."""
    walked = walk_args(argv, OPTIONS)
    if walked is None or any(len(walked[1][k]) > 1 for k in SINGLE + ("--roi",)):
        return None
    pos, seen = walked
    one = {k: seen[k][0][0] if seen[k] else None for k in SINGLE}
    try:
        views, view_boxes, rois = ([tuple(float(x) for x in vals) for vals in seen[k]]
                                   for k in ("--view", "--view-box", "--roi"))
        num = {k: (None if one[k] is None else float(one[k])) for k in ("--pad", "--tau", "--tau-px", "--tanfovx",
                                                                        "--width", "--min-extent")}
        max_nodes = None if one["--max-nodes"] is None else int(one["--max-nodes"])
    except ValueError:
        return None
    roi = (rois[0][:3], rois[0][3:]) if rois else None
    if len(pos) != 2 or (one["--cameras"] is None and not views and not view_boxes):
        return None
    if any(x is not None and x != x for x in num.values()) or any(x != x for v in views + view_boxes for x in v):
        return None
    px_parts = [num[k] for k in ("--tau-px", "--tanfovx", "--width")]
    if num["--tau"] is not None:
        if any(x is not None for x in px_parts):
            return None
        tau = num["--tau"]
    else:
        if any(x is None for x in px_parts) or not (px_parts[1] > 0.0 and px_parts[2] > 0.0):
            return None
        tau = tau_from_pixels(*px_parts)
    if (num["--pad"] is not None and not num["--pad"] >= 0.0) or (max_nodes is not None and max_nodes < 1):
        return None
    if roi is not None and any(x != x for r in roi for x in r):
        return None
    return dict(in_path=pos[0], out_path=pos[1], cameras=one["--cameras"], views=views, view_boxes=view_boxes,
                pad=0.0 if num["--pad"] is None else num["--pad"], tau=tau,
                min_extent=0.0 if num["--min-extent"] is None else num["--min-extent"], max_nodes=max_nodes, roi=roi)


def regions_of(cameras=None, views=(), view_boxes=(), pad=0.0):
    """The view set of a command line (hgs.hierarchy.view_regions): camera positions and --view points padded, --view-box
    boxes as they are."""
    from .hierarchy import view_regions
    points = (read_camera_positions(cameras) if cameras is not None else []) + [list(v) for v in views]
    return view_regions(points=points or None, boxes=list(view_boxes) or None, pad=pad)


def run(in_path, out_path, regions, tau, min_extent=0.0, max_nodes=None, roi=None) -> dict:
    """Read, trim, write; -> figures of the run."""
    from .hierarchy import trim_to_views_gpu
    host, N, G, read_s = read_input("trim_to_views", in_path)
    stats = {}
    r = trim_to_views_gpu(upload(host, rows=N), regions, tau, min_extent, roi, max_nodes, stats)
    write_s = write_output(out_path, with_tail(r.hierarchy, host, N) + [r.hierarchy.nodes, r.hierarchy.boxes])
    return dict(nodes=N, kept=r.hierarchy.num_nodes, stubs=r.stubs, regions=int(regions[0].shape[0]), tau=r.tau,
                tail=G - N, reach_ms=stats["reach_ms"], plan_ms=stats["plan_ms"], apply_ms=stats["apply_ms"],
                read_s=read_s, write_s=write_s, beside=side_files_beside(in_path), path=out_path)


def main(argv=None) -> int:
    a = parse_args(sys.argv[1:] if argv is None else list(argv))
    if a is None or missing_path("trim_to_views", a["in_path"], a["cameras"]):
        return usage_exit(USAGE)
    try:
        regions = regions_of(a["cameras"], a["views"], a["view_boxes"], a["pad"])
    except (ValueError, OSError) as e:
        return usage_exit(USAGE, f"trim_to_views: {e}")
    from .hierarchy import HierarchyTrimError
    try:
        r = run(a["in_path"], a["out_path"], regions, a["tau"], a["min_extent"], a["max_nodes"], a["roi"])
    except HierarchyTrimError as e:
        return check_exit("trim_to_views", f"{a['in_path']}: {e.check} (node {e.node}): {e}")
    print(f"trim_to_views: N = {r['nodes']} -> {r['kept']} nodes ({r['stubs']} stubs), {r['regions']} view regions, tau "
          f"{r['tau']:.9g} used, {r['tail']} rows behind the nodes carried through, reach {r['reach_ms']:.2f} ms, plan "
          f"{r['plan_ms']:.2f} ms, apply {r['apply_ms']:.2f} ms on the device (read {r['read_s']:.2f} s, write "
          f"{r['write_s']:.2f} s) -> {r['path']}", flush=True)
    for f in r["beside"]:
        print(f"trim_to_views: {f} beside the input is not copied or remapped", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
