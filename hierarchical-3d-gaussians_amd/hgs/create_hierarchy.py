"""Hierarchy creator: a trained chunk's ``point_cloud.ply`` -> ``<out dir>/hierarchy.hier``.

    python -m hgs.create_hierarchy [--align] <point_cloud.ply> <chunk dir> <out dir> [<scaffold dir>]

The positional form of the reference's per-chunk creator call (scripts/full_train.py:185-196), so only the executable
changes; the output is what ``train_post.py --hierarchy`` and ``render_hierarchy.py`` load.  Steps:

  1. read the PLY (hgs.ply: save_ply layout, activated rows);
  2. drop the first ``skybox_points`` rows: the count is the first line of ``pc_info.txt`` beside the PLY, else of
     ``<scaffold dir>/pc_info.txt``, else 0 (the reference puts skybox rows first, scene/gaussian_model.py:169-180, and
     appends the scaffold's skybox again when it loads a hierarchy);
  3. if ``<chunk dir>/center.txt`` and ``extent.txt`` exist, keep the rows with max(|x - cx|, |y - cy|) <= 0.5 extent[0]
     -- the complement of the reference's "outside the chunk" test (scene/gaussian_model.py:232-235), which drops the
     scaffold ring train_single.py put in front of the chunk's own Gaussians;
  4. build with ``hgs.hierarchy.build_hierarchy_gpu`` and write the upstream .hier layout (write_hierarchy).

``--align`` (opt-in, anywhere among the arguments) runs ``hgs.hierarchy.align_hierarchy_gpu`` between the build and the
write: every node's rotation and scales re-parametrised to lie close to its parent's frame, the
Gaussians unchanged.  Without the flag the output is byte for byte what it was before the flag existed.

This project's construction rule, not a restatement of the reference's creator."""
from __future__ import annotations

import os
import sys
import time

import torch

from . import ply
from ._hier_command import require_gpu, usage_exit, write_output
from .synth import Scene

USAGE = "usage: python -m hgs.create_hierarchy [--align] <point_cloud.ply> <chunk dir> <out dir> [<scaffold dir>]"


def read_skybox_count(ply_path, scaffold_dir=None) -> int:
    for d in (os.path.dirname(os.path.abspath(ply_path)), scaffold_dir):
        if d and os.path.exists(os.path.join(d, "pc_info.txt")):
            with open(os.path.join(d, "pc_info.txt")) as f:
                return int(f.readline())
    return 0


def read_chunk_bounds(chunk_dir):
    """-> (center[3], extent[3]) float32 tensors, or None without center.txt / extent.txt (parsed as the reference
    parses them: the first line, split at single spaces)."""
    c_path, e_path = os.path.join(chunk_dir, "center.txt"), os.path.join(chunk_dir, "extent.txt")
    if not (os.path.exists(c_path) and os.path.exists(e_path)):
        return None
    with open(c_path) as cf, open(e_path) as ef:
        c, e = cf.readline().split(" "), ef.readline().split(" ")
    return torch.tensor([float(c[0]), float(c[1]), float(c[2])]), torch.tensor([float(e[0]), float(e[1]), float(e[2])])


def select_rows(xyz, skybox_points=0, bounds=None) -> torch.Tensor:
    """Row indices (int64, ascending) kept for the hierarchy: the rows behind the first ``skybox_points``, and of
    those, with ``bounds`` = (center, extent), the ones with max(|x - cx|, |y - cy|) <= 0.5 extent[0] (float32, as the
    reference's test)."""
    xyz = torch.as_tensor(xyz, dtype=torch.float32)
    keep = torch.ones(xyz.shape[0], dtype=torch.bool)
    keep[:max(int(skybox_points), 0)] = False
    if bounds is not None:
        center, extent = bounds
        d = torch.abs(xyz - center.to(torch.float32))
        keep &= torch.max(d[:, 0], d[:, 1]) <= 0.5 * extent.to(torch.float32)[0]
    return keep.nonzero().flatten()


def subset(scene: Scene, rows) -> Scene:
    return Scene(*(t[rows].contiguous() for t in (scene.means3D, scene.scales, scene.rotations, scene.opacities,
                                                    scene.shs)), scene.sh_degree)


def split_flags(argv, flags=("--align",)):
    """-> (the positional arguments in order, the set of ``flags`` present): a flag may stand anywhere."""
    return [a for a in argv if a not in flags], {a for a in argv if a in flags}


def run(ply_path, chunk_dir, out_dir, scaffold_dir=None, align=False) -> dict:
    """Read, select, build, (align,) write; -> figures of the run (rows read / kept, N, read / write seconds, build ms
    and, with ``align``, align ms from device events)."""
    from .hierarchy import align_hierarchy_gpu, build_hierarchy_gpu
    require_gpu("create_hierarchy")
    t0 = time.perf_counter()
    scene = ply.read_ply(ply_path)
    rows = select_rows(scene.means3D, read_skybox_count(ply_path, scaffold_dir), read_chunk_bounds(chunk_dir))
    if rows.numel() == 0:
        raise RuntimeError(f"{ply_path}: no rows left after the skybox drop and the chunk bounds")
    sel = subset(scene, rows)
    t_read = time.perf_counter() - t0
    dev = torch.device("cuda", torch.cuda.current_device())
    sel_dev = sel.to(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    h = build_hierarchy_gpu(sel_dev, dev)
    ev[1].record()
    ev[1].synchronize()
    stats = {}
    if align:
        align_hierarchy_gpu(h, stats)
    out_path = os.path.join(out_dir, "hierarchy.hier")
    write_s = write_output(out_path, h)
    return dict(rows_read=scene.P, rows_kept=int(rows.numel()), nodes=h.num_nodes, build_ms=ev[0].elapsed_time(ev[1]),
                align_ms=stats.get("align_ms"), read_s=t_read, write_s=write_s, path=out_path)


def main(argv=None) -> int:
    argv, flags = split_flags(sys.argv[1:] if argv is None else list(argv))
    if len(argv) not in (3, 4):
        return usage_exit(USAGE)
    r = run(*argv, align="--align" in flags)
    aligned = f", align {r['align_ms']:.2f} ms" if r["align_ms"] is not None else ""
    print(f"create_hierarchy: read {r['rows_read']} rows, kept {r['rows_kept']}, N = {r['nodes']} nodes, "
          f"build {r['build_ms']:.2f} ms{aligned} (read {r['read_s']:.2f} s, write {r['write_s']:.2f} s) -> {r['path']}",
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
