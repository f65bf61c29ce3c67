"""A coloured triangle mesh of a region of a hierarchy file: ``<in.hier>`` -> ``<out.ply>``.

    python -m hgs.mesh_hierarchy <in.hier> <out.ply> --cameras <cameras.json> (--roi x0 y0 z0 x1 y1 z1 | --roi-root)
        --voxel S [--trunc T] [--tau-px PX] [--min-alpha A] [--min-weight K] [--no-colour] [--no-frustum]
        [--resolution-scale S] [--volume-out <v.npz>] [--sparse]

For collision and navigation, for measuring, for placing ``--remove-box`` / ``--roi`` boxes, and to see what a cut at a
given granularity shows as a surface.  Every camera of the ``cameras.json`` (the file ``python -m hgs.score_hierarchy``
reads) is rendered at the cut of ``--tau-px`` pixels (default 0: the leaves) and read per pixel; the depth at which a
pixel becomes half opaque is fused over the views into a truncated signed distance volume over the region, and a
surface-net mesh is extracted from it.  Steps:

  1. read the cameras (``--resolution-scale S`` divides every camera's width and height by S), then the file;
  2. the region: ``--roi`` in world units, or ``--roi-root`` for the root node's box; the lattice ``lo + S i`` inside it
     must hold at most ``hgs.meshing.MAX_EXTRACT_SAMPLES`` samples -- else the voxel size that fits is named;
  3. ``hgs.meshing.fuse_hierarchy`` (pixels with ``alpha < --min-alpha``, default 0.5, carry no depth; ``--trunc`` is
     the truncation distance, default 4 voxels; ``--no-colour`` skips the colour volume and the render it needs), then
     ``TsdfVolume.extract`` over the samples of weight >= ``--min-weight`` (default 1: seen by one view);
  4. ``hgs.meshing.write_mesh_ply``; ``--volume-out`` also writes the volume's arrays.

``--sparse`` fuses into a ``hgs.meshing.SparseTsdfVolume``: the lattice is virtual, 8 x 8 x 8
blocks are allocated near the surface the cameras see (a first pass over the cameras reads the depth alone), and the limit
of step 2 becomes 2^31 - 1 BLOCKS of the region -- which makes ``--roi-root`` practical at a voxel worth having.  The mesh
is the dense one with its vertices and faces in block order.

Printed: one sentence with the volume size and the vertex and face counts.  Usage errors exit with 2; a hierarchy or
camera file that cannot be used, or a region that is too large, is named, nothing is written, exit status 1."""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np

from ._hier_command import check_exit, missing_path, read_input, upload, usage_exit, walk_args
from .score_hierarchy import read_cameras

USAGE = ("usage: python -m hgs.mesh_hierarchy <in.hier> <out.ply> --cameras <cameras.json> "
         "(--roi x0 y0 z0 x1 y1 z1 | --roi-root) --voxel S [--trunc T] [--tau-px PX] [--min-alpha A] [--min-weight K] "
         "[--no-colour] [--no-frustum] [--resolution-scale S] [--volume-out <v.npz>] [--sparse]")
SINGLE = ("--cameras", "--roi", "--voxel", "--trunc", "--tau-px", "--min-alpha", "--min-weight", "--resolution-scale",
          "--volume-out")
OPTIONS = {**dict.fromkeys(SINGLE, 1), "--roi": 6, "--roi-root": 0, "--no-colour": 0, "--no-frustum": 0, "--sparse": 0}


def parse_args(argv):
    """-> dict(in_path, out_path, cameras, roi, voxel, trunc, tau_px, min_alpha, min_weight, colour, frustum,
    resolution_scale, volume_out), with the key ``sparse`` (True) only when --sparse is given, or None for a usage error:
    an option given twice, not two paths, no --cameras, no --voxel, not exactly one of --roi / --roi-root, a --roi with
    lo > hi, a number that is not one or out of range."""
    walked = walk_args(argv, OPTIONS)
    if walked is None or any(len(walked[1][k]) > 1 for k in OPTIONS):
        return None
    pos, seen = walked
    one = {k: seen[k][0] if seen[k] else None for k in SINGLE}
    number = lambda k, default: default if one[k] is None else float(one[k][0])
    positive = lambda x: x is None or (x > 0.0 and math.isfinite(x))
    try:
        roi = None if one["--roi"] is None else tuple(float(t) for t in one["--roi"])
        voxel, trunc = number("--voxel", None), number("--trunc", None)
        tau_px, min_alpha, min_weight = number("--tau-px", 0.0), number("--min-alpha", 0.5), number("--min-weight", 1.0)
        scale = number("--resolution-scale", 1.0)
    except ValueError:
        return None
    if len(pos) != 2 or one["--cameras"] is None or voxel is None or (roi is None) == (not seen["--roi-root"]):
        return None
    if roi is not None and not (all(math.isfinite(v) for v in roi) and all(roi[a] <= roi[a + 3] for a in range(3))):
        return None
    if not (positive(voxel) and positive(trunc) and positive(min_weight) and positive(scale)):
        return None
    if not tau_px >= 0.0 or not 0.0 <= min_alpha <= 1.0:
        return None
    out = dict(in_path=pos[0], out_path=pos[1], cameras=one["--cameras"][0], roi=roi, voxel=voxel, trunc=trunc,
               tau_px=tau_px, min_alpha=min_alpha, min_weight=min_weight, colour=not seen["--no-colour"],
               frustum=not seen["--no-frustum"], resolution_scale=scale,
               volume_out=None if one["--volume-out"] is None else one["--volume-out"][0])
    if seen["--sparse"]:
        out["sparse"] = True
    return out


def checked_region(roi, voxel, sparse=False):
    """-> (lo, hi, dims) of the region; ValueError naming the voxel size that fits when it holds too many samples (with
    ``sparse``: too many blocks)."""
    from .meshing import BLOCK, MAX_EXTRACT_SAMPLES, MAX_GRID_BLOCKS, fitting_voxel, volume_dims
    lo, hi = np.asarray(roi[:3], np.float64), np.asarray(roi[3:], np.float64)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise ValueError(f"the region {lo.tolist()} .. {hi.tolist()} is not a finite box")
    dims = volume_dims(lo, hi, voxel)
    n = dims[0] * dims[1] * dims[2]
    if sparse:
        blocks = math.prod((d - 1) // BLOCK + 1 for d in dims)
        if max(dims) > 2 ** 31 - 1 or blocks > MAX_GRID_BLOCKS:
            raise ValueError(f"the region holds {dims[0]} x {dims[1]} x {dims[2]} samples at --voxel {voxel:g}: {blocks} "
                             f"blocks, more than {MAX_GRID_BLOCKS}")
        return lo, hi, dims
    if n > MAX_EXTRACT_SAMPLES:
        raise ValueError(f"the region holds {dims[0]} x {dims[1]} x {dims[2]} = {n} samples at --voxel {voxel:g}, more than "
                         f"{MAX_EXTRACT_SAMPLES}; --voxel {fitting_voxel(lo, hi):g} fits")
    return lo, hi, dims


def run(in_path, out_path, cameras, roi, voxel, trunc=None, tau_px=0.0, min_alpha=0.5, min_weight=1.0, colour=True,
        frustum=True, volume_out=None, sparse=False) -> dict:
    """Read, fuse, extract, write; -> figures of the run.  ``cameras``: a list of ``hgs.synth.Camera``; ``roi``: six
    numbers or None for the root node's box."""
    import torch
    from .meshing import SparseTsdfVolume, TsdfVolume, fuse_hierarchy, write_mesh_ply
    host, N, G, read_s = read_input("mesh_hierarchy", in_path)
    if roi is None:
        box = host.boxes.reshape(-1, 2, 4)[0].double().numpy()
        roi = tuple(box[0, :3]) + tuple(box[1, :3])
    lo, hi, dims = checked_region(roi, voxel, sparse)
    h = upload(host, rows=N)
    t0 = time.perf_counter()
    vol = (SparseTsdfVolume if sparse else TsdfVolume)(lo, hi, voxel, trunc=trunc, colour=colour)
    fuse_hierarchy(h, cameras, vol, tau_px=tau_px, frustum=frustum, min_alpha=min_alpha, colour=colour)
    mesh = vol.extract(min_weight=min_weight)
    torch.cuda.synchronize()
    run_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    write_mesh_ply(out_path, mesh)
    if volume_out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(volume_out)), exist_ok=True)
        with open(volume_out, "wb") as f:            # (a file object: numpy appends no suffix of its own)
            np.savez(f, **vol.numpy())
    write_s = time.perf_counter() - t0
    return dict(nodes=N, tail=G - N, dims=dims, lo=lo, hi=hi, trunc=vol.trunc, views=len(cameras),
                observed=int((vol.weight >= min_weight).sum()), vertices=int(mesh.vertices.shape[0]),
                faces=int(mesh.faces.shape[0]), run_s=run_s, read_s=read_s, write_s=write_s,
                blocks=vol.n_blocks if sparse else None)


def main(argv=None) -> int:
    a = parse_args(sys.argv[1:] if argv is None else list(argv))
    if a is None or missing_path("mesh_hierarchy", a["in_path"], a["cameras"]):
        return usage_exit(USAGE)
    try:
        cameras = read_cameras(a["cameras"], a["resolution_scale"])
    except (ValueError, OSError) as e:
        return usage_exit(USAGE, f"mesh_hierarchy: {e}")
    try:
        if a["roi"] is not None:
            checked_region(a["roi"], a["voxel"], a.get("sparse", False))         # before the file is read
        r = run(a["in_path"], a["out_path"], cameras, a["roi"], a["voxel"], a["trunc"], a["tau_px"], a["min_alpha"],
                a["min_weight"], a["colour"], a["frustum"], a["volume_out"], a.get("sparse", False))
    except ValueError as e:
        return check_exit("mesh_hierarchy", f"{a['in_path']}: {e}")
    nx, ny, nz = r["dims"]
    outs = [p for p in (a["out_path"], a["volume_out"]) if p is not None]
    blocks = "" if r["blocks"] is None else f", sparse: {r['blocks']} blocks of 512 allocated"
    print(f"mesh_hierarchy: N = {r['nodes']} nodes, {r['views']} views at {a['tau_px']:g} px"
          f"{'' if a['frustum'] else ', no frustum cull'}; volume {nx} x {ny} x {nz} = {nx * ny * nz} samples of "
          f"{a['voxel']:g} (truncation {r['trunc']:g}){blocks}, {r['observed']} observed; {r['vertices']} vertices, {r['faces']} "
          f"faces{'' if a['colour'] else ', no colour'}; {r['tail']} rows behind the nodes ignored; fused and extracted in "
          f"{r['run_s']:.2f} s (read {r['read_s']:.2f} s, write {r['write_s']:.2f} s) -> {', '.join(outs)}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
