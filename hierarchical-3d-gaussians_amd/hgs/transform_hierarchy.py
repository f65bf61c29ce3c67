"""Similarity transform of an existing hierarchy file: ``<in.hier>`` -> ``<out.hier>`` in another coordinate frame.

    python -m hgs.transform_hierarchy <in.hier> <out.hier> [--scale S]
        [--quat w x y z | --axis-angle ax ay az deg | --matrix <16 numbers, row-major, similarity>]
        [--translate x y z] [--invert] [--half] [--refit cube|ellipsoid|keep]

The map is x' = s R x + t (``--invert``: its inverse).  ``--matrix`` takes the 4x4 matrix of column vectors
[[s R, t], [0 0 0 1]] and replaces --scale, the rotation options and --translate; a matrix with shear, non-uniform
scale, a mirror or a projective last row is refused and named.  At least one option that defines a map is required.
Steps:

  1. read the file (load_hierarchy: any of the layouts it accepts);
  2. ``hgs.hierarchy.transform_hierarchy_gpu`` in place on the device: every row -- the rows
     behind the node rows (the skybox tail) included -- gets its mean, rotation, scales and SH bands moved, every box
     becomes the box of the rotated box, node records and opacities are copied; ``--refit``: then
     ``hgs.hierarchy.refit_boxes_gpu`` in place with that leaf rule, so that the boxes are tight in the new frame again
     (a general rotation grows them by up to sqrt 3); without the flag the output is what it was before the flag existed;
  3. write the result (write_hierarchy; ``--half``: its half-precision variant).

``anchors.bin`` and ``exposure.json`` beside the input hold indices and per-image data, which a change of frame does
not touch: they are copied beside the output (said so when they exist).  Printed: the map, N and the tail rows, the
device time, read and write seconds."""
from __future__ import annotations

import math
import sys

import numpy as np

from ._hier_command import carry_side_files, missing_path, read_input, upload, usage_exit, walk_args, write_output

USAGE = ("usage: python -m hgs.transform_hierarchy <in.hier> <out.hier> [--scale S] [--quat w x y z | --axis-angle ax ay az "
         "deg | --matrix <16 numbers, row-major>] [--translate x y z] [--invert] [--half] [--refit cube|ellipsoid|keep]   (at least one of --scale, "
         "--quat, --axis-angle, --matrix, --translate)")
OPTIONS = {"--scale": 1, "--quat": 4, "--axis-angle": 4, "--matrix": 16, "--translate": 3, "--refit": 1, "--invert": 0,
           "--half": 0}
REFIT_MODES = ("cube", "ellipsoid", "keep")
MATRIX_TOL = 1e-6     # how far a typed matrix may be from a similarity; its rotation is then the nearest one (SVD)


class NotASimilarity(ValueError):
    """--matrix named something that is not x' = s R x + t with a proper rotation."""


def similarity_from_matrix(m):
    """16 numbers, row-major, of [[s R, t], [0 0 0 1]] -> (R float64 [3,3], s, t float64 [3]); ``NotASimilarity`` names
    a projective last row, a mirror, or shear / non-uniform scale (|A A^T / s^2 - I| > MATRIX_TOL)."""
    m = np.asarray(m, dtype=np.float64).reshape(4, 4)
    if not np.isfinite(m).all():
        raise NotASimilarity("the matrix has a value that is not finite")
    if np.abs(m[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > MATRIX_TOL:
        raise NotASimilarity("the last row is not 0 0 0 1: a projective matrix, not a similarity")
    A = m[:3, :3]
    det = float(np.linalg.det(A))
    if det < 0:
        raise NotASimilarity("the determinant is negative: a mirror, not a similarity with a proper rotation")
    if det == 0:
        raise NotASimilarity("the matrix is singular")
    s = det ** (1.0 / 3.0)
    Q = A / s
    if np.abs(Q @ Q.T - np.eye(3)).max() > MATRIX_TOL:
        raise NotASimilarity("shear or non-uniform scale: the upper 3x3 is not a rotation times one scale")
    u, _, vt = np.linalg.svd(Q)
    return u @ vt, s, m[:3, 3].copy()


def parse_args(argv):
    """-> dict(in_path, out_path, R or None, quat or None, scale, translate, invert, half, refit or None), None for a
    usage error; a --matrix that is not a similarity raises ``NotASimilarity``."""
    walked = walk_args(argv, OPTIONS)
    if walked is None:
        return None
    pos, seen = walked
    last = lambda name: ([[float(x) for x in vals] for vals in seen[name]] or [None])[-1]     # the last occurrence wins
    try:
        scale, quat, axis_angle, matrix, translate = (last(k) for k in ("--scale", "--quat", "--axis-angle", "--matrix",
                                                                        "--translate"))
    except ValueError:
        return None
    refits = [v[0] for v in seen["--refit"]]
    if any(v not in REFIT_MODES for v in refits):
        return None
    scale, refit = None if scale is None else scale[0], refits[-1] if refits else None
    invert, half = bool(seen["--invert"]), bool(seen["--half"])
    given = [x is not None for x in (quat, axis_angle, matrix)]
    if len(pos) != 2 or sum(given) > 1 or (matrix is not None and (scale is not None or translate is not None)):
        return None
    if not any(given) and scale is None and translate is None:
        return None
    every = [v for x in (quat, axis_angle, matrix, translate) if x is not None for v in x] + ([scale] if scale is not None else [])
    if not all(math.isfinite(v) for v in every) or (scale is not None and scale <= 0.0):
        return None
    R = None
    if quat is not None and not any(quat):
        return None
    if axis_angle is not None:
        n = math.sqrt(sum(v * v for v in axis_angle[:3]))
        if n == 0.0:
            return None
        half_angle = math.radians(axis_angle[3]) / 2
        quat = [math.cos(half_angle)] + [math.sin(half_angle) * v / n for v in axis_angle[:3]]
    if matrix is not None:
        R, scale, translate = similarity_from_matrix(matrix)
        translate = [float(v) for v in translate]
    return dict(in_path=pos[0], out_path=pos[1], R=R, quat=quat, scale=1.0 if scale is None else float(scale),
                translate=[0.0, 0.0, 0.0] if translate is None else translate, invert=invert, half=half, refit=refit)


def build_similarity(p):
    from .hierarchy import similarity
    sim = similarity(R=p["R"], quat=p["quat"], scale=p["scale"], translate=p["translate"])
    return sim.inverse() if p["invert"] else sim


def run(p) -> dict:
    """Read, transform, write; -> figures of the run."""
    from .hierarchy import refit_boxes_gpu, transform_hierarchy_gpu
    sim = build_similarity(p)
    host, N, G, read_s = read_input("transform_hierarchy", p["in_path"])
    h = upload(host)
    stats = {}
    transform_hierarchy_gpu(h, sim, inplace=True, stats=stats)
    if p.get("refit"):
        refit_boxes_gpu(h, p["refit"], inplace=True, stats=stats)
    write_s = write_output(p["out_path"], h, p["half"])
    beside, same_dir = carry_side_files(p["in_path"], p["out_path"])
    return dict(nodes=N, tail=G - N, sim=sim, transform_ms=stats["transform_ms"], refit=p.get("refit"),
                refit_ms=stats.get("refit_ms"), read_s=read_s, write_s=write_s, beside=beside, same_dir=same_dir,
                path=p["out_path"])


def main(argv=None) -> int:
    try:
        p = parse_args(sys.argv[1:] if argv is None else list(argv))
    except NotASimilarity as e:
        return usage_exit(USAGE, f"transform_hierarchy: --matrix is refused: {e}")
    if p is None or missing_path("transform_hierarchy", p["in_path"]):
        return usage_exit(USAGE)
    r = run(p)
    sim = r["sim"]
    fmt = lambda v: " ".join(f"{x:.9g}" for x in np.asarray(v).reshape(-1))
    print(f"transform_hierarchy: x' = s R x + t with s = {sim.s:.9g}, quaternion (w x y z) = {fmt(sim.q_R)}, t = {fmt(sim.t)}; "
          f"N = {r['nodes']} nodes, {r['tail']} rows behind the nodes transformed with them, transform "
          f"{r['transform_ms']:.2f} ms on the device (read {r['read_s']:.2f} s, write {r['write_s']:.2f} s) -> {r['path']}",
          flush=True)
    if r["refit"]:
        print(f"transform_hierarchy: boxes refit in the new frame (--refit {r['refit']}), {r['refit_ms']:.2f} ms on the "
              f"device", flush=True)
    for f in r["beside"]:
        how = "stays valid beside the output" if r["same_dir"] else "copied beside the output"
        print(f"transform_hierarchy: {f} holds indices / per-image data, which a change of frame does not touch: {how}",
              flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
