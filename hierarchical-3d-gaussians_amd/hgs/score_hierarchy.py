"""Contribution scores of a hierarchy file over a set of cameras: ``<in.hier>`` -> ``<scores.npz>`` and a prune mask.

    python -m hgs.score_hierarchy <in.hier> <scores.npz> --cameras <cameras.json> [--tau-px PX] [--no-frustum]
        [--resolution-scale S] [--mask-out <mask.npy> (--max-weight-below X | --sum-below X | --pixels-below K)...
        [--unseen keep|remove]]

Which Gaussians never blend a visible weight into any of the views?  For every node of the hierarchy the command collects,
over the cameras of a ``cameras.json`` (the file a training run writes beside its model: per entry ``width``, ``height``,
``position``, ``rotation`` -- camera to world --, ``fx``, ``fy``), the largest blending weight alpha * T it reaches at a
pixel, the sum of its weights, the number of pixels it is blended into and the number of views whose cut held it
(DESIGN.md section 7, f-22).  Steps:

  1. read the file (load_hierarchy: any of the layouts it accepts) and the cameras; ``--resolution-scale S`` divides
     every camera's width and height by S (the field of view stays);
  2. ``hgs.importance.score_hierarchy`` on the N node rows: per camera the cut at ``--tau-px`` pixels (default 0: the
     leaves), culled to the frustum unless ``--no-frustum``, rendered and scored on the device;
  3. write ``wmax`` float32, ``wsum`` float64, ``count`` int64, ``entries`` int64 (all [N]) and ``views`` to the ``.npz``;
  4. with ``--mask-out``: ``hgs.importance.low_contribution_mask`` under the given criteria (all must hold; at least one
     is required) as a uint8 ``.npy`` with one entry per node -- what ``python -m hgs.prune_hierarchy ... --mask`` reads.

Printed: one sentence with the counts.  Usage errors exit with 2; a hierarchy or camera file that cannot be used is named,
nothing is written, exit status 1."""
from __future__ import annotations

import json
import math
import os
import sys
import time

import numpy as np

from ._hier_command import check_exit, missing_path, read_input, upload, usage_exit, walk_args

USAGE = ("usage: python -m hgs.score_hierarchy <in.hier> <scores.npz> --cameras <cameras.json> [--tau-px PX] [--no-frustum] "
         "[--resolution-scale S] [--mask-out <mask.npy> (--max-weight-below X | --sum-below X | --pixels-below K)... "
         "[--unseen keep|remove]]")
SINGLE = ("--cameras", "--tau-px", "--resolution-scale", "--mask-out", "--max-weight-below", "--sum-below",
          "--pixels-below", "--unseen")
OPTIONS = {**dict.fromkeys(SINGLE, 1), "--no-frustum": 0}
CRITERIA = ("--max-weight-below", "--sum-below", "--pixels-below")


def parse_args(argv):
    """-> dict(in_path, out_path, cameras, tau_px, frustum, resolution_scale, mask_out, max_weight_below, sum_below,
    pixels_below, unseen) or None for a usage error: an option given twice, no --cameras, a criterion or --unseen
    without --mask-out, --mask-out without a criterion."""
    walked = walk_args(argv, OPTIONS)
    if walked is None or any(len(walked[1][k]) > 1 for k in SINGLE):
        return None
    pos, seen = walked
    one = {k: seen[k][0][0] if seen[k] else None for k in SINGLE}
    try:
        num = {k: (None if one[k] is None else float(one[k])) for k in ("--tau-px", "--resolution-scale") + CRITERIA}
    except ValueError:
        return None
    if len(pos) != 2 or one["--cameras"] is None or any(x is not None and x != x for x in num.values()):
        return None
    tau_px = 0.0 if num["--tau-px"] is None else num["--tau-px"]
    scale = 1.0 if num["--resolution-scale"] is None else num["--resolution-scale"]
    if not tau_px >= 0.0 or not (scale > 0.0 and scale != math.inf):
        return None
    crit = [num[k] for k in CRITERIA]
    if one["--mask-out"] is None:
        if any(x is not None for x in crit) or one["--unseen"] is not None:
            return None
    elif all(x is None for x in crit):
        return None
    if one["--unseen"] not in (None, "keep", "remove"):
        return None
    return dict(in_path=pos[0], out_path=pos[1], cameras=one["--cameras"], tau_px=tau_px, frustum=not seen["--no-frustum"],
                resolution_scale=scale, mask_out=one["--mask-out"], max_weight_below=crit[0], sum_below=crit[1],
                pixels_below=crit[2], unseen=one["--unseen"] or "keep")


def camera_from_entry(entry, k, resolution_scale=1.0):
    """One entry of a cameras.json -> ``hgs.synth.Camera``: ``position`` / ``rotation`` are camera to world, the
    tangents 0.5 size / f, near and far as ``hgs.synth.make_camera``.  ValueError naming the entry and the field."""
    import torch
    from .synth import Camera, projection_matrix
    if not isinstance(entry, dict):
        raise ValueError(f"camera {k} is no object")
    try:
        W, H = int(entry["width"]), int(entry["height"])
        fx, fy = float(entry["fx"]), float(entry["fy"])
        C = np.asarray(entry["position"], dtype=np.float64).reshape(3)
        R = np.asarray(entry["rotation"], dtype=np.float64).reshape(3, 3)
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError(f"camera {k}: width, height, fx, fy, position [3] and rotation [3][3] expected ({e})") from None
    if W < 1 or H < 1 or not (fx > 0.0 and fy > 0.0) or not (np.isfinite(C).all() and np.isfinite(R).all()):
        raise ValueError(f"camera {k}: sizes and focal lengths must be positive, position and rotation finite")
    fovx, fovy = 2.0 * math.atan(0.5 * W / fx), 2.0 * math.atan(0.5 * H / fy)
    W, H = max(1, int(round(W / resolution_scale))), max(1, int(round(H / resolution_scale)))
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = R.T
    Rt[:3, 3] = -R.T @ C
    Rt[3, 3] = 1.0
    znear, zfar = 0.01, 100.0
    wv = torch.tensor(np.float32(Rt)).transpose(0, 1).contiguous()
    proj = projection_matrix(znear, zfar, fovx, fovy).transpose(0, 1)
    full = (wv.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0).contiguous()
    return Camera(W, H, fovx, fovy, wv, full, wv.inverse()[3, :3].contiguous(), znear, zfar)


def read_cameras(path, resolution_scale=1.0):
    with open(path) as f:
        data = json.load(f)
    if not isinstance(data, list) or not data:
        raise ValueError(f"{path}: a non-empty list of cameras expected")
    try:
        return [camera_from_entry(e, k, resolution_scale) for k, e in enumerate(data)]
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None


def run(in_path, out_path, cameras, tau_px=0.0, frustum=True, mask_out=None, max_weight_below=None, sum_below=None,
        pixels_below=None, unseen="keep") -> dict:
    """Read, score, write; -> figures of the run.  ``cameras``: a list of ``hgs.synth.Camera``."""
    import torch
    from .importance import low_contribution_mask, score_hierarchy
    host, N, G, read_s = read_input("score_hierarchy", in_path)
    h = upload(host, rows=N)
    t0 = time.perf_counter()
    scores = score_hierarchy(h, cameras, tau_px=tau_px, frustum=frustum)
    torch.cuda.synchronize()
    score_s = time.perf_counter() - t0
    arrays = scores.numpy()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "wb") as f:              # (a file object: numpy appends no suffix of its own)
        np.savez(f, **arrays)
    marked = None
    if mask_out is not None:
        mask = low_contribution_mask(h.nodes, scores, max_weight_below, sum_below, pixels_below, unseen).cpu().numpy()
        os.makedirs(os.path.dirname(os.path.abspath(mask_out)), exist_ok=True)
        with open(mask_out, "wb") as f:
            np.save(f, mask)
        marked = int(mask.sum())
    leaves = int((host.nodes[:, 6] == 0).sum())
    return dict(nodes=N, leaves=leaves, views=len(cameras), seen=int((arrays["entries"] > 0).sum()),
                blended=int((arrays["count"] > 0).sum()), marked=marked, tail=G - N, score_s=score_s, read_s=read_s,
                path=out_path, mask_path=mask_out)


def main(argv=None) -> int:
    a = parse_args(sys.argv[1:] if argv is None else list(argv))
    if a is None or missing_path("score_hierarchy", a["in_path"], a["cameras"]):
        return usage_exit(USAGE)
    try:
        cameras = read_cameras(a["cameras"], a["resolution_scale"])
    except (ValueError, OSError) as e:
        return usage_exit(USAGE, f"score_hierarchy: {e}")
    try:
        r = run(a["in_path"], a["out_path"], cameras, a["tau_px"], a["frustum"], a["mask_out"], a["max_weight_below"],
                a["sum_below"], a["pixels_below"], a["unseen"])
    except ValueError as e:
        return check_exit("score_hierarchy", f"{a['in_path']}: {e}")
    mask = "" if r["marked"] is None else f", {r['marked']} leaves marked -> {r['mask_path']}"
    print(f"score_hierarchy: N = {r['nodes']} nodes ({r['leaves']} leaves), {r['views']} views at {a['tau_px']:g} px"
          f"{'' if a['frustum'] else ', no frustum cull'}: {r['seen']} nodes in a cut, {r['blended']} blended into a pixel, "
          f"{r['tail']} rows behind the nodes ignored; scored in {r['score_s']:.2f} s (read {r['read_s']:.2f} s) -> "
          f"{r['path']}{mask}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
