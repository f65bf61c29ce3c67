"""Per-node error of a hierarchy file over a set of cameras: ``<in.hier>`` -> ``<out.npz>``.

    python -m hgs.lod_error <in.hier> <out.npz> --cameras <cameras.json> --tau-px PX
        [--ref-tau-px PX | --targets <dir>] [--no-frustum] [--resolution-scale S]

Which interior nodes are bad stand-ins for their subtrees?  Every camera of the ``cameras.json`` (the file
``python -m hgs.score_hierarchy`` reads) is rendered at the cut of ``--tau-px`` pixels and compared with a target: the
same hierarchy rendered at ``--ref-tau-px`` (default 0: the leaves), or, with ``--targets <dir>``, the image
``<dir>/<k>.npy`` (float32 [3, H, W]) for camera k -- with ground-truth images a per-row photometric error.  Every
pixel's ``e = mean over the channels of |render - target|`` is handed to the cut entries that blended the pixel, weighted
by their blending weights ``w = alpha * T``.  Steps:

  1. read the cameras (``--resolution-scale S`` divides every camera's width and height by S) and, with ``--targets``,
     every target; then the file (load_hierarchy: any of the layouts it accepts);
  2. ``hgs.importance.lod_error_hierarchy`` or ``error_hierarchy`` on the N node rows;
  3. write ``err`` float64 [N] (the sum of ``w e`` over views and pixels), ``wsum`` float64 [N] (the sum of ``w``:
     ``err / wsum`` is the mean error under a node), ``entries`` int64 [N] and ``views`` to the ``.npz``.

Printed: one sentence with the counts.  Usage errors exit with 2; a hierarchy, camera or target file that cannot be used
is named, nothing is written, exit status 1."""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np

from ._hier_command import check_exit, missing_path, read_input, upload, usage_exit, walk_args
from .score_hierarchy import read_cameras

USAGE = ("usage: python -m hgs.lod_error <in.hier> <out.npz> --cameras <cameras.json> --tau-px PX "
         "[--ref-tau-px PX | --targets <dir>] [--no-frustum] [--resolution-scale S]")
SINGLE = ("--cameras", "--tau-px", "--ref-tau-px", "--targets", "--resolution-scale")
OPTIONS = {**dict.fromkeys(SINGLE, 1), "--no-frustum": 0}


def parse_args(argv):
    """-> dict(in_path, out_path, cameras, tau_px, ref_tau_px, targets, frustum, resolution_scale) or None for a usage
    error: an option given twice, no --cameras, no --tau-px, --ref-tau-px together with --targets.  ``ref_tau_px`` is
    None with --targets and 0.0 by default."""
    walked = walk_args(argv, OPTIONS)
    if walked is None or any(len(walked[1][k]) > 1 for k in SINGLE):
        return None
    pos, seen = walked
    one = {k: seen[k][0][0] if seen[k] else None for k in SINGLE}
    try:
        num = {k: (None if one[k] is None else float(one[k])) for k in ("--tau-px", "--ref-tau-px", "--resolution-scale")}
    except ValueError:
        return None
    if len(pos) != 2 or one["--cameras"] is None or num["--tau-px"] is None:
        return None
    if any(x is not None and x != x for x in num.values()):
        return None
    if one["--targets"] is not None and num["--ref-tau-px"] is not None:
        return None
    scale = 1.0 if num["--resolution-scale"] is None else num["--resolution-scale"]
    ref = None if one["--targets"] is not None else (0.0 if num["--ref-tau-px"] is None else num["--ref-tau-px"])
    if not num["--tau-px"] >= 0.0 or (ref is not None and not ref >= 0.0) or not (scale > 0.0 and scale != math.inf):
        return None
    return dict(in_path=pos[0], out_path=pos[1], cameras=one["--cameras"], tau_px=num["--tau-px"], ref_tau_px=ref,
                targets=one["--targets"], frustum=not seen["--no-frustum"], resolution_scale=scale)


def read_targets(directory, cameras):
    """``<directory>/<k>.npy`` for every camera k -> a list of float32 [3, H, W] host tensors; ValueError naming the
    first file that is missing, unreadable or not of its camera's shape."""
    import torch
    out = []
    for k, cam in enumerate(cameras):
        path = os.path.join(directory, f"{k}.npy")
        if not os.path.exists(path):
            raise ValueError(f"{path} does not exist (the target of camera {k})")
        try:
            a = np.load(path, allow_pickle=False)
        except (ValueError, OSError) as e:
            raise ValueError(f"{path} is no .npy array ({e})") from None
        want = (3, int(cam.image_height), int(cam.image_width))
        if a.dtype != np.float32 or a.shape != want:
            raise ValueError(f"{path}: float32 {list(want)} expected for camera {k}, got {a.dtype} {list(a.shape)}")
        out.append(torch.from_numpy(np.ascontiguousarray(a)))
    return out


def run(in_path, out_path, cameras, tau_px, ref_tau_px=0.0, targets=None, frustum=True) -> dict:
    """Read, attribute, write; -> figures of the run.  ``cameras``: a list of ``hgs.synth.Camera``; ``targets``: None
    (the hierarchy at ``ref_tau_px``) or one float32 [3, H, W] tensor per camera."""
    import torch
    from .importance import error_hierarchy, lod_error_hierarchy
    host, N, G, read_s = read_input("lod_error", in_path)
    h = upload(host, rows=N)
    t0 = time.perf_counter()
    if targets is None:
        att = lod_error_hierarchy(h, cameras, tau_px, ref_tau_px=ref_tau_px, frustum=frustum)
    else:
        att = error_hierarchy(h, cameras, targets, tau_px=tau_px, frustum=frustum)
    torch.cuda.synchronize()
    run_s = time.perf_counter() - t0
    a = att.numpy()
    arrays = dict(err=np.ascontiguousarray(a["acc"][:, 0]), wsum=a["wsum"], entries=a["entries"], views=a["views"])
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "wb") as f:              # (a file object: numpy appends no suffix of its own)
        np.savez(f, **arrays)
    total_w = float(arrays["wsum"].sum())
    return dict(nodes=N, views=len(cameras), seen=int((arrays["entries"] > 0).sum()),
                carrying=int((arrays["err"] > 0).sum()), mean=float(arrays["err"].sum()) / total_w if total_w else 0.0,
                tail=G - N, run_s=run_s, read_s=read_s, path=out_path)


def main(argv=None) -> int:
    a = parse_args(sys.argv[1:] if argv is None else list(argv))
    if a is None or missing_path("lod_error", a["in_path"], a["cameras"], a["targets"]):
        return usage_exit(USAGE)
    try:
        cameras = read_cameras(a["cameras"], a["resolution_scale"])
    except (ValueError, OSError) as e:
        return usage_exit(USAGE, f"lod_error: {e}")
    try:
        targets = None if a["targets"] is None else read_targets(a["targets"], cameras)
    except ValueError as e:
        return check_exit("lod_error", str(e))
    try:
        r = run(a["in_path"], a["out_path"], cameras, a["tau_px"], a["ref_tau_px"], targets, a["frustum"])
    except ValueError as e:
        return check_exit("lod_error", f"{a['in_path']}: {e}")
    against = f"the targets of {a['targets']}" if a["targets"] is not None else f"the cut at {a['ref_tau_px']:g} px"
    print(f"lod_error: N = {r['nodes']} nodes, {r['views']} views at {a['tau_px']:g} px against {against}"
          f"{'' if a['frustum'] else ', no frustum cull'}: {r['seen']} nodes in a cut, {r['carrying']} carry an error, "
          f"weighted mean {r['mean']:.3e}, {r['tail']} rows behind the nodes ignored; attributed in {r['run_s']:.2f} s "
          f"(read {r['read_s']:.2f} s) -> {r['path']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
