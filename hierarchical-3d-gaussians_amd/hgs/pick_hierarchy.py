"""Point at a render of a hierarchy file and get the nodes behind the pixels: ``<in.hier>`` -> ids on stdout.

    python -m hgs.pick_hierarchy <in.hier> --cameras <cameras.json> --camera K
        (--rect x0 y0 x1 y1 | --pixel x y | --pixel-mask <m.npy>) [--which front|back|heaviest|median]...
        [--tau-px PX] [--no-frustum] [--resolution-scale S]
        [--ids-out <ids.npy>] [--mask-out <mask.npy>] [--readout-out <r.npz>]

"Delete what I see in this rectangle", "which node is this floater", "how deep is the surface here".  Camera K of the
``cameras.json`` (the file ``python -m hgs.score_hierarchy`` reads) is rendered at the cut of ``--tau-px`` pixels
(default 0: the leaves) and read per pixel: the node in front, the last one, the one that
carries the pixel, the one at which the pixel becomes half opaque.  Steps:

  1. read the cameras (``--resolution-scale S`` divides every camera's width and height by S), take camera K, check
     the region against its image; then the file (load_hierarchy: any of the layouts it accepts);
  2. ``hgs.picking.read_hierarchy_view`` on the N node rows, ``hgs.picking.pick`` of the planes ``--which`` (default
     ``front``; repeatable) inside the region: ``--rect`` is half-open, ``--pixel x y`` the one pixel, ``--pixel-mask``
     a bool / uint8 [H, W] ``.npy``;
  3. ``--ids-out`` writes the picked ids (int64), ``--mask-out`` the uint8 [N] mask of the leaves below them
     (``hgs.picking.leaves_below``: what ``python -m hgs.prune_hierarchy --mask`` reads), ``--readout-out`` the planes.

Printed: one sentence with the counts, then one line per picked id with its tree depth; for ``--pixel`` also the world
point where the pixel becomes half opaque.  Usage errors exit with 2; a hierarchy, camera or mask file that cannot be
used is named, nothing is written, exit status 1."""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np

from ._hier_command import check_exit, missing_path, read_input, upload, usage_exit, walk_args
from .score_hierarchy import read_cameras

USAGE = ("usage: python -m hgs.pick_hierarchy <in.hier> --cameras <cameras.json> --camera K "
         "(--rect x0 y0 x1 y1 | --pixel x y | --pixel-mask <m.npy>) [--which front|back|heaviest|median]... "
         "[--tau-px PX] [--no-frustum] [--resolution-scale S] [--ids-out <ids.npy>] [--mask-out <mask.npy>] "
         "[--readout-out <r.npz>]")
SINGLE = ("--cameras", "--camera", "--rect", "--pixel", "--pixel-mask", "--tau-px", "--resolution-scale", "--ids-out",
          "--mask-out", "--readout-out")
OPTIONS = {**dict.fromkeys(SINGLE, 1), "--rect": 4, "--pixel": 2, "--which": 1, "--no-frustum": 0}
WHICH = ("front", "back", "heaviest", "median")
MAX_LINES = 200          # picked ids printed one per line; the rest are counted


def _ints(tokens):
    return [int(t) for t in tokens]         # (ValueError on "1.5", "x")


def parse_args(argv):
    """-> dict(in_path, cameras, camera, rect, pixel, pixel_mask, which, tau_px, frustum, resolution_scale, ids_out,
    mask_out, readout_out) or None for a usage error: an option but --which given twice, no --cameras, no --camera, not
    exactly one region, an empty or inverted --rect, a negative pixel, an unknown or repeated plane."""
    walked = walk_args(argv, OPTIONS)
    if walked is None or any(len(walked[1][k]) > 1 for k in SINGLE):
        return None
    pos, seen = walked
    one = {k: seen[k][0] if seen[k] else None for k in SINGLE}
    first = lambda k: None if one[k] is None else one[k][0]
    try:
        camera = None if one["--camera"] is None else _ints(one["--camera"])[0]
        rect = None if one["--rect"] is None else tuple(_ints(one["--rect"]))
        pixel = None if one["--pixel"] is None else tuple(_ints(one["--pixel"]))
        tau_px = 0.0 if one["--tau-px"] is None else float(first("--tau-px"))
        scale = 1.0 if one["--resolution-scale"] is None else float(first("--resolution-scale"))
    except ValueError:
        return None
    if len(pos) != 1 or one["--cameras"] is None or camera is None or camera < 0:
        return None
    if sum(x is not None for x in (rect, pixel, first("--pixel-mask"))) != 1:
        return None
    if rect is not None and not (rect[0] < rect[2] and rect[1] < rect[3]):
        return None
    if pixel is not None and min(pixel) < 0:
        return None
    if not tau_px >= 0.0 or not (scale > 0.0 and scale != math.inf):
        return None
    which = tuple(v[0] for v in seen["--which"]) or ("front",)
    if any(w not in WHICH for w in which) or len(set(which)) != len(which):
        return None
    return dict(in_path=pos[0], cameras=first("--cameras"), camera=camera, rect=rect, pixel=pixel,
                pixel_mask=first("--pixel-mask"), which=which, tau_px=tau_px, frustum=not seen["--no-frustum"],
                resolution_scale=scale, ids_out=first("--ids-out"), mask_out=first("--mask-out"),
                readout_out=first("--readout-out"))


def region_of(a, cam):
    """The region ``hgs.picking.pick`` takes, checked against the camera's image; ValueError naming what does not fit."""
    W, H = int(cam.image_width), int(cam.image_height)
    if a["pixel"] is not None:
        x, y = a["pixel"]
        if x >= W or y >= H:
            raise ValueError(f"pixel ({x}, {y}) lies outside the {W} x {H} image of camera {a['camera']}")
        return (x, y, x + 1, y + 1)
    if a["rect"] is not None:
        x0, y0, x1, y1 = a["rect"]
        if x1 <= 0 or y1 <= 0 or x0 >= W or y0 >= H:
            raise ValueError(f"rectangle {a['rect']} does not meet the {W} x {H} image of camera {a['camera']}")
        return a["rect"]
    path = a["pixel_mask"]
    try:
        m = np.load(path, allow_pickle=False)
    except (ValueError, OSError) as e:
        raise ValueError(f"{path} is no .npy array ({e})") from None
    if m.dtype not in (np.bool_, np.uint8) or m.shape != (H, W):
        raise ValueError(f"{path}: bool or uint8 [{H}, {W}] expected for camera {a['camera']}, got {m.dtype} {list(m.shape)}")
    return np.ascontiguousarray(m)


def _save(path, writer):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:                  # (a file object: numpy appends no suffix of its own)
        writer(f)


def run(in_path, cam, region, which=("front",), tau_px=0.0, frustum=True, ids_out=None, mask_out=None,
        readout_out=None, pixel=None) -> dict:
    """Read, render, pick, write; -> figures of the run.  ``cam``: a ``hgs.synth.Camera``; ``region`` as for
    ``hgs.picking.pick``; ``pixel``: (x, y) whose world point is wanted, or None."""
    import torch
    from .picking import leaves_below, node_depth_image, pick, read_hierarchy_view, world_points
    host, N, G, read_s = read_input("pick_hierarchy", in_path)
    h = upload(host, rows=N)
    t0 = time.perf_counter()
    region = torch.from_numpy(region) if isinstance(region, np.ndarray) else region
    r = read_hierarchy_view(h, cam, tau_px=tau_px, frustum=frustum)
    ids = pick(r, region, which)
    depths = node_depth_image(ids, h.nodes)
    mask = leaves_below(h.nodes, ids)
    point = None
    if pixel is not None:
        point = world_points(r, cam)[pixel[1], pixel[0]].cpu().numpy()
    torch.cuda.synchronize()
    run_s = time.perf_counter() - t0
    ids_np, mask_np = ids.cpu().numpy(), mask.cpu().numpy()
    if ids_out is not None:
        _save(ids_out, lambda f: np.save(f, ids_np))
    if mask_out is not None:
        _save(mask_out, lambda f: np.save(f, mask_np))
    if readout_out is not None:
        _save(readout_out, lambda f: np.savez(f, **r.numpy()))
    return dict(nodes=N, tail=G - N, ids=ids_np, depths=depths.cpu().numpy(), leaves=int(mask_np.sum()), point=point,
                covered=int((r.count > 0).sum()), run_s=run_s, read_s=read_s)


def main(argv=None) -> int:
    a = parse_args(sys.argv[1:] if argv is None else list(argv))
    if a is None or missing_path("pick_hierarchy", a["in_path"], a["cameras"], a["pixel_mask"]):
        return usage_exit(USAGE)
    try:
        cameras = read_cameras(a["cameras"], a["resolution_scale"])
    except (ValueError, OSError) as e:
        return usage_exit(USAGE, f"pick_hierarchy: {e}")
    if a["camera"] >= len(cameras):
        return usage_exit(USAGE, f"pick_hierarchy: --camera {a['camera']}: {a['cameras']} holds {len(cameras)} cameras")
    cam = cameras[a["camera"]]
    try:
        region = region_of(a, cam)
    except ValueError as e:
        return check_exit("pick_hierarchy", str(e))
    try:
        r = run(a["in_path"], cam, region, a["which"], a["tau_px"], a["frustum"], a["ids_out"], a["mask_out"],
                a["readout_out"], a["pixel"])
    except ValueError as e:
        return check_exit("pick_hierarchy", f"{a['in_path']}: {e}")
    what = (f"pixel {a['pixel']}" if a["pixel"] is not None else f"rectangle {a['rect']}" if a["rect"] is not None
            else f"the mask {a['pixel_mask']}")
    outs = [p for p in (a["ids_out"], a["mask_out"], a["readout_out"]) if p is not None]
    print(f"pick_hierarchy: N = {r['nodes']} nodes, camera {a['camera']} ({cam.image_width} x {cam.image_height}) at "
          f"{a['tau_px']:g} px{'' if a['frustum'] else ', no frustum cull'}: {r['covered']} pixels show a row; "
          f"{len(r['ids'])} nodes picked by {', '.join(a['which'])} in {what}, {r['leaves']} leaves below them, "
          f"{r['tail']} rows behind the nodes ignored; read out in {r['run_s']:.2f} s (read {r['read_s']:.2f} s)"
          f"{' -> ' + ', '.join(outs) if outs else ''}", flush=True)
    for i, d in list(zip(r["ids"], r["depths"]))[:MAX_LINES]:
        print(f"node {int(i)} depth {int(d)}")
    if len(r["ids"]) > MAX_LINES:
        print(f"... and {len(r['ids']) - MAX_LINES} more")
    if r["point"] is not None:
        p = r["point"]
        print("world point: none (the pixel never becomes half opaque)" if np.isnan(p).any()
              else f"world point: {p[0]:.6g} {p[1]:.6g} {p[2]:.6g}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
