"""Look at per-node values of a hierarchy file as an image: ``<in.hier>`` + values -> ``<image.npy>``.

    python -m hgs.paint_hierarchy <in.hier> --cameras <cameras.json> --camera K
        (--values <v.npy> | --builtin level|extent|opacity | --lod-error <err.npz>)
        [--tau-px PX] [--no-frustum] [--resolution-scale S] [--normalize] [--background v ...] --out <image.npy>

"Where in the picture are the nodes that stand in badly for their subtrees", "which tree levels does this cut show".
Camera K of the ``cameras.json`` (the file ``python -m hgs.score_hierarchy`` reads) is rendered at the cut of
``--tau-px`` pixels (default 0: the leaves) and a value per node is blended into it with the render's own weights
``w = alpha * T``.  Steps:

  1. read the cameras (``--resolution-scale S`` divides every camera's width and height by S), take camera K; then the
     values: ``--values`` a float32 / float64 ``.npy`` [N] or [N, C]; ``--builtin`` the tree level, the box extent or
     the opacity of every node; ``--lod-error`` the ``.npz`` of ``python -m hgs.lod_error`` as ``err / wsum`` (NaN
     where a node was never blended: it shows wherever the cut blends such a node); then the file (load_hierarchy: any
     of the layouts it accepts);
  2. ``hgs.painting.paint_hierarchy_view`` on the N node rows; ``--normalize`` divides by the sum of the weights (the
     weighted mean under the pixel; NaN where no node is blended), ``--background`` takes one value or one per channel
     (as many tokens as follow it up to the next option);
  3. write float32 [C, H, W] to ``--out``.

Printed: one sentence with the counts.  Usage errors exit with 2; a hierarchy, camera or value file that cannot be used
is named, nothing is written, exit status 1."""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np

from ._hier_command import check_exit, missing_path, read_input, upload, usage_exit, walk_args
from .score_hierarchy import read_cameras

USAGE = ("usage: python -m hgs.paint_hierarchy <in.hier> --cameras <cameras.json> --camera K "
         "(--values <v.npy> | --builtin level|extent|opacity | --lod-error <err.npz>) [--tau-px PX] [--no-frustum] "
         "[--resolution-scale S] [--normalize] [--background v ...] --out <image.npy>")
SINGLE = ("--cameras", "--camera", "--values", "--builtin", "--lod-error", "--tau-px", "--resolution-scale", "--out")
FLAGS = ("--no-frustum", "--normalize")
BUILTINS = ("level", "extent", "opacity")


def _split_background(argv):
    """``--background v ...`` takes the tokens up to the next option: -> (argv without it, its values or None), or None
    when it stands twice, has no token, or one that is no finite number."""
    argv = list(argv)
    if "--background" not in argv:
        return argv, None
    i = argv.index("--background")
    j = i + 1
    while j < len(argv) and not argv[j].startswith("--"):
        j += 1
    rest = argv[:i] + argv[j:]
    if "--background" in rest or j == i + 1:
        return None
    try:
        vals = tuple(float(t) for t in argv[i + 1:j])
    except ValueError:
        return None
    if not all(math.isfinite(v) for v in vals):
        return None
    return rest, vals


def parse_args(argv):
    """-> dict(in_path, cameras, camera, values, builtin, lod_error, tau_px, frustum, resolution_scale, normalize,
    background, out_path) or None for a usage error: an option given twice, no --cameras, no --camera, no --out, not
    exactly one source of values, an unknown --builtin, a --background without finite numbers."""
    split = _split_background(argv)
    if split is None:
        return None
    argv, background = split
    walked = walk_args(argv, {**dict.fromkeys(SINGLE, 1), **dict.fromkeys(FLAGS, 0)})
    if walked is None or any(len(walked[1][k]) > 1 for k in SINGLE + FLAGS):
        return None
    pos, seen = walked
    one = {k: seen[k][0][0] if seen[k] else None for k in SINGLE}
    try:
        camera = None if one["--camera"] is None else int(one["--camera"])
        tau_px = 0.0 if one["--tau-px"] is None else float(one["--tau-px"])
        scale = 1.0 if one["--resolution-scale"] is None else float(one["--resolution-scale"])
    except ValueError:
        return None
    if len(pos) != 1 or one["--cameras"] is None or camera is None or camera < 0 or one["--out"] is None:
        return None
    if sum(one[k] is not None for k in ("--values", "--builtin", "--lod-error")) != 1:
        return None
    if one["--builtin"] is not None and one["--builtin"] not in BUILTINS:
        return None
    if not tau_px >= 0.0 or not (scale > 0.0 and scale != math.inf):
        return None
    return dict(in_path=pos[0], cameras=one["--cameras"], camera=camera, values=one["--values"],
                builtin=one["--builtin"], lod_error=one["--lod-error"], tau_px=tau_px, frustum=not seen["--no-frustum"],
                resolution_scale=scale, normalize=bool(seen["--normalize"]), background=background,
                out_path=one["--out"])


def read_values(a):
    """The host array of ``--values`` / ``--lod-error`` (None for ``--builtin``); ValueError naming what cannot be used."""
    from .painting import error_per_weight
    if a["values"] is not None:
        path = a["values"]
        try:
            v = np.load(path, allow_pickle=False)
        except (ValueError, OSError) as e:
            raise ValueError(f"{path} is no .npy array ({e})") from None
        if v.dtype not in (np.float32, np.float64) or v.ndim not in (1, 2) or v.size == 0:
            raise ValueError(f"{path}: float32 or float64 [N] or [N, C] expected, got {v.dtype} {list(v.shape)}")
        return np.ascontiguousarray(v, dtype=np.float32)
    if a["lod_error"] is not None:
        path = a["lod_error"]
        try:
            with np.load(path, allow_pickle=False) as z:
                if "err" not in z.files or "wsum" not in z.files:
                    raise ValueError("it holds no err and wsum (the arrays python -m hgs.lod_error writes)")
                att = dict(err=z["err"], wsum=z["wsum"])
            return error_per_weight(att).numpy()
        except (ValueError, OSError) as e:
            raise ValueError(f"{path} cannot be used ({e})") from None
    return None


def builtin_values(name, h):
    from .painting import node_extents, node_levels, node_opacities
    return {"level": lambda: node_levels(h.nodes), "extent": lambda: node_extents(h.boxes),
            "opacity": lambda: node_opacities(h)}[name]()


def run(in_path, cam, out_path, values=None, builtin=None, tau_px=0.0, frustum=True, normalize=False,
        background=None) -> dict:
    """Read, render, paint, write; -> figures of the run.  ``cam``: a ``hgs.synth.Camera``; ``values``: a host array [N]
    or [N, C], or None with ``builtin`` one of ``BUILTINS``."""
    import torch
    from .painting import paint_hierarchy_view
    host, N, G, read_s = read_input("paint_hierarchy", in_path)
    if values is not None and values.shape[0] != N:
        raise ValueError(f"{values.shape[0]} values for N = {N} nodes")
    h = upload(host, rows=N)
    t0 = time.perf_counter()
    v = builtin_values(builtin, h) if values is None else torch.from_numpy(values)
    C = 1 if v.dim() == 1 else int(v.shape[1])
    if background is not None and len(background) not in (1, C):
        raise ValueError(f"{len(background)} background values for {C} channels (one, or one per channel)")
    img = paint_hierarchy_view(h, cam, v, tau_px=tau_px, frustum=frustum, background=background, normalize=normalize)
    torch.cuda.synchronize()
    run_s = time.perf_counter() - t0
    img_np = img.cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "wb") as f:              # (a file object: numpy appends no suffix of its own)
        np.save(f, img_np)
    finite = np.isfinite(img_np)
    return dict(nodes=N, tail=G - N, channels=C, finite=int(finite.all(axis=0).sum()),
                lo=float(img_np[finite].min()) if finite.any() else math.nan,
                hi=float(img_np[finite].max()) if finite.any() else math.nan, run_s=run_s, read_s=read_s, path=out_path)


def main(argv=None) -> int:
    a = parse_args(sys.argv[1:] if argv is None else list(argv))
    if a is None or missing_path("paint_hierarchy", a["in_path"], a["cameras"], a["values"], a["lod_error"]):
        return usage_exit(USAGE)
    try:
        cameras = read_cameras(a["cameras"], a["resolution_scale"])
    except (ValueError, OSError) as e:
        return usage_exit(USAGE, f"paint_hierarchy: {e}")
    if a["camera"] >= len(cameras):
        return usage_exit(USAGE, f"paint_hierarchy: --camera {a['camera']}: {a['cameras']} holds {len(cameras)} cameras")
    cam = cameras[a["camera"]]
    try:
        values = read_values(a)
    except ValueError as e:
        return check_exit("paint_hierarchy", str(e))
    try:
        r = run(a["in_path"], cam, a["out_path"], values, a["builtin"], a["tau_px"], a["frustum"], a["normalize"],
                a["background"])
    except ValueError as e:
        return check_exit("paint_hierarchy", f"{a['in_path']}: {e}")
    what = (f"the values of {a['values']}" if a["values"] is not None else f"err / wsum of {a['lod_error']}"
            if a["lod_error"] is not None else f"the nodes' {a['builtin']}")
    print(f"paint_hierarchy: N = {r['nodes']} nodes, camera {a['camera']} ({cam.image_width} x {cam.image_height}) at "
          f"{a['tau_px']:g} px{'' if a['frustum'] else ', no frustum cull'}: {what}, {r['channels']} channels"
          f"{', normalized' if a['normalize'] else ''}; {r['finite']} finite pixels in [{r['lo']:.6g}, {r['hi']:.6g}], "
          f"{r['tail']} rows behind the nodes ignored; painted in {r['run_s']:.2f} s (read {r['read_s']:.2f} s) "
          f"-> {r['path']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
