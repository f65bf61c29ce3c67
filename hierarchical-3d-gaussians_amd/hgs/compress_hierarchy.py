"""Half-precision copy of a hierarchy file: ``<in.hier>`` -> ``<out.hier>``.

    python -m hgs.compress_hierarchy <in.hier> <out.hier>

Reads the file (load_hierarchy: any of the layouts it accepts, 16 SH coefficients) and writes it with
``write_hierarchy(..., half=True)``: the upstream tools' compressed variant -- positions stay float32; rotations,
log-scales, alpha and SH become IEEE half under the narrowing rule of include/hgs.h (round to nearest even, a finite
value beyond +-65504 saturates) -- 124 bytes per Gaussian instead of 236.  Nodes and boxes are copied bit for bit, and
so is the count of rows: rows behind the node rows (the skybox tail save_hier appends) are kept.  Compressing a
compressed file reproduces it byte for byte.  No GPU is needed.  Printed: the two file sizes."""
from __future__ import annotations

import os
import sys

from ._hier_command import check_exit, missing_path, usage_exit, write_output

USAGE = "usage: python -m hgs.compress_hierarchy <in.hier> <out.hier>"


def run(in_path, out_path) -> dict:
    """Read, write with ``half=True``; -> figures of the run."""
    from gaussian_hierarchy._C import load_hierarchy
    arrays = xyz, shs, _, _, _, nodes, _ = load_hierarchy(in_path)
    if shs.shape[1] != 16:
        raise ValueError(f"{in_path}: {shs.shape[1]} SH coefficients per Gaussian; the compressed layout stores exactly 16")
    write_output(out_path, arrays, half=True)
    return dict(rows=int(xyz.shape[0]), nodes=int(nodes.shape[0]), bytes_in=os.path.getsize(in_path),
                bytes_out=os.path.getsize(out_path), path=out_path)


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) != 2 or missing_path("compress_hierarchy", argv[0]):
        return usage_exit(USAGE)
    if os.path.exists(argv[1]) and os.path.samefile(argv[0], argv[1]):
        return usage_exit(USAGE, f"compress_hierarchy: {argv[1]} is the input file; refusing to overwrite it")
    try:
        r = run(*argv)
    except ValueError as e:
        return check_exit("compress_hierarchy", e)
    print(f"compress_hierarchy: {r['rows']} rows ({r['rows'] - r['nodes']} behind the {r['nodes']} node rows kept), "
          f"{r['bytes_in']} bytes -> {r['bytes_out']} bytes ({100.0 * r['bytes_out'] / max(r['bytes_in'], 1):.1f} %) -> "
          f"{r['path']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
