"""Reader of a trained model's ``point_cloud.ply`` (the reference's ``save_ply`` layout, scene/gaussian_model.py:491-508).

Only what ``save_ply`` writes is accepted: ``binary_little_endian``, one ``vertex`` element of scalar ``float``
properties ``x y z nx ny nz f_dc_0..2 f_rest_0..(3(M-1)-1) opacity scale_0..2 rot_0..3`` (M in {1, 4, 9, 16}).
Anything else is rejected with a message that names what is wrong.  numpy only (no ``plyfile``)."""
from __future__ import annotations

import math

import numpy as np
import torch

from .synth import Scene

_FLOAT_TYPES = ("float", "float32")
_REQUIRED = ("x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2",
             "rot_0", "rot_1", "rot_2", "rot_3")


class PlyFormatError(ValueError):
    pass


def _read_header(f, path):
    if f.readline().strip() != b"ply":
        raise PlyFormatError(f"{path}: not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise PlyFormatError(f"{path}: header without end_header")
        tok = line.decode("ascii", errors="replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1] if len(tok) > 1 else ""
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise PlyFormatError(f"{path}: property before any element")
            if tok[1] == "list":
                raise PlyFormatError(f"{path}: list property '{tok[-1]}' of element '{elements[-1][0]}' "
                                     f"(only scalar float properties are supported)")
            elements[-1][2].append((tok[2], tok[1]))
        elif tok[0] == "end_header":
            return fmt, elements


def read_ply(path) -> Scene:
    """-> activated ``hgs.synth.Scene``: sigmoid opacity [P,1], exp scales, normalised rotations, SH [P,M,3]
    (f_rest is stored channel-major [P,3,M-1] and transposed here)."""
    with open(path, "rb") as f:
        fmt, elements = _read_header(f, path)
        if fmt != "binary_little_endian":
            raise PlyFormatError(f"{path}: format '{fmt}' is not supported (binary_little_endian only)")
        if not elements or elements[0][0] != "vertex":
            raise PlyFormatError(f"{path}: the first element must be 'vertex'")
        _, P, props = elements[0]
        for name, typ in props:
            if typ not in _FLOAT_TYPES:
                raise PlyFormatError(f"{path}: property '{name}' has type '{typ}' (float expected)")
        names = [n for n, _ in props]
        missing = [n for n in _REQUIRED if n not in names]
        if missing:
            raise PlyFormatError(f"{path}: missing properties {', '.join(missing)}")
        n_rest = sum(1 for n in names if n.startswith("f_rest_"))
        M = 1 + n_rest // 3
        if n_rest % 3 or M not in (1, 4, 9, 16):
            raise PlyFormatError(f"{path}: {n_rest} f_rest properties (0, 9, 24 or 45 expected)")
        missing = [f"f_rest_{i}" for i in range(n_rest) if f"f_rest_{i}" not in names]
        if missing:
            raise PlyFormatError(f"{path}: missing properties {', '.join(missing)}")
        dt = np.dtype([(n, "<f4") for n in names])
        data = np.fromfile(f, dtype=dt, count=P)
    if data.shape[0] != P:
        raise PlyFormatError(f"{path}: {data.shape[0]} of {P} vertices present (file truncated)")
    col = lambda *ns: torch.from_numpy(np.stack([data[n] for n in ns], 1))
    xyz = col("x", "y", "z")
    shs = torch.empty(P, M, 3)
    shs[:, 0] = col("f_dc_0", "f_dc_1", "f_dc_2")
    if M > 1:
        shs[:, 1:] = col(*[f"f_rest_{i}" for i in range(n_rest)]).reshape(P, 3, M - 1).transpose(1, 2)
    op = torch.sigmoid(col("opacity"))
    sc = torch.exp(col("scale_0", "scale_1", "scale_2"))
    rot = torch.nn.functional.normalize(col("rot_0", "rot_1", "rot_2", "rot_3"), dim=1)
    return Scene(xyz.contiguous(), sc.contiguous(), rot.contiguous(), op.contiguous(), shs.contiguous(),
                 int(math.isqrt(M)) - 1)
