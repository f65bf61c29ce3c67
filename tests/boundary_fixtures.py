"""The boundary fixtures tests/golden/boundary_*.npz (written by tests/golden/make_boundary_golden.py, whose docstring
holds the key schema) and the torch restatement of render_post's LOD lerp shared by the GPU tests."""
import glob
import os

import numpy as np
import torch

from harness.recorder import ARGS, LOD_FIELDS, SETTINGS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TENSOR_FIELDS = ("bg", "viewmatrix", "projmatrix", "campos") + LOD_FIELDS
FULL = ("xyz", "scaling", "rotation", "opacity", "features")
# the op's argument that each full array becomes
ROW_ARG = dict(xyz="means3D", scaling="scales", rotation="rotations", opacity="opacities", features="shs")


def files():
    return sorted(glob.glob(os.path.join(GOLDEN, "boundary_*.npz")))


def load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def records(z, kind):
    """Prefixes of the records of one kind ("op", "lod", "cut", "knn") in a loaded fixture, in index order."""
    ids = {k.split("__")[0][len(kind):] for k in z if k.startswith(kind)}
    return [f"{kind}{i}" for i in sorted(int(i) for i in ids if i.isdigit())]


def cases(kind):
    """[(file name, record prefix)] of every record of ``kind`` in every fixture file."""
    return [(os.path.basename(f), pre) for f in files() for pre in records(load(f), kind)]


def settings(z, op, device):
    """The op call's GaussianRasterizationSettings keywords, each tensor where the reference puts it: the render_post LOD
    fields that are empty stay on the CPU (gaussian_renderer/__init__.py:145-148, 244-245), everything else goes to
    ``device``."""
    site = int(z[f"{op}__site"])
    out = {}
    for f in SETTINGS:
        v = z[f"{op}__set__{f}"]
        if f not in TENSOR_FIELDS:
            out[f] = v.item()
            continue
        t = torch.from_numpy(v.copy())
        out[f] = t if (site == 1 and f in LOD_FIELDS and t.numel() == 0) else t.to(device)
    return out


def args(z, op, device):
    """The eight call arguments on ``device`` (None where the reference passed None)."""
    return {n: (torch.from_numpy(z[f"{op}__arg__{n}"].copy()).to(device) if f"{op}__arg__{n}" in z else None)
            for n in ARGS}


def lod_lerp(attrs, r, p, w):
    """render_post's python-side LOD interpolation (gaussian_renderer/__init__.py:199-218) restated in torch: row i is
    w_i * a[r_i] + (1 - w_i) * a[p_i] (two rounded products, one rounded sum), the parent quaternion negated first when
    its dot with the node's is strictly negative.  ``attrs``: {name: [G, ...] tensor} with the quaternions under
    "rotation"; r, p: int64 [n]; w: float32 [n].  Returns {name: [n, ...] rows}."""
    t, ti = w.unsqueeze(1), (1 - w).unsqueeze(1)
    out = {}
    for k, a in attrs.items():
        if k == "rotation":
            q, qp = a[r], a[p]
            # q . qp summed left to right, one rounding per operation (the order of lod_gather.hip); only its sign is
            # used, and the fixtures keep it away from zero unless it is exactly zero
            d = ((q[:, 0] * qp[:, 0] + q[:, 1] * qp[:, 1]) + q[:, 2] * qp[:, 2]) + q[:, 3] * qp[:, 3]
            out[k] = t * q + ti * torch.where((d < 0).unsqueeze(1), -qp, qp)
        elif a.dim() == 3:
            out[k] = t.unsqueeze(2) * a[r] + ti.unsqueeze(2) * a[p]
        else:
            out[k] = t * a[r] + ti * a[p]
    return out
