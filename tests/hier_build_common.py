"""Shared by the hierarchy-builder tests: a PLY in the reference's save_ply layout."""
import numpy as np

from harness import ply_to_hier            # noqa: F401  (puts the plyfile shim on sys.path)


def save_ply_layout(path, P, M, seed=0, xyz=None):
    """A PLY in the reference's save_ply layout (scene/gaussian_model.py:491-508), written with the plyfile shim:
    raw (pre-activation) parameters, f_rest channel-major [P,3,M-1]."""
    from plyfile import PlyData, PlyElement
    rng = np.random.default_rng(seed)
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    names += [f"f_rest_{i}" for i in range(3 * (M - 1))]
    names += ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    el = np.zeros(P, dtype=[(n, "f4") for n in names])
    for n in names:
        el[n] = rng.standard_normal(P).astype(np.float32)
    for n in ("nx", "ny", "nz"):
        el[n] = 0.0
    for n in ("scale_0", "scale_1", "scale_2"):
        el[n] = (rng.uniform(-6.0, -2.0, P)).astype(np.float32)
    if xyz is not None:
        for a, n in enumerate(("x", "y", "z")):
            el[n] = xyz[:, a]
    PlyData([PlyElement.describe(el, "vertex")]).write(path)
    return el
