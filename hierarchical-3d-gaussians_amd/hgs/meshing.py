"""Geometry from a hierarchy: depth maps fused into a truncated signed distance volume, a triangle mesh extracted from
it (csrc/tsdf.hip, the rules in csrc/tsdf_rule.h, the spec in tests/tsdf_spec.py)::

    vol = TsdfVolume(lo, hi, voxel=0.05, colour=True)
    fuse_hierarchy(h, cameras, vol)                        # per camera: the surface depth of hgs.picking, integrated
    mesh = vol.extract()                                   # Mesh(vertices, normals, colours, faces), device tensors
    write_mesh_ply("mesh.ply", mesh)

``TsdfVolume.integrate`` takes any depth maps (view-space depth per pixel, 0 where there is no surface) with the cameras
they were made with; ``fuse_hierarchy`` makes them from a hierarchy with ``hgs.picking.read_hierarchy_view`` -- the depth
at which a pixel becomes half opaque.  Both kernels' results equal the numpy spec bit for bit.  ``python -m
hgs.mesh_hierarchy`` is the command.  The volume lives on the GPU: there is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

MAX_SAMPLES = 2 ** 31 - 1                  # of a volume
MAX_EXTRACT_SAMPLES = (2 ** 32 - 1) // 3   # of a volume a mesh is extracted from (32-bit quad offsets)


@dataclass
class Mesh:
    vertices: torch.Tensor              # float32 [V,3] world positions, ascending cell index
    normals: torch.Tensor               # float32 [V,3] unit, towards free space (0 for a zero gradient)
    colours: Optional[torch.Tensor]     # float32 [V,3] or None
    faces: torch.Tensor                 # int32 [F,3], two triangles per quad

    def numpy(self) -> dict:
        out = dict(vertices=self.vertices.cpu().numpy(), normals=self.normals.cpu().numpy(), faces=self.faces.cpu().numpy())
        if self.colours is not None:
            out["colours"] = self.colours.cpu().numpy()
        return out


def volume_dims(lo, hi, voxel):
    """(nx, ny, nz) of the lattice lo + voxel * i that stays inside [lo, hi]: floor((hi - lo) / voxel) + 1 per axis, on
    the float32 values the volume holds."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    voxel = float(np.float32(voxel))
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError(f"voxel must be positive and finite, not {voxel}")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError(f"lo <= hi, both finite, expected; got {lo.tolist()} and {hi.tolist()}")
    return tuple(int(v) for v in np.floor((hi - np.float32(lo).astype(np.float64)) / voxel) + 1)


def fitting_voxel(lo, hi, limit=MAX_EXTRACT_SAMPLES):
    """A voxel size (three significant digits, rounded up) at which [lo, hi] holds at most ``limit`` samples."""
    extent = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    s = float(np.prod(np.maximum(extent, 1e-30)) / limit) ** (1.0 / 3.0)
    for _ in range(200):
        digits = 2 - int(math.floor(math.log10(s)))
        s = math.ceil(s * 10 ** digits) / 10 ** digits
        n = volume_dims(lo, hi, s)
        if n[0] * n[1] * n[2] <= limit:
            return s
        s *= 1.01
    raise ValueError("no voxel size fits")


class TsdfVolume:
    """A dense TSDF volume on the GPU over the lattice ``lo + voxel * i`` inside [lo, hi]: ``tsdf`` [nz,ny,nx] in units
    of ``trunc`` (default 4 voxels), ``weight``, and with ``colour`` [nz,ny,nx,3]."""

    def __init__(self, lo, hi, voxel, trunc=None, colour=False, max_weight=math.inf, device=None):
        from . import _lib
        self._lib = _lib
        if not torch.cuda.is_available():
            raise RuntimeError("TsdfVolume lives on the GPU; no GPU is visible (there is no CPU path; tests/tsdf_spec.py is "
                               "the numpy spec)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.nx, self.ny, self.nz = volume_dims(lo, hi, voxel)
        n = self.nx * self.ny * self.nz
        if n > MAX_SAMPLES:
            raise ValueError(f"{self.nx} x {self.ny} x {self.nz} = {n} samples; at most 2^31 - 1 "
                             f"(a voxel of {fitting_voxel(lo, hi, MAX_SAMPLES):g} fits)")
        self.lo = np.asarray(lo, np.float32).reshape(3)
        self.voxel = float(np.float32(voxel))
        self.trunc = float(np.float32(4.0) * np.float32(voxel)) if trunc is None else float(np.float32(trunc))
        self.max_weight = float(np.float32(max_weight))
        if not (self.trunc > 0.0 and math.isfinite(self.trunc)) or not self.max_weight > 0.0:
            raise ValueError("trunc must be positive and finite, max_weight positive")
        shape = (self.nz, self.ny, self.nx)
        self.tsdf = torch.ones(shape, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.colour = torch.zeros(shape + (3,), dtype=torch.float32, device=self.device) if colour else None

    @property
    def dims(self):
        return self.nx, self.ny, self.nz

    def _struct(self):
        L = self._lib
        return L.TsdfVolume(self.tsdf.data_ptr(), self.weight.data_ptr(), None if self.colour is None else self.colour.data_ptr(),
                            (C.c_float * 3)(*self.lo.tolist()), self.voxel, self.nx, self.ny, self.nz, self.trunc,
                            self.max_weight)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _plane(self, t, shape, what, k):
        if t is None:
            return None
        t = torch.as_tensor(t)
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError(f"{what} {k} must be float32 {list(shape)}, not {t.dtype} {list(t.shape)}")
        return t.to(self.device).contiguous()

    def integrate(self, depths, cams, weights=None, images=None, z_min=None):
        """Fuse views into the volume, in order: ``depths[k]`` float32 [H,W] view-space depth under ``cams[k]`` (an
        object with the fields of ``hgs.synth.Camera``; 0, negative or NaN: no surface at the pixel), ``weights[k]``
        float32 [H,W] or None (1 everywhere), ``images[k]`` float32 [3,H,W] or None (a colour volume only).  Any number of
        views: hgs_tsdf_integrate takes 8 per pass over the volume.  ``z_min``: samples nearer than it are skipped
        (default: each camera's ``znear``).  Asynchronous on the current stream."""
        L = self._lib
        depths, cams = list(depths), list(cams)
        weights = [None] * len(cams) if weights is None else list(weights)
        images = [None] * len(cams) if images is None else list(images)
        if not (len(depths) == len(cams) == len(weights) == len(images)):
            raise ValueError(f"{len(depths)} depths, {len(weights)} weights and {len(images)} images for {len(cams)} cameras")
        if self.colour is None and any(i is not None for i in images):
            raise ValueError("images given, but the volume was made without colour")
        lib = L.lib()
        with torch.cuda.device(self.device):
            for g0 in range(0, len(cams), L.TSDF_MAX_VIEWS):
                views, keep = (L.TsdfView * L.TSDF_MAX_VIEWS)(), []
                group = range(g0, min(g0 + L.TSDF_MAX_VIEWS, len(cams)))
                for slot, k in enumerate(group):
                    cam = cams[k]
                    H, W = int(cam.image_height), int(cam.image_width)
                    d = self._plane(depths[k], (H, W), "depth", k)
                    w = self._plane(weights[k], (H, W), "weight", k)
                    rgb = self._plane(images[k], (3, H, W), "image", k)
                    if d is None:
                        raise ValueError(f"depth {k} is None")
                    keep += [d, w, rgb]
                    m = np.asarray(cam.world_view_transform.detach().cpu().numpy(), np.float32)[:, :3].reshape(12)
                    views[slot] = L.TsdfView(d.data_ptr(), None if w is None else w.data_ptr(),
                                             None if rgb is None else rgb.data_ptr(), W, H, (C.c_float * 12)(*m.tolist()),
                                             float(cam.tanfovx), float(cam.tanfovy),
                                             float(cam.znear if z_min is None else z_min))
                vol = self._struct()
                L.check(lib.hgs_tsdf_integrate(C.byref(vol), views, len(group), self._stream(), self.device.index or 0),
                        "hgs_tsdf_integrate")
        return self

    def extract(self, min_weight=1.0) -> Mesh:
        """The surface-net mesh of the samples seen with weight >= ``min_weight``: one host wait for the two counts, then
        the arrays are allocated and filled asynchronously on the current stream."""
        L = self._lib
        lib = L.lib()
        dev = self.device
        nbytes = lib.hgs_tsdf_extract_tmp_bytes(self.nx, self.ny, self.nz)
        if nbytes == 0:
            raise ValueError(f"{self.nx} x {self.ny} x {self.nz} samples; a mesh is extracted from at most "
                             f"{MAX_EXTRACT_SAMPLES} (the quad offsets are 32-bit)")
        with torch.cuda.device(dev):
            tmp = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            totals = (C.c_int64 * 2)()
            vol = self._struct()
            L.check(lib.hgs_tsdf_extract_plan(C.byref(vol), float(min_weight), tmp.data_ptr(), totals, self._stream(),
                                              dev.index or 0), "hgs_tsdf_extract_plan")
            V, Q = int(totals[0]), int(totals[1])
            # (one spare row: an empty tensor has no address to hand to the call)
            vertices = torch.empty((V + 1, 3), dtype=torch.float32, device=dev)
            normals = torch.empty((V + 1, 3), dtype=torch.float32, device=dev)
            colours = torch.empty((V + 1, 3), dtype=torch.float32, device=dev) if self.colour is not None else None
            faces = torch.empty((2 * Q + 1, 3), dtype=torch.int32, device=dev)
            L.check(lib.hgs_tsdf_extract_apply(C.byref(vol), tmp.data_ptr(), vertices.data_ptr(), normals.data_ptr(),
                                               None if colours is None else colours.data_ptr(), faces.data_ptr(),
                                               self._stream(), dev.index or 0), "hgs_tsdf_extract_apply")
        return Mesh(vertices[:V], normals[:V], None if colours is None else colours[:V], faces[:2 * Q])

    def numpy(self) -> dict:
        out = dict(tsdf=self.tsdf.cpu().numpy(), weight=self.weight.cpu().numpy(), lo=self.lo.copy(),
                   voxel=np.float32(self.voxel), trunc=np.float32(self.trunc), max_weight=np.float32(self.max_weight))
        if self.colour is not None:
            out["colour"] = self.colour.cpu().numpy()
        return out


def surface_depth(readout, min_alpha=0.5):
    """The depth map ``fuse_hierarchy`` integrates: ``median_depth`` where the pixel's ``alpha >= min_alpha``, else 0."""
    return torch.where(readout.alpha < min_alpha, torch.zeros_like(readout.median_depth), readout.median_depth)


def fuse_hierarchy(h, cameras, volume: TsdfVolume, tau_px=0.0, frustum=True, min_alpha=0.5, colour=True):
    """Fuse what ``h`` shows under ``cameras`` into ``volume``; -> ``volume``.  Per camera one
    ``hgs.picking.read_hierarchy_view`` (alpha and median_depth) at the cut of ``tau_px`` pixels, the depth zeroed where
    ``alpha < min_alpha``; with ``colour`` (and a colour volume) also ``hgs.importance.render_hierarchy``'s image.  The
    cull bounds are computed once; the views are integrated 8 per pass over the volume, in order."""
    from . import _lib
    from .importance import _nodes_only, activated, render_hierarchy
    from .picking import read_hierarchy_view
    if not h.nodes.is_cuda:
        raise RuntimeError("fuse_hierarchy works on the GPU: upload the hierarchy first (there is no CPU path)")
    colour = bool(colour) and volume.colour is not None
    bounds = None
    if frustum:
        from .frustum import cull_bounds
        rows = activated(_nodes_only(h))
        bounds = cull_bounds(h.nodes, rows["means3D"], rows["scales"])
    cameras = list(cameras)
    for g0 in range(0, len(cameras), _lib.TSDF_MAX_VIEWS):
        group = cameras[g0:g0 + _lib.TSDF_MAX_VIEWS]
        depths, images = [], []
        for cam in group:
            r = read_hierarchy_view(h, cam, tau_px=tau_px, frustum=frustum, bounds=bounds, want=("alpha", "median_depth"))
            depths.append(surface_depth(r, min_alpha))
            if colour:
                images.append(render_hierarchy(h, cam, tau_px=tau_px, frustum=frustum, bounds=bounds))
        volume.integrate(depths, group, images=images if colour else None)
    return volume


def write_mesh_ply(path, mesh):
    """Binary little-endian PLY of a ``Mesh`` (or its ``numpy()`` dict): vertices x y z nx ny nz (float32), red green blue
    (uint8, the colours clipped to [0, 1]) when the mesh has colours, faces as lists of three int32."""
    m = mesh.numpy() if isinstance(mesh, Mesh) else mesh
    v, n, f = (np.asarray(m[k]) for k in ("vertices", "normals", "faces"))
    c = m.get("colours")
    fields = [(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")]
    if c is not None:
        fields += [(k, "u1") for k in ("red", "green", "blue")]
    vert = np.zeros(v.shape[0], dtype=fields)
    for a, k in enumerate("xyz"):
        vert[k] = v[:, a]
        vert["n" + k] = n[:, a]
    if c is not None:
        c8 = np.rint(np.clip(np.nan_to_num(np.asarray(c, np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
        for a, k in enumerate(("red", "green", "blue")):
            vert[k] = c8[:, a]
    face = np.zeros(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"] = 3
    face["v"] = f
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    header += [f"property {'float' if t == '<f4' else 'uchar'} {k}" for k, t in fields]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vert.tobytes())
        out.write(face.tobytes())
