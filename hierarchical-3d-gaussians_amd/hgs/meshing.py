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
    cells: Optional[torch.Tensor] = None    # int32 [V,3]: the lattice cell of every vertex (a sparse volume's mesh only)

    def numpy(self) -> dict:
        out = dict(vertices=self.vertices.cpu().numpy(), normals=self.normals.cpu().numpy(), faces=self.faces.cpu().numpy())
        if self.colours is not None:
            out["colours"] = self.colours.cpu().numpy()
        if self.cells is not None:
            out["cells"] = self.cells.cpu().numpy()
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


BLOCK = 8                                               # samples per edge of a sparse volume's block
MAX_GRID_BLOCKS = 2 ** 31 - 1                           # of a sparse volume's block grid
MAX_EXTRACT_BLOCKS = (2 ** 32 - 1) // 3 // BLOCK ** 3   # allocated blocks a mesh is extracted from (32-bit quad offsets)
MAX_MARK_TAN = 1.5                                      # the widest half field of view ``allocate`` takes, as a tangent


class SparseTsdfVolume:
    """A sparse TSDF volume on the GPU (csrc/tsdf_sparse.hip): the lattice of ``TsdfVolume``
    is virtual -- any dimension up to 2^31 - 1 --, storage is 8 x 8 x 8 blocks near the observed surface::

        vol = SparseTsdfVolume(lo, hi, voxel=0.05, colour=True)
        vol.allocate(depths, cams)              # mark the blocks the depth maps' bands pass through; any number of calls
        vol.commit()                            # dilate, number the slots, create the arrays: the table is final
        vol.integrate(depths, cams, images=images)
        mesh = vol.extract()                    # Mesh with ``cells``

    After ``commit``: ``tsdf`` / ``weight`` [B,8,8,8] (k, j, i), ``colour`` [B,8,8,8,3] or None, ``block_of_slot`` [B],
    ``slots`` [gz,gy,gx] (-1: none).  Views allocated, committed and then integrated leave in every allocated sample the
    bits a ``TsdfVolume`` holds, and the mesh is the dense one in another order.  A view integrated without having been
    allocated is legal: it updates the allocated blocks only."""

    def __init__(self, lo, hi, voxel, trunc=None, colour=False, max_weight=math.inf, device=None):
        self.nx, self.ny, self.nz = volume_dims(lo, hi, voxel)
        if max(self.nx, self.ny, self.nz) > 2 ** 31 - 1:
            raise ValueError(f"{self.nx} x {self.ny} x {self.nz} samples; a dimension is at most 2^31 - 1")
        self.grid = tuple((n - 1) // BLOCK + 1 for n in (self.nx, self.ny, self.nz))
        if self.grid[0] * self.grid[1] * self.grid[2] > MAX_GRID_BLOCKS:
            raise ValueError(f"a block grid of {self.grid[0]} x {self.grid[1]} x {self.grid[2]}; at most 2^31 - 1 blocks "
                             "(hashed tables are not built)")
        self.lo = np.asarray(lo, np.float32).reshape(3)
        self.voxel = float(np.float32(voxel))
        self.trunc = float(np.float32(4.0) * np.float32(voxel)) if trunc is None else float(np.float32(trunc))
        self.max_weight = float(np.float32(max_weight))
        if not (self.trunc > 0.0 and math.isfinite(self.trunc)) or not self.max_weight > 0.0:
            raise ValueError("trunc must be positive and finite, max_weight positive")
        self.want_colour = bool(colour)
        from . import _lib
        self._lib = _lib
        if not torch.cuda.is_available():
            raise RuntimeError("SparseTsdfVolume lives on the GPU; no GPU is visible (there is no CPU path; "
                               "tests/tsdf_sparse_spec.py is the numpy spec)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        layout = (C.c_int64 * 4)()
        _lib.check(_lib.lib().hgs_tsdf_sparse_table_layout(self.nx, self.ny, self.nz, layout), "hgs_tsdf_sparse_table_layout")
        self._layout = tuple(int(v) for v in layout)
        self._table = torch.zeros(self._layout[3], dtype=torch.uint8, device=self.device)
        self.n_blocks = None
        self.tsdf = self.weight = self.colour = self.block_of_slot = None

    @property
    def dims(self):
        return self.nx, self.ny, self.nz

    @property
    def slots(self):
        G = self._layout[0]
        return self._table[:4 * G].view(torch.int32).view(self.grid[2], self.grid[1], self.grid[0])

    @property
    def marks(self):
        G, off = self._layout[0], self._layout[1]
        return self._table[off:off + G].view(self.grid[2], self.grid[1], self.grid[0])

    @property
    def nbytes(self):
        """Bytes held: the table and, after ``commit``, the blocks."""
        arrays = [a for a in (self.tsdf, self.weight, self.colour, self.block_of_slot) if a is not None]
        return self._table.numel() + sum(a.numel() * a.element_size() for a in arrays)

    def _struct(self):
        L = self._lib
        ptr = lambda t: None if t is None else t.data_ptr()
        return L.TsdfSparse(ptr(self.tsdf), ptr(self.weight), ptr(self.colour), ptr(self.block_of_slot),
                            self._table.data_ptr(), (C.c_float * 3)(*self.lo.tolist()), self.voxel, self.nx, self.ny, self.nz,
                            self.trunc, self.max_weight, -1 if self.n_blocks is None else self.n_blocks,
                            0 if self.tsdf is None else self.tsdf.shape[0])

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _plane(self, t, shape, what, k):
        if t is None:
            return None
        t = torch.as_tensor(t)
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError(f"{what} {k} must be float32 {list(shape)}, not {t.dtype} {list(t.shape)}")
        return t.to(self.device).contiguous()

    def _groups(self, depths, cams, weights, images, z_min):
        """The views 8 at a time: (hgs_tsdf_view array, count, the tensors it points into)."""
        L = self._lib
        depths, cams = list(depths), list(cams)
        weights = [None] * len(cams) if weights is None else list(weights)
        images = [None] * len(cams) if images is None else list(images)
        if not (len(depths) == len(cams) == len(weights) == len(images)):
            raise ValueError(f"{len(depths)} depths, {len(weights)} weights and {len(images)} images for {len(cams)} cameras")
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
            yield views, len(group), keep

    def allocate(self, depths, cams, weights=None, z_min=None):
        """Mark the blocks that the truncation bands of ``depths[k]`` under ``cams[k]`` pass through (``weights[k]``: a
        pixel of weight 0 marks nothing).  Any number of views and of calls, before ``commit``.  Asynchronous."""
        if self.n_blocks is not None:
            raise RuntimeError("allocate after commit: a committed volume's table is final (growing it is not built)")
        cams = list(cams)
        for k, cam in enumerate(cams):
            if not (0.0 < float(cam.tanfovx) <= MAX_MARK_TAN and 0.0 < float(cam.tanfovy) <= MAX_MARK_TAN):
                raise ValueError(f"field of view: camera {k} has tangents {float(cam.tanfovx):g}, {float(cam.tanfovy):g}; "
                                 f"at most {MAX_MARK_TAN} is allocated from")
        L = self._lib
        lib = L.lib()
        with torch.cuda.device(self.device):
            for views, n, keep in self._groups(depths, cams, weights, None, z_min):
                vol = self._struct()
                L.check(lib.hgs_tsdf_sparse_mark(C.byref(vol), views, n, self._stream(), self.device.index or 0),
                        "hgs_tsdf_sparse_mark")
        return self

    def commit(self):
        """Dilate the marks by one block, number the allocated blocks and create their arrays (1 / 0 / 0).  One host wait
        for the block count.  Afterwards the table is final.  Raises (a ``RuntimeError`` naming the "sub-pixel grid")
        when an allocated pixel was wider than 16 x 2 voxels at the far end of its band: that pixel was not marched, so
        the volume can never be committed -- make a new one with a larger voxel or without that view."""
        if self.n_blocks is not None:
            raise RuntimeError("commit after commit: a committed volume's table is final")
        L = self._lib
        lib = L.lib()
        dev = self.device
        with torch.cuda.device(dev):
            tmp = torch.empty(lib.hgs_tsdf_sparse_commit_tmp_bytes(self.nx, self.ny, self.nz), dtype=torch.uint8, device=dev)
            total = C.c_int64()
            vol = self._struct()
            L.check(lib.hgs_tsdf_sparse_commit_plan(C.byref(vol), tmp.data_ptr(), C.byref(total), self._stream(),
                                                    dev.index or 0), "hgs_tsdf_sparse_commit_plan")
            B = int(total.value)
            rows = max(B, 1)          # (an empty tensor has no address to hand to the calls)
            self.tsdf = torch.ones((rows, BLOCK, BLOCK, BLOCK), dtype=torch.float32, device=dev)
            self.weight = torch.zeros((rows, BLOCK, BLOCK, BLOCK), dtype=torch.float32, device=dev)
            self.colour = torch.zeros((rows, BLOCK, BLOCK, BLOCK, 3), dtype=torch.float32, device=dev) if self.want_colour else None
            self.block_of_slot = torch.full((rows,), -1, dtype=torch.int32, device=dev)
            self.n_blocks = B
            vol = self._struct()
            L.check(lib.hgs_tsdf_sparse_commit_apply(C.byref(vol), tmp.data_ptr(), self._stream(), dev.index or 0),
                    "hgs_tsdf_sparse_commit_apply")
        return self

    def _committed(self, what):
        if self.n_blocks is None:
            raise RuntimeError(f"{what} before commit: allocate the views and commit first")

    def integrate(self, depths, cams, weights=None, images=None, z_min=None):
        """``TsdfVolume.integrate`` on the allocated blocks.  Asynchronous on the current stream."""
        self._committed("integrate")
        if self.colour is None and images is not None and any(i is not None for i in images):
            raise ValueError("images given, but the volume was made without colour")
        L = self._lib
        lib = L.lib()
        with torch.cuda.device(self.device):
            for views, n, keep in self._groups(depths, cams, weights, images, z_min):
                vol = self._struct()
                L.check(lib.hgs_tsdf_sparse_integrate(C.byref(vol), views, n, self._stream(), self.device.index or 0),
                        "hgs_tsdf_sparse_integrate")
        return self

    def extract(self, min_weight=1.0) -> Mesh:
        """The surface-net mesh over the allocated blocks, with ``cells``; vertices by (slot, place of the cell in its
        block), faces by (slot, place of the edge's lower sample, axis).  One host wait for the two counts."""
        self._committed("extract")
        L = self._lib
        lib = L.lib()
        dev = self.device
        if self.n_blocks > MAX_EXTRACT_BLOCKS:
            raise ValueError(f"{self.n_blocks} blocks; a mesh is extracted from at most {MAX_EXTRACT_BLOCKS} "
                             "(the quad offsets are 32-bit)")
        with torch.cuda.device(dev):
            tmp = torch.empty(lib.hgs_tsdf_sparse_extract_tmp_bytes(self.n_blocks), dtype=torch.uint8, device=dev)
            totals = (C.c_int64 * 2)()
            vol = self._struct()
            L.check(lib.hgs_tsdf_sparse_extract_plan(C.byref(vol), float(min_weight), tmp.data_ptr(), totals, self._stream(),
                                                     dev.index or 0), "hgs_tsdf_sparse_extract_plan")
            V, Q = int(totals[0]), int(totals[1])
            vertices = torch.empty((V + 1, 3), dtype=torch.float32, device=dev)
            normals = torch.empty((V + 1, 3), dtype=torch.float32, device=dev)
            colours = torch.empty((V + 1, 3), dtype=torch.float32, device=dev) if self.colour is not None else None
            faces = torch.empty((2 * Q + 1, 3), dtype=torch.int32, device=dev)
            cells = torch.empty((V + 1, 3), dtype=torch.int32, device=dev)
            L.check(lib.hgs_tsdf_sparse_extract_apply(C.byref(vol), tmp.data_ptr(), vertices.data_ptr(), normals.data_ptr(),
                                                      None if colours is None else colours.data_ptr(), faces.data_ptr(),
                                                      cells.data_ptr(), self._stream(), dev.index or 0),
                    "hgs_tsdf_sparse_extract_apply")
        return Mesh(vertices[:V], normals[:V], None if colours is None else colours[:V], faces[:2 * Q], cells[:V])

    def numpy(self) -> dict:
        self._committed("numpy")
        B = self.n_blocks
        out = dict(tsdf=self.tsdf[:B].cpu().numpy(), weight=self.weight[:B].cpu().numpy(), slots=self.slots.cpu().numpy(),
                   marks=self.marks.cpu().numpy(), block_of_slot=self.block_of_slot[:B].cpu().numpy(), lo=self.lo.copy(),
                   voxel=np.float32(self.voxel), trunc=np.float32(self.trunc), max_weight=np.float32(self.max_weight),
                   dims=np.array(self.dims, np.int64))
        if self.colour is not None:
            out["colour"] = self.colour[:B].cpu().numpy()
        return out

    def to_dense(self, return_allocated=False):
        """A ``TsdfVolume`` over the same lattice holding the allocated samples (1 / 0 / 0 elsewhere); with
        ``return_allocated`` also the bool [nz,ny,nx] of the allocated samples.  Refused above the dense limits."""
        self._committed("to_dense")
        n = self.nx * self.ny * self.nz
        if n > MAX_SAMPLES:
            raise ValueError(f"{self.nx} x {self.ny} x {self.nz} = {n} samples; a dense volume holds at most 2^31 - 1")
        hi = self.lo.astype(np.float64) + self.voxel * (np.array(self.dims) - 1) + 0.25 * self.voxel
        dense = TsdfVolume(self.lo, hi, self.voxel, trunc=self.trunc, colour=self.colour is not None,
                           max_weight=self.max_weight, device=self.device)
        if dense.dims != self.dims:
            raise RuntimeError(f"the dense lattice came out as {dense.dims}, not {self.dims}")
        B, dev = self.n_blocks, self.device
        b = self.block_of_slot[:B].to(torch.int64)
        l = torch.arange(BLOCK, device=dev)
        i = (BLOCK * (b % self.grid[0]))[:, None, None, None] + l[None, None, None, :]
        j = (BLOCK * ((b // self.grid[0]) % self.grid[1]))[:, None, None, None] + l[None, None, :, None]
        k = (BLOCK * (b // (self.grid[0] * self.grid[1])))[:, None, None, None] + l[None, :, None, None]
        exists = ((i < self.nx) & (j < self.ny) & (k < self.nz)).expand(B, BLOCK, BLOCK, BLOCK)
        i, j, k = (a.expand(B, BLOCK, BLOCK, BLOCK)[exists] for a in (i, j, k))
        dense.tsdf[k, j, i] = self.tsdf[:B][exists]
        dense.weight[k, j, i] = self.weight[:B][exists]
        if self.colour is not None:
            dense.colour[k, j, i] = self.colour[:B][exists]
        if not return_allocated:
            return dense
        allocated = torch.zeros((self.nz, self.ny, self.nx), dtype=torch.bool, device=dev)
        allocated[k, j, i] = True
        return dense, allocated


def surface_depth(readout, min_alpha=0.5):
    """The depth map ``fuse_hierarchy`` integrates: ``median_depth`` where the pixel's ``alpha >= min_alpha``, else 0."""
    return torch.where(readout.alpha < min_alpha, torch.zeros_like(readout.median_depth), readout.median_depth)


KEEP_DEPTH_BYTES = 1 << 30      # depth maps a sparse fuse keeps between its two passes; beyond it they are rendered again


def fuse_hierarchy(h, cameras, volume, tau_px=0.0, frustum=True, min_alpha=0.5, colour=True, keep_depth_bytes=KEEP_DEPTH_BYTES):
    """Fuse what ``h`` shows under ``cameras`` into ``volume``; -> ``volume``.  Per camera one
    ``hgs.picking.read_hierarchy_view`` (alpha and median_depth) at the cut of ``tau_px`` pixels, the depth zeroed where
    ``alpha < min_alpha``; with ``colour`` (and a colour volume) also ``hgs.importance.render_hierarchy``'s image.  The
    cull bounds are computed once; the views are integrated 8 per pass over the volume, in order.

    A ``SparseTsdfVolume`` (not yet committed) takes two passes over the cameras: the first reads the depth alone and
    allocates, then the volume is committed; the second integrates as above.  The depth maps of the first pass are kept
    for the second while they fit ``keep_depth_bytes`` (default 1 GiB) in all, and rendered again otherwise."""
    from . import _lib
    from .importance import _nodes_only, activated, render_hierarchy
    from .picking import read_hierarchy_view
    if not h.nodes.is_cuda:
        raise RuntimeError("fuse_hierarchy works on the GPU: upload the hierarchy first (there is no CPU path)")
    colour = bool(colour) and (volume.want_colour if isinstance(volume, SparseTsdfVolume) else volume.colour is not None)
    bounds = None
    if frustum:
        from .frustum import cull_bounds
        rows = activated(_nodes_only(h))
        bounds = cull_bounds(h.nodes, rows["means3D"], rows["scales"])
    cameras = list(cameras)

    def depth_of(cam):
        r = read_hierarchy_view(h, cam, tau_px=tau_px, frustum=frustum, bounds=bounds, want=("alpha", "median_depth"))
        return surface_depth(r, min_alpha)

    kept = {}
    if isinstance(volume, SparseTsdfVolume):
        if volume.n_blocks is not None:
            raise RuntimeError("fuse_hierarchy allocates a sparse volume itself: hand it one that is not committed")
        held = 0
        for k, cam in enumerate(cameras):
            d = depth_of(cam)
            volume.allocate([d], [cam])
            nbytes = d.numel() * d.element_size()
            if held + nbytes <= keep_depth_bytes:
                kept[k] = d
                held += nbytes
        volume.commit()
    for g0 in range(0, len(cameras), _lib.TSDF_MAX_VIEWS):
        group = cameras[g0:g0 + _lib.TSDF_MAX_VIEWS]
        depths, images = [], []
        for k, cam in enumerate(group, g0):
            depths.append(kept.pop(k) if k in kept else depth_of(cam))
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
