"""The spec of TSDF fusion and of the surface-net extraction: a numpy float32 restatement of
both rules in the order csrc/tsdf_rule.h writes them -- every operation a float32 numpy operation, left to right, no
contraction -- so that the host build of the header and the kernels of csrc/tsdf.hip can be held against it bit for bit.
Also the analytic float64 depth maps (a plane, a sphere) the property tests fuse.  A helper module, not a test."""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

F = np.float32


# ---- volume and views ------------------------------------------------------------------------------------------------
@dataclass
class Volume:
    lo: np.ndarray                 # float32 [3]
    voxel: np.float32
    trunc: np.float32
    max_weight: np.float32
    tsdf: np.ndarray               # float32 [nz,ny,nx]
    weight: np.ndarray             # float32 [nz,ny,nx]
    colour: Optional[np.ndarray]   # float32 [nz,ny,nx,3]

    @property
    def dims(self):
        nz, ny, nx = self.tsdf.shape
        return nx, ny, nz

    def copy(self):
        return Volume(self.lo.copy(), self.voxel, self.trunc, self.max_weight, self.tsdf.copy(), self.weight.copy(),
                      None if self.colour is None else self.colour.copy())


def new_volume(lo, voxel, dims, trunc=None, colour=False, max_weight=np.inf) -> Volume:
    nx, ny, nz = dims
    voxel = F(voxel)
    return Volume(np.asarray(lo, F), voxel, F(4) * voxel if trunc is None else F(trunc), F(max_weight),
                  np.ones((nz, ny, nx), F), np.zeros((nz, ny, nx), F), np.zeros((nz, ny, nx, 3), F) if colour else None)


@dataclass
class View:
    depth: np.ndarray              # float32 [H,W]
    view: np.ndarray               # float32 [12]: world_view_transform[r][c] at 3 r + c
    tanfovx: np.float32
    tanfovy: np.float32
    z_min: np.float32
    weight: Optional[np.ndarray] = None    # float32 [H,W]
    rgb: Optional[np.ndarray] = None       # float32 [3,H,W]

    @property
    def W(self):
        return self.depth.shape[1]

    @property
    def H(self):
        return self.depth.shape[0]


def view_words(cam) -> np.ndarray:
    """The 12 matrix words of a ``hgs.synth.Camera`` (or anything with a [4,4] ``world_view_transform``)."""
    return np.ascontiguousarray(np.asarray(cam.world_view_transform, dtype=F)[:, :3]).reshape(12)


def view_of(cam, depth, weight=None, rgb=None, z_min=None) -> View:
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=F)
    return View(f(depth), view_words(cam), F(cam.tanfovx), F(cam.tanfovy), F(cam.znear if z_min is None else z_min),
                f(weight), f(rgb))


def lattice(lo, voxel, n):
    return F(lo) + F(voxel) * np.arange(n).astype(F)


# ---- the integrate rule ------------------------------------------------------------------------------------------------
def project(x0, x1, x2, v: View):
    """Steps 1 and 2 on float32 arrays (broadcast): -> (ok, z, px, py); px / py are int64, 0 where not ok."""
    m, W, H = v.view, F(v.W), F(v.H)
    with np.errstate(all="ignore"):
        p0 = ((x0 * m[0] + x1 * m[3]) + x2 * m[6]) + m[9]
        p1 = ((x0 * m[1] + x1 * m[4]) + x2 * m[7]) + m[10]
        z = ((x0 * m[2] + x1 * m[5]) + x2 * m[8]) + m[11]
        ok = z > v.z_min
        fx = ((p0 / (z * v.tanfovx) + F(1)) * W - F(1)) * F(0.5)
        fy = ((p1 / (z * v.tanfovy) + F(1)) * H - F(1)) * F(0.5)
        px, py = np.floor(fx + F(0.5)), np.floor(fy + F(0.5))
        ok = ok & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    assert p0.dtype == F and fx.dtype == F
    return ok, z, np.where(ok, px, 0).astype(np.int64), np.where(ok, py, 0).astype(np.int64)


def update(tsdf, weight, colour, ok, z, d, w, rgb, trunc, max_weight):
    """Steps 3 to 6 on arrays: -> (tsdf, weight, colour, applied)."""
    with np.errstate(all="ignore"):
        ok = ok & (d > 0) & (w > 0)
        sdf = d - z
        ok = ok & (sdf >= -trunc)
        q = sdf / trunc
        t = np.where(q < 1, q, F(1))
        Wn = weight + w
        new_t = (weight * tsdf + w * t) / Wn
        if colour is not None and rgb is not None:
            new_c = (weight[..., None] * colour + w[..., None] * rgb) / Wn[..., None]
            colour = np.where(ok[..., None], new_c, colour)
        new_w = np.where(Wn < max_weight, Wn, max_weight)
    assert new_t.dtype == F and new_w.dtype == F
    return np.where(ok, new_t, tsdf), np.where(ok, new_w, weight), colour, ok


def integrate(vol: Volume, views) -> np.ndarray:
    """Applies ``views`` in order, in place; -> bool [nz,ny,nx]: the samples some view's image holds (steps 1 and 2)."""
    nx, ny, nz = vol.dims
    x0 = lattice(vol.lo[0], vol.voxel, nx)[None, None, :]
    x1 = lattice(vol.lo[1], vol.voxel, ny)[None, :, None]
    x2 = lattice(vol.lo[2], vol.voxel, nz)[:, None, None]
    seen = np.zeros((nz, ny, nx), bool)
    for v in views:
        ok, z, px, py = project(x0, x1, x2, v)
        ok, z = np.broadcast_to(ok, seen.shape), np.broadcast_to(z, seen.shape)
        seen |= ok
        d = v.depth[py, px]
        w = v.weight[py, px] if v.weight is not None else np.ones(seen.shape, F)
        rgb = np.moveaxis(v.rgb[:, py, px], 0, -1) if v.rgb is not None else None
        vol.tsdf, vol.weight, vol.colour, _ = update(vol.tsdf, vol.weight, vol.colour, ok, z, d, w, rgb, vol.trunc,
                                                     vol.max_weight)
    return seen


# ---- the extraction rule -----------------------------------------------------------------------------------------------
def edge_lo(e):
    axis, q = e >> 2, e & 3
    return 2 * q if axis == 0 else (q >> 1) * 4 + (q & 1) if axis == 1 else q


def cell_vertex(t):
    """t: float32 [..., 8], a cell's samples in the order 4 dk + 2 dj + di -> (local [..., 3], normal [..., 3])."""
    ins = t < 0
    zero = np.zeros(t.shape[:-1], F)
    s, g, count = [zero, zero, zero], [None, None, None], np.zeros(t.shape[:-1], np.int32)
    with np.errstate(all="ignore"):
        for e in range(12):
            axis, a = e >> 2, edge_lo(e)
            b = a + (1 << axis)
            ta, tb = t[..., a], t[..., b]
            g[axis] = (tb - ta) if (e & 3) == 0 else g[axis] + (tb - ta)
            cross = ins[..., a] != ins[..., b]
            tau = ta / (ta - tb)
            for c in range(3):
                base = F((a >> c) & 1)
                s[c] = np.where(cross, s[c] + ((base + tau) if c == axis else base), s[c])
            count = count + cross
        local = np.stack([s[c] / count.astype(F) for c in range(3)], -1)
        n = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        normal = np.stack([np.where(n > 0, g[c] / n, F(0)) for c in range(3)], -1)
    assert local.dtype == F and normal.dtype == F
    return local, normal


def cell_colour(c):
    """c: float32 [..., 8] -> the mean in sample order."""
    s = c[..., 0]
    for k in range(1, 8):
        s = s + c[..., k]
    return s / F(8)


def quad_cells(axis):
    """[4][3]: the (di, dj, dk) of the four cells around an edge along ``axis``, normal along +axis."""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    out = []
    for du, dv in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
        o = [0, 0, 0]
        o[u], o[v] = du, dv
        out.append(o)
    return out


def quad_faces(v, lower_inside):
    """v: int [..., 4] -> int [..., 2, 3]."""
    v1 = np.where(lower_inside, v[..., 1], v[..., 3])
    v3 = np.where(lower_inside, v[..., 3], v[..., 1])
    return np.stack([np.stack([v[..., 0], v1, v[..., 2]], -1), np.stack([v[..., 0], v[..., 2], v3], -1)], -2)


@dataclass
class SpecMesh:
    vertices: np.ndarray   # float32 [V,3]
    normals: np.ndarray    # float32 [V,3]
    colours: Optional[np.ndarray]
    faces: np.ndarray      # int32 [2Q,3]
    active: np.ndarray     # bool [nz-1,ny-1,nx-1] (empty where a dimension is 1)
    cells: np.ndarray      # int64 [V,3]: (i, j, k) of every vertex' cell
    quad_edges: np.ndarray  # int64 [Q,4]: (i, j, k, axis) of every quad's edge


def corners(a):
    """a [nz,ny,nx,...] -> [nz-1,ny-1,nx-1,...,8]: every cell's samples in sample order."""
    nz, ny, nx = a.shape[:3]
    return np.stack([a[(s >> 2):nz - 1 + (s >> 2), ((s >> 1) & 1):ny - 1 + ((s >> 1) & 1), (s & 1):nx - 1 + (s & 1)]
                     for s in range(8)], -1)


def extract(vol: Volume, min_weight=1.0) -> SpecMesh:
    nx, ny, nz = vol.dims
    min_weight = F(min_weight)
    obs, ins = vol.weight >= min_weight, vol.tsdf < 0
    t8 = corners(vol.tsdf)
    ins8 = corners(ins)
    active = corners(obs).all(-1) & ins8.any(-1) & ~ins8.all(-1)
    ck, cj, ci = np.nonzero(active)                      # ascending linear cell index
    V = ck.size
    local, normal = cell_vertex(t8[ck, cj, ci])
    at = np.stack([ci, cj, ck], -1).astype(F)
    vertices = vol.lo[None, :] + vol.voxel * (at + local)
    assert vertices.dtype == F
    colours = None
    if vol.colour is not None:
        c8 = corners(vol.colour)[ck, cj, ci]             # [V,3,8]
        colours = cell_colour(c8)
    vidx = np.full((nz + 1, ny + 1, nx + 1), -1, np.int64)      # cell (i, j, k) at [k + 1, j + 1, i + 1]
    vidx[ck + 1, cj + 1, ci + 1] = np.arange(V)
    keys, faces, edges = [], [], []
    step = ((0, 0, 1), (0, 1, 0), (1, 0, 0))            # (dk, dj, di) of the axes x, y, z
    for axis in range(3):
        dk, dj, di = step[axis]
        lo_s = (slice(0, nz - dk), slice(0, ny - dj), slice(0, nx - di))
        hi_s = (slice(dk, nz), slice(dj, ny), slice(di, nx))
        edge = obs[lo_s] & obs[hi_s] & (ins[lo_s] != ins[hi_s])
        k, j, i = np.nonzero(edge)
        v = np.stack([vidx[k + o[2] + 1, j + o[1] + 1, i + o[0] + 1] for o in quad_cells(axis)], -1)
        keep = (v >= 0).all(-1)
        k, j, i, v = k[keep], j[keep], i[keep], v[keep]
        keys.append(((k * ny + j) * nx + i) * 3 + axis)
        faces.append(quad_faces(v, ins[k, j, i]))
        edges.append(np.stack([i, j, k, np.full_like(i, axis)], -1))
    keys, faces, edges = np.concatenate(keys), np.concatenate(faces), np.concatenate(edges)
    order = np.argsort(keys, kind="stable")
    return SpecMesh(vertices, normal, colours, faces[order].reshape(-1, 3).astype(np.int32), active,
                    np.stack([ci, cj, ck], -1), edges[order])


# ---- analytic depth maps (float64) -------------------------------------------------------------------------------------
def pixel_rays(cam):
    """float64 [H,W,3]: every pixel centre's camera-space direction with z = 1 (the renderer's pixel-centre convention)."""
    W, H = int(cam.image_width), int(cam.image_height)
    x = ((2.0 * np.arange(W) + 1.0) / W - 1.0) * math.tan(cam.FoVx * 0.5)
    y = ((2.0 * np.arange(H) + 1.0) / H - 1.0) * math.tan(cam.FoVy * 0.5)
    return np.stack([np.broadcast_to(x[None, :], (H, W)), np.broadcast_to(y[:, None], (H, W)), np.ones((H, W))], -1)


def _camera(cam):
    m = np.asarray(cam.world_view_transform, dtype=np.float64)
    return m[:3, :3], m[3, :3]          # p_cam = x_world @ A + t


def plane_depth(cam, normal, offset):
    """The view-space depth at every pixel of the plane normal . x = offset; 0 where the ray misses it."""
    A, t = _camera(cam)
    Ainv = np.linalg.inv(A)
    n = np.asarray(normal, np.float64)
    with np.errstate(all="ignore"):
        z = (offset + n @ (t @ Ainv)) / (pixel_rays(cam) @ Ainv @ n)
    return np.where(np.isfinite(z) & (z > 0), z, 0.0)


def sphere_depth(cam, centre, radius):
    """The view-space depth of the near side of a sphere; 0 where the ray misses it."""
    A, t = _camera(cam)
    c = np.asarray(centre, np.float64) @ A + t
    d = pixel_rays(cam)
    a, b, cc = (d * d).sum(-1), d @ c, c @ c - radius * radius
    disc = b * b - a * cc
    with np.errstate(all="ignore"):
        z = (b - np.sqrt(disc)) / a
    return np.where((disc > 0) & (z > 0), z, 0.0)


def e_pix(depths):
    """The largest depth difference between 4-neighbouring valid pixels of the maps."""
    worst = 0.0
    for d in depths:
        d = np.asarray(d, np.float64)
        for a, b in ((d[:, 1:], d[:, :-1]), (d[1:, :], d[:-1, :])):
            both = (a > 0) & (b > 0)
            if both.any():
                worst = max(worst, float(np.abs(a - b)[both].max()))
    return worst
