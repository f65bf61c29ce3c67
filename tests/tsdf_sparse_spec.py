"""The spec of the SPARSE TSDF volume: a numpy float32 restatement of the allocation rule in
the order csrc/tsdf_block_rule.h writes it (marking, dilation, slot order), of the block-wise integration and of the
sparse extraction -- both through tests/tsdf_spec.py's own ``project`` / ``update`` / ``cell_vertex``, as the kernels of
csrc/tsdf_sparse.hip go through csrc/tsdf_rule.h -- so that the host build of the header and the kernels can be held
against it bit for bit.  Nothing here walks the virtual lattice: a volume of 4096 x 4096 x 512 samples costs its block
table.  Also the brute-force required set R and the mesh comparison the tests use.  A helper module, not a test."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import tsdf_spec as ts

F = np.float32
BLOCK = 8
MAX_SUB = 16
MAX_STEPS = 4096
MAX_TAN = 1.5


def block_grid(dims):
    return tuple((int(n) - 1) // BLOCK + 1 for n in dims)


def steps(trunc, voxel):
    c = np.ceil(F(trunc) / F(voxel))
    if not c <= MAX_STEPS:
        return MAX_STEPS + 1
    return int(c) if c >= 1 else 1


@dataclass
class SparseVolume:
    lo: np.ndarray                 # float32 [3]
    voxel: np.float32
    trunc: np.float32
    max_weight: np.float32
    dims: tuple                    # (nx, ny, nz) of the virtual lattice
    marks: np.ndarray              # bool [gbz,gby,gbx]
    refused: bool = False          # a pixel asked for more than MAX_SUB sub-positions
    slots: Optional[np.ndarray] = None           # int32 [gbz,gby,gbx] after commit
    block_of_slot: Optional[np.ndarray] = None   # int32 [B]
    tsdf: Optional[np.ndarray] = None            # float32 [B,8,8,8] (k, j, i)
    weight: Optional[np.ndarray] = None
    colour: Optional[np.ndarray] = None          # float32 [B,8,8,8,3]
    want_colour: bool = False

    @property
    def grid(self):
        return block_grid(self.dims)

    @property
    def n_blocks(self):
        return None if self.block_of_slot is None else int(self.block_of_slot.size)


def new_sparse(lo, voxel, dims, trunc=None, colour=False, max_weight=np.inf) -> SparseVolume:
    voxel = F(voxel)
    gx, gy, gz = block_grid(dims)
    return SparseVolume(np.asarray(lo, F), voxel, F(4) * voxel if trunc is None else F(trunc), F(max_weight),
                        tuple(int(n) for n in dims), np.zeros((gz, gy, gx), bool), want_colour=bool(colour))


# ---- the allocation rule -------------------------------------------------------------------------------------------------
def pixel_sub(v: ts.View, trunc, voxel):
    """-> (marched bool [H,W], M int [H,W], over bool [H,W]): the rule's pixel test, its M, and where M > MAX_SUB."""
    d = v.depth
    w = v.weight if v.weight is not None else np.ones_like(d)
    with np.errstate(all="ignore"):
        ok = (d > 0) & (w > 0)
        far = d + trunc
        ok &= (far - far) == 0
        fx = ((F(2) * v.tanfovx) * far) / F(v.W)
        fy = ((F(2) * v.tanfovy) * far) / F(v.H)
        m = np.ceil(np.where(fx > fy, fx, fy) / (F(2) * voxel))
        over = ok & ~(m <= MAX_SUB)
        M = np.where(m >= 1, m, 1)
    assert fx.dtype == F and m.dtype == F
    return ok & ~over, np.where(ok & ~over, M, 1).astype(np.int64), over


def block_point(px, py, a, b, M, z, v: ts.View, lo, voxel, grid):
    """tsdf_block_point on arrays: -> (marks bool, block int64 [..., 3]): the point's block clamped onto the grid, for a
    point up to one block outside it."""
    m = v.view
    with np.errstate(all="ignore"):
        fx = px.astype(F) + ((F(a) + F(0.5)) / F(M) - F(0.5))
        fy = py.astype(F) + ((F(b) + F(0.5)) / F(M) - F(0.5))
        p0 = ((F(2) * fx + F(1)) / F(v.W) - F(1)) * (z * v.tanfovx)
        p1 = ((F(2) * fy + F(1)) / F(v.H) - F(1)) * (z * v.tanfovy)
        q0, q1, q2 = p0 - m[9], p1 - m[10], z - m[11]
        inside, block = np.ones(z.shape, bool), []
        for c in range(3):
            x = (q0 * m[3 * c] + q1 * m[3 * c + 1]) + q2 * m[3 * c + 2]
            g = (x - lo[c]) / voxel
            bf = np.floor(g * F(0.125))
            assert x.dtype == F and bf.dtype == F
            fits = (bf >= -1) & (bf < F(2147483648.0))
            bi = np.where(fits, bf, -2).astype(np.int64)
            ok = (bi >= -1) & (bi <= grid[c])                  # up to one block outside the grid: the border block
            inside &= ok
            block.append(np.where(ok, np.clip(bi, 0, grid[c] - 1), 0))
    return inside, np.stack(block, -1)


def marched_points(sv: SparseVolume, v: ts.View):
    """Every (inside, block) batch of the marking of one view, with the pixels and depths it came from."""
    ok, M, over = pixel_sub(v, sv.trunc, sv.voxel)
    sv.refused = sv.refused or bool(over.any())
    S = steps(sv.trunc, sv.voxel)
    dz = (F(2) * sv.trunc) / F(S)
    for Mv in np.unique(M[ok]):
        py, px = np.nonzero(ok & (M == Mv))
        d = v.depth[py, px]
        for s in range(S + 1):
            z = (d - sv.trunc) + F(s) * dz
            assert z.dtype == F
            keep = z > v.z_min
            for b in range(int(Mv)):
                for a in range(int(Mv)):
                    inside, block = block_point(px[keep], py[keep], a, b, int(Mv), z[keep], v, sv.lo, sv.voxel, sv.grid)
                    yield inside, block, px[keep], py[keep], z[keep]


def mark(sv: SparseVolume, views):
    assert sv.slots is None, "mark after commit"
    for v in views:
        for inside, block, _, _, _ in marched_points(sv, v):
            b = block[inside]
            sv.marks[b[:, 2], b[:, 1], b[:, 0]] = True
    return sv


def dilate(marks):
    gz, gy, gx = marks.shape
    p = np.zeros((gz + 2, gy + 2, gx + 2), bool)
    p[1:-1, 1:-1, 1:-1] = marks
    out = np.zeros_like(marks)
    for dk in range(3):
        for dj in range(3):
            for di in range(3):
                out |= p[dk:dk + gz, dj:dj + gy, di:di + gx]
    return out


def dilate_sparse(marks):
    """``dilate`` for a table too large to shift 27 times: from the marked blocks alone."""
    gz, gy, gx = marks.shape
    out = np.zeros_like(marks)
    k, j, i = np.nonzero(marks)
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                kk, jj, ii = k + dk, j + dj, i + di
                ok = (kk >= 0) & (kk < gz) & (jj >= 0) & (jj < gy) & (ii >= 0) & (ii < gx)
                out[kk[ok], jj[ok], ii[ok]] = True
    return out


def commit(sv: SparseVolume):
    assert sv.slots is None and not sv.refused
    alloc = dilate_sparse(sv.marks)
    flat = alloc.reshape(-1)
    sv.block_of_slot = np.nonzero(flat)[0].astype(np.int32)          # ascending linear block index
    slots = np.full(flat.shape, -1, np.int32)
    slots[sv.block_of_slot] = np.arange(sv.block_of_slot.size, dtype=np.int32)
    sv.slots = slots.reshape(alloc.shape)
    B = sv.block_of_slot.size
    sv.tsdf = np.ones((B, 8, 8, 8), F)
    sv.weight = np.zeros((B, 8, 8, 8), F)
    sv.colour = np.zeros((B, 8, 8, 8, 3), F) if sv.want_colour else None
    return sv


def block_coords(sv: SparseVolume):
    """int64 [B,3]: (bi, bj, bk) of every slot."""
    gx, gy, gz = sv.grid
    b = sv.block_of_slot.astype(np.int64)
    return np.stack([b % gx, (b // gx) % gy, b // (gx * gy)], -1)


def sample_coords(sv: SparseVolume):
    """Lattice indices of every stored sample, broadcastable to [B,8,8,8]: (i, j, k), and whether it lies in the lattice."""
    bc = block_coords(sv)
    l = np.arange(8)
    i = (8 * bc[:, 0])[:, None, None, None] + l[None, None, None, :]
    j = (8 * bc[:, 1])[:, None, None, None] + l[None, None, :, None]
    k = (8 * bc[:, 2])[:, None, None, None] + l[None, :, None, None]
    nx, ny, nz = sv.dims
    return i, j, k, np.broadcast_to((i < nx) & (j < ny) & (k < nz), (bc.shape[0], 8, 8, 8))


# ---- integration: tsdf_spec's rule, block by block ---------------------------------------------------------------------------
def integrate(sv: SparseVolume, views):
    i, j, k, exists = sample_coords(sv)
    x0 = sv.lo[0] + sv.voxel * i.astype(F)
    x1 = sv.lo[1] + sv.voxel * j.astype(F)
    x2 = sv.lo[2] + sv.voxel * k.astype(F)
    assert x0.dtype == F
    shape = exists.shape
    for v in views:
        ok, z, px, py = ts.project(x0, x1, x2, v)
        ok, z = np.broadcast_to(ok, shape) & exists, np.broadcast_to(z, shape)
        px, py = np.broadcast_to(px, shape), np.broadcast_to(py, shape)
        d = v.depth[py, px]
        w = v.weight[py, px] if v.weight is not None else np.ones(shape, F)
        rgb = np.moveaxis(v.rgb[:, py, px], 0, -1) if v.rgb is not None else None
        sv.tsdf, sv.weight, sv.colour, _ = ts.update(sv.tsdf, sv.weight, sv.colour, ok, z, d, w, rgb, sv.trunc,
                                                     sv.max_weight)
    return sv


def to_dense(sv: SparseVolume):
    """-> (ts.Volume created as 1 / 0 / 0 and filled where allocated, allocated bool [nz,ny,nx]); small lattices only."""
    nx, ny, nz = sv.dims
    vol = ts.new_volume(sv.lo, sv.voxel, sv.dims, trunc=sv.trunc, colour=sv.colour is not None, max_weight=sv.max_weight)
    i, j, k, exists = sample_coords(sv)
    i, j, k = (np.broadcast_to(a, exists.shape)[exists] for a in (i, j, k))
    allocated = np.zeros((nz, ny, nx), bool)
    allocated[k, j, i] = True
    vol.tsdf[k, j, i] = sv.tsdf[exists]
    vol.weight[k, j, i] = sv.weight[exists]
    if sv.colour is not None:
        vol.colour[k, j, i] = sv.colour[exists]
    return vol, allocated


# ---- extraction ----------------------------------------------------------------------------------------------------------------
def halo(sv: SparseVolume, a, fill):
    """a [B,8,8,8,...] -> [B,9,9,9,...]: every block with the +1 faces of its neighbours; ``fill`` where the sample lies
    beyond the lattice or in no allocated block."""
    B = a.shape[0]
    out = np.full((B, 9, 9, 9) + a.shape[4:], fill, a.dtype)
    bc = block_coords(sv)
    gx, gy, gz = sv.grid
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                n = bc + np.array([di, dj, dk])
                ok = (n[:, 0] < gx) & (n[:, 1] < gy) & (n[:, 2] < gz)
                slot = np.full(B, -1, np.int64)
                slot[ok] = sv.slots[n[ok, 2], n[ok, 1], n[ok, 0]]
                have = slot >= 0
                dst = tuple(slice(8, 9) if o else slice(0, 8) for o in (dk, dj, di))
                src = tuple(slice(0, 1) if o else slice(0, 8) for o in (dk, dj, di))
                out[(have,) + dst] = a[(slot[have],) + src]
    return out


@dataclass
class SparseMesh:
    vertices: np.ndarray   # float32 [V,3]
    normals: np.ndarray
    colours: Optional[np.ndarray]
    faces: np.ndarray      # int32 [2Q,3]
    cells: np.ndarray      # int32 [V,3]


def extract(sv: SparseVolume, min_weight=1.0) -> SparseMesh:
    min_weight = F(min_weight)
    B = sv.n_blocks
    _, _, _, exists = sample_coords(sv)
    w = np.where(exists, sv.weight, F(-1))                 # a stored sample beyond the lattice does not exist
    hw, ht = halo(sv, w, F(-1)), halo(sv, sv.tsdf, F(1))
    obs, ins = hw >= min_weight, ht < 0
    c8 = lambda a: np.stack([a[:, (s >> 2):8 + (s >> 2), ((s >> 1) & 1):8 + ((s >> 1) & 1), (s & 1):8 + (s & 1)]
                             for s in range(8)], -1)
    ins8 = c8(ins)
    active = c8(obs).all(-1) & ins8.any(-1) & ~ins8.all(-1)           # [B,8,8,8]
    vs, vk, vj, vi = np.nonzero(active)                                # (slot, place) ascending
    V = vs.size
    local, normal = ts.cell_vertex(c8(ht)[vs, vk, vj, vi])
    bc = block_coords(sv)
    cells = 8 * bc[vs] + np.stack([vi, vj, vk], -1)
    vertices = sv.lo[None, :] + sv.voxel * (cells.astype(F) + local)
    assert vertices.dtype == F
    colours = None
    if sv.colour is not None:
        hc = halo(sv, sv.colour, F(0))
        colours = ts.cell_colour(c8(hc)[vs, vk, vj, vi])      # [V,3,8]
    vidx = np.full((B, 8, 8, 8), -1, np.int64)
    vidx[vs, vk, vj, vi] = np.arange(V)
    gx, gy, gz = sv.grid

    def vertex_of(cell):
        ok = (cell >= 0).all(-1)
        b, l = cell >> 3, cell & 7
        ok &= (b[:, 0] < gx) & (b[:, 1] < gy) & (b[:, 2] < gz)
        slot = np.full(cell.shape[0], -1, np.int64)
        slot[ok] = sv.slots[b[ok, 2], b[ok, 1], b[ok, 0]]
        out = np.full(cell.shape[0], -1, np.int64)
        have = slot >= 0
        out[have] = vidx[slot[have], l[have, 2], l[have, 1], l[have, 0]]
        return out

    keys, faces = [], []
    for axis in range(3):
        up = tuple(slice(1, 9) if a == axis else slice(0, 8) for a in (2, 1, 0))       # (k, j, i) slices
        lo_s = (slice(0, 8),) * 3
        edge = obs[(slice(None),) + lo_s] & obs[(slice(None),) + up] & (ins[(slice(None),) + lo_s] != ins[(slice(None),) + up])
        s, k, j, i = np.nonzero(edge)
        at = 8 * bc[s] + np.stack([i, j, k], -1)
        v = np.stack([vertex_of(at + np.array(o)) for o in ts.quad_cells(axis)], -1)
        keep = (v >= 0).all(-1)
        s, k, j, i, v = s[keep], k[keep], j[keep], i[keep], v[keep]
        keys.append((s * 512 + (k * 64 + j * 8 + i)) * 3 + axis)
        faces.append(ts.quad_faces(v, ins[s, k, j, i]))
    keys, faces = np.concatenate(keys), np.concatenate(faces)
    order = np.argsort(keys, kind="stable")
    return SparseMesh(vertices, normal, colours, faces[order].reshape(-1, 3).astype(np.int32), cells.astype(np.int32))


# ---- what the tests compare with -----------------------------------------------------------------------------------------
def near_samples(lo, voxel, trunc, dims, views):
    """bool [nz,ny,nx]: the near samples of ``views`` by brute force over a (small) dense lattice."""
    nx, ny, nz = dims
    x0 = ts.lattice(lo[0], voxel, nx)[None, None, :]
    x1 = ts.lattice(lo[1], voxel, ny)[None, :, None]
    x2 = ts.lattice(lo[2], voxel, nz)[:, None, None]
    near = np.zeros((nz, ny, nx), bool)
    for v in views:
        ok, z, px, py = ts.project(x0, x1, x2, v)
        d = v.depth[py, px]
        w = v.weight[py, px] if v.weight is not None else np.ones_like(d)
        with np.errstate(invalid="ignore"):
            sdf = d - z
            near |= ok & (d > 0) & (w > 0) & (sdf >= -trunc) & (sdf < trunc)
    return near


def required_blocks(near):
    """bool [gbz,gby,gbx]: R, every block holding a sample within one lattice step per axis of a near sample."""
    wide = dilate(near)
    nz, ny, nx = near.shape
    gx, gy, gz = block_grid((nx, ny, nz))
    p = np.zeros((8 * gz, 8 * gy, 8 * gx), bool)
    p[:nz, :ny, :nx] = wide
    return p.reshape(gz, 8, gy, 8, gx, 8).any((1, 3, 5))


def canonical_mesh(vertices, faces, cells, dims, *more):
    """A mesh in the order that does not depend on the path: vertices (and ``more`` per-vertex arrays) by ascending
    linear cell index, the triangles' rows remapped and sorted as a multiset (winding untouched)."""
    nx, ny, nz = dims
    c = np.asarray(cells, np.int64)
    lin = (c[:, 2] * (ny - 1) + c[:, 1]) * (nx - 1) + c[:, 0] if c.size else np.zeros(0, np.int64)
    order = np.argsort(lin, kind="stable")
    inv = np.empty(order.size, np.int64)
    inv[order] = np.arange(order.size)
    f = inv[np.asarray(faces, np.int64)] if np.asarray(faces).size else np.zeros((0, 3), np.int64)
    f = f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]
    return (np.asarray(vertices)[order], f, lin[order]) + tuple(np.asarray(m)[order] for m in more)
