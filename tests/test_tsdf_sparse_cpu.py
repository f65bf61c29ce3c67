"""The sparse TSDF volume without a GPU: the numpy spec tests/tsdf_sparse_spec.py held against
the dense spec tests/tsdf_spec.py -- the allocated set holds the required set, the allocated samples carry the dense
bits, no active cell reaches outside the allocation, the meshes are equal --, the derived over-allocation bound, and the
C ABI's and the Python class's argument checks and size queries.  tests/test_tsdf_sparse_gpu.py runs the same scenes on
the device."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import tsdf_sparse_spec as sp
import tsdf_spec as ts
from hgs import _lib, synth

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def noisy_views(rng, n, W, H, centre_z, trunc, weight, colour, z_min=0.05):
    views = []
    for k in range(n):
        cam = synth.orbit_camera(W, H, k, max(n, 3), radius=0.35, tilt=0.1) if k else synth.make_camera(W, H)
        depth = (centre_z + 3.0 * trunc * (2 * rng.random((H, W)) - 1)).astype(F)
        if W * H > 1:
            depth[rng.random((H, W)) < 0.1] = 0.0                  # holes
            depth[rng.random((H, W)) < 0.05] = np.nan
        w = None
        if weight:
            w = (2 * rng.random((H, W))).astype(F)
            w[rng.random((H, W)) < 0.15] = 0.0
        rgb = rng.random((3, H, W)).astype(F) if colour and k % 3 != 2 else None      # (a view without colours among them)
        views.append(ts.view_of(cam, depth, w, rgb, z_min=z_min))
    return views


def centred_lo(dims, voxel, z0):
    voxel = F(voxel)
    return np.array([F(-0.5) * voxel * F(dims[0] - 1) + F(0.003), F(-0.5) * voxel * F(dims[1] - 1) - F(0.002), F(z0)], F)


def scene(name):
    """-> dict(dims, lo, voxel, trunc, colour, max_weight, views, cams, surface): the cases of DESIGN.md f-28's tests."""
    rng = np.random.default_rng(sum(map(ord, name)))
    s = dict(colour=False, max_weight=np.inf, surface=None, cams=None)
    if name in ("1x1x1", "8x8x8", "9x9x9", "65x7x9", "17x9x23"):
        dims = tuple(int(v) for v in name.split("x"))
        image, n, weight, colour, mw = {"1x1x1": ((1, 1), 1, False, False, np.inf), "8x8x8": ((7, 5), 2, True, True, np.inf),
                                        "9x9x9": ((33, 17), 3, False, True, np.inf), "65x7x9": ((80, 60), 2, True, False, 1.5),
                                        "17x9x23": ((33, 17), 8, True, True, 4.0)}[name]
        voxel = F(1.3 / max(dims)) if max(dims) > 1 else F(0.1)
        lo = centred_lo(dims, voxel, 1.0)
        trunc = F(2.5) * voxel
        centre = 1.0 + 0.5 * float(voxel) * dims[2]
        s.update(dims=dims, lo=lo, voxel=voxel, trunc=trunc, colour=colour, max_weight=mw,
                 views=noisy_views(rng, n, *image, centre, float(trunc), weight, colour))
        return s
    if name in ("seam", "border", "nan", "zero", "behind"):
        dims, voxel = (24, 24, 24) if name != "border" else (20, 20, 20), F(0.05)
        lo = np.array([-0.6, -0.6, 0.8], F)
        k_plane = {"seam": 7.5, "border": 18.5}.get(name, 11.3)           # in lattice steps along z
        off = float(lo[2]) + float(voxel) * k_plane
        cam = synth.make_camera(80, 60)
        depth = ts.plane_depth(cam, (0.0, 0.0, 1.0), off)
        view = ts.view_of(cam, depth, z_min=0.05)
        if name == "nan":
            view.depth[rng.random(depth.shape) < 0.2] = np.nan
            view.weight = np.where(rng.random(depth.shape) < 0.3, 0.0, 1.5).astype(F)
        if name == "zero":
            view.depth[:] = 0.0
        views = [view]
        if name == "behind":              # one view whose z_min lies behind the lattice, one that looks past it
            far = synth.make_camera(80, 60, T=(50.0, 0.0, 0.0))
            views = [ts.view_of(cam, depth, z_min=5.0), ts.view_of(far, depth, z_min=0.05)]
        s.update(dims=dims, lo=lo, voxel=voxel, trunc=F(4) * voxel, views=views,
                 surface=("plane", (0.0, 0.0, 1.0), off) if name in ("seam", "border") else None)
        return s
    if name in ("sphere", "nine"):
        n = 4 if name == "sphere" else 9
        dims, voxel = (40, 40, 40), F(0.03)
        centre = np.array([0.0, 0.0, 1.5])
        lo = (centre - 16 * float(voxel)).astype(F)                     # sample 16: a block corner
        centre = lo.astype(np.float64) + 16 * float(voxel)
        radius = 10 * float(voxel)
        cams = [synth.orbit_camera(80, 60, k, n, radius=0.5) for k in range(n)]
        depths = [ts.sphere_depth(cam, centre, radius) for cam in cams]
        rgb = [np.stack([(d > 0) * 0.1 * (k + 1), d * 0.3, 1.0 - d * 0.3]) for k, d in enumerate(depths)]
        s.update(dims=dims, lo=lo, voxel=voxel, trunc=F(4) * voxel, colour=True, max_weight=3.0 if name == "nine" else np.inf,
                 views=[ts.view_of(c, d, rgb=i) for c, d, i in zip(cams, depths, rgb)], cams=cams,
                 surface=("sphere", centre, radius))
        return s
    if name == "fine":                    # a 4 x 3 image over fine voxels: M > 1
        dims, voxel = (60, 46, 24), F(0.012)
        lo = centred_lo(dims, voxel, 0.4)
        cam = synth.make_camera(4, 3)
        depth = ts.plane_depth(cam, (0.0, 0.0, 1.0), 0.55)
        s.update(dims=dims, lo=lo, voxel=voxel, trunc=F(4) * voxel, views=[ts.view_of(cam, depth, z_min=0.05)])
        return s
    if name == "edge_ray":                # one pixel whose ray runs half a voxel OUTSIDE the lattice, along its x = lo face:
        voxel = F(0.05)                   # the near samples just inside have their marched points outside the grid
        cam = synth.make_camera(1, 1, fovy_deg=math.degrees(2 * math.atan(0.04)))
        s.update(dims=(16, 16, 16), lo=np.array([0.5 * float(voxel), -0.39, 0.7], F), voxel=voxel, trunc=F(4) * voxel,
                 views=[ts.view_of(cam, np.ones((1, 1), F), z_min=0.05)])
        return s
    if name == "corner":                  # the lattice's corner inside the frustum under a map that is mostly holes: the
        voxel = F(0.05)                   # only surface pixels' rays pass the lattice a few voxels outside it.  Marched
        cam = synth.make_camera(8, 8)     # points outside the grid used to be dropped: B = 0 against 4 dense vertices
        rng = np.random.default_rng(168)
        depth = (1.0 + 0.15 * (2 * rng.random((8, 8)) - 1)).astype(F)
        depth[rng.random((8, 8)) < 0.9] = 0.0
        depth[rng.random((8, 8)) < 0.2] = 3.0
        lo = np.array([rng.uniform(0.0, 0.5), rng.uniform(0.0, 0.5), 0.7], F)
        s.update(dims=(12, 12, 12), lo=lo, voxel=voxel, trunc=F(4) * voxel, views=[ts.view_of(cam, depth, z_min=0.05)])
        return s
    raise KeyError(name)


SCENES = ("1x1x1", "8x8x8", "9x9x9", "65x7x9", "17x9x23", "seam", "sphere", "border", "zero", "behind", "nan", "nine", "fine",
          "edge_ray", "corner")
_FUSED = {}


def fused(name):
    """The scene fused by both specs, once: (scene, dense volume, sparse volume).  Shared; leave it unchanged."""
    if name not in _FUSED:
        s = scene(name)
        dense = ts.new_volume(s["lo"], s["voxel"], s["dims"], trunc=s["trunc"], colour=s["colour"], max_weight=s["max_weight"])
        ts.integrate(dense, s["views"])
        sv = sp.new_sparse(s["lo"], s["voxel"], s["dims"], trunc=s["trunc"], colour=s["colour"], max_weight=s["max_weight"])
        sp.mark(sv, s["views"])
        sp.commit(sv)
        sp.integrate(sv, s["views"])
        _FUSED[name] = (s, dense, sv)
    return _FUSED[name]


def assert_same_mesh(dense, sparse, dims):
    """dense / sparse: dicts of vertices, normals, faces, cells (and colours).  Equal after ordering the vertices by linear
    cell index and comparing the remapped triangle rows as sorted multisets; the winding is untouched."""
    more = ("normals",) + (("colours",) if dense.get("colours") is not None else ())
    a = sp.canonical_mesh(dense["vertices"], dense["faces"], dense["cells"], dims, *[dense[k] for k in more])
    b = sp.canonical_mesh(sparse["vertices"], sparse["faces"], sparse["cells"], dims, *[sparse[k] for k in more])
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, (a[0].shape, b[0].shape, a[1].shape, b[1].shape)
    assert np.array_equal(a[2], b[2])                                   # the same cells
    assert np.array_equal(bits(a[0]), bits(b[0]))
    assert np.array_equal(a[1], b[1])
    for x, y in zip(a[3:], b[3:]):
        assert np.array_equal(bits(x), bits(y))


def mesh_dict(m):
    return dict(vertices=m.vertices, normals=m.normals, colours=m.colours, faces=m.faces, cells=m.cells)


# ---- spec against spec -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_the_allocation_holds_the_required_set_and_the_sparse_spec_equals_the_dense_one(name):
    s, dense, sv = fused(name)
    dims = s["dims"]
    near = sp.near_samples(s["lo"], s["voxel"], s["trunc"], dims, s["views"])
    R, A = sp.required_blocks(near), sv.slots >= 0
    assert (A | ~R).all(), f"{int((R & ~A).sum())} required blocks are not allocated"
    # slots by ascending linear block index
    assert np.array_equal(np.nonzero(A.reshape(-1))[0], sv.block_of_slot)
    assert np.array_equal(sv.slots.reshape(-1)[sv.block_of_slot], np.arange(sv.n_blocks))
    # every allocated in-lattice sample carries the dense bits
    back, allocated = sp.to_dense(sv)
    for k in ("tsdf", "weight") + (("colour",) if s["colour"] else ()):
        assert np.array_equal(bits(getattr(back, k))[allocated], bits(getattr(dense, k))[allocated]), k
    # every inside sample of the dense volume is a near sample; no active cell reaches outside the allocation
    assert not ((dense.tsdf < 0) & ~near).any()
    dmesh = ts.extract(dense, 1.0)
    if min(dims) > 1:
        assert ts.corners(allocated).all(-1)[dmesh.active].all()
    smesh = sp.extract(sv, 1.0)
    assert_same_mesh(mesh_dict(dmesh), mesh_dict(smesh), dims)
    print(f"{name}: {sv.n_blocks} of {A.size} blocks allocated, {int(R.sum())} required, {int(sv.marks.sum())} marked; "
          f"{dmesh.vertices.shape[0]} vertices, {dmesh.faces.shape[0]} faces")
    if name in ("edge_ray", "corner"):      # the lattice's border between the near samples and their rays
        assert R.any() and sv.n_blocks > 0
    if name == "corner":
        assert dmesh.vertices.shape[0] == 4
    if name in ("zero", "behind"):
        assert sv.n_blocks == 0 and smesh.vertices.shape[0] == 0 and smesh.faces.shape[0] == 0
    if name in ("seam", "sphere", "nine", "border", "fine"):
        assert dmesh.faces.shape[0] > 0


def test_the_seam_and_the_corner_are_what_they_claim():
    """The seam plane's quads take their vertices from four blocks; the sphere centred on a block corner is given 27 blocks or more,
    the 8 that meet at its centre among them; the fine scene marches sub-pixel grids."""
    s, _, sv = fused("seam")
    m = sp.extract(sv)
    quads = m.faces.reshape(-1, 2, 3)
    blocks_per_quad = [len({tuple(c) for c in (m.cells[np.unique(q)] >> 3)}) for q in quads]
    assert max(blocks_per_quad) == 4
    assert {int(c) for c in m.cells[:, 2]} == {7}                      # cells whose samples lie in two layers of blocks
    s, _, sv = fused("sphere")
    m = sp.extract(sv)
    assert sv.n_blocks >= 27 and (sv.slots[1:3, 1:3, 1:3] >= 0).all()      # the 8 blocks that meet at the centre among them
    assert len({tuple(c) for c in (m.cells >> 3)}) > 8                  # (the cameras see the near half of the sphere)
    s, _, sv = fused("fine")
    _, M, _ = sp.pixel_sub(s["views"][0], s["trunc"], s["voxel"])
    assert 1 < M.max() <= sp.MAX_SUB
    s, _, sv = fused("65x7x9")
    assert (sv.weight == F(1.5)).any()                                  # max_weight binds


def test_marks_accumulate_and_a_view_that_was_not_allocated_updates_the_allocated_blocks_only():
    s, dense, sv = fused("nine")
    one = sp.new_sparse(s["lo"], s["voxel"], s["dims"], trunc=s["trunc"])
    for v in s["views"]:
        sp.mark(one, [v])
    assert np.array_equal(one.marks, sv.marks)
    part = sp.new_sparse(s["lo"], s["voxel"], s["dims"], trunc=s["trunc"], colour=True, max_weight=s["max_weight"])
    full = s["views"][0]
    first = int(np.nonzero((full.depth > 0).any(0))[0][0])                # the sphere's leftmost column in the image
    strip = ts.View(np.where(np.arange(full.W)[None, :] < first + 3, full.depth, F(0)), full.view, full.tanfovx, full.tanfovy,
                    full.z_min)
    sp.mark(part, [strip])                # allocated from three columns of one view, fused from all nine
    sp.commit(part)
    sp.integrate(part, s["views"])
    assert 0 < part.n_blocks < sv.n_blocks
    back, allocated = sp.to_dense(part)
    assert np.array_equal(bits(back.tsdf)[allocated], bits(dense.tsdf)[allocated])
    assert np.array_equal(bits(back.tsdf)[~allocated], bits(np.ones_like(back.tsdf))[~allocated])


# ---- the over-allocation bound -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seam", "border", "sphere", "nine"])
def test_every_allocated_sample_lies_within_the_derived_distance_of_the_surface(name):
    """A marched point lies on its pixel's centre ray within trunc of the surface IN DEPTH, so within trunc * |ray| <=
    trunc * sqrt(1 + tanfovx^2 + tanfovy^2) of it; a sample of the marked block or of one of its 26 neighbours lies less
    than two block diagonals, 2 sqrt(3) 8 voxel, from the point.  Derived, not measured; the cameras march M = 1."""
    s, _, sv = fused(name)
    voxel, trunc = float(s["voxel"]), float(s["trunc"])
    tx = max(float(v.tanfovx) for v in s["views"])
    ty = max(float(v.tanfovy) for v in s["views"])
    for v in s["views"]:
        assert sp.pixel_sub(v, s["trunc"], s["voxel"])[1].max() == 1
    bound = trunc * math.sqrt(1 + tx * tx + ty * ty) + 2 * math.sqrt(3.0) * 8 * voxel
    i, j, k, _ = sp.sample_coords(sv)
    shape = (sv.n_blocks, 8, 8, 8)
    x = np.stack([np.broadcast_to(s["lo"][a].astype(np.float64) + voxel * c, shape) for a, c in enumerate((i, j, k))], -1)
    kind, p, q = s["surface"]
    dist = np.abs(x @ np.asarray(p) - q) if kind == "plane" else np.abs(np.linalg.norm(x - p, axis=-1) - q)
    print(f"{name}: {sv.n_blocks} blocks, farthest allocated sample {dist.max():.4f}, bound {bound:.4f}")
    assert sv.n_blocks > 0 and dist.max() <= bound


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------
FAKE = 4096          # a non-null, aligned address: every case below is refused before anything is followed


def _sparse(**kw):
    f = dict(tsdf=FAKE, weight=FAKE, colour=None, block_of_slot=FAKE, table=FAKE, lo=(C.c_float * 3)(0, 0, 0), voxel=0.1,
             nx=20, ny=20, nz=20, trunc=0.4, max_weight=math.inf, n_blocks=3, capacity=3)
    f.update(kw)
    return _lib.TsdfSparse(**f)


def _views(n=1, **kw):
    f = dict(depth=FAKE, weight=None, rgb=None, W=8, H=6, view=(C.c_float * 12)(*([0.0] * 12)), tanfovx=1.0, tanfovy=1.0,
             z_min=0.01)
    f.update(kw)
    return (_lib.TsdfView * 8)(*[_lib.TsdfView(**f) for _ in range(n)])


def _refused(rc, *words):
    msg = _lib.lib().hgs_last_error().decode()
    assert rc == 1, (rc, msg)
    assert all(w in msg for w in words), msg


def sparse_calls():
    """name -> (call(volume, **overrides), committed): every entry point that takes a volume, on fake addresses."""
    lib = _lib.lib()
    total, totals = C.c_int64(), (C.c_int64 * 2)()
    return {
        "mark": (lambda v, views=None, n=1, tmp=FAKE: lib.hgs_tsdf_sparse_mark(C.byref(v), views or _views(), n, None, 0), False),
        "commit_plan": (lambda v, views=None, n=1, tmp=FAKE: lib.hgs_tsdf_sparse_commit_plan(C.byref(v), tmp, C.byref(total), None, 0), False),
        "commit_apply": (lambda v, views=None, n=1, tmp=FAKE: lib.hgs_tsdf_sparse_commit_apply(C.byref(v), tmp, None, 0), True),
        "integrate": (lambda v, views=None, n=1, tmp=FAKE: lib.hgs_tsdf_sparse_integrate(C.byref(v), views or _views(), n, None, 0), True),
        "extract_plan": (lambda v, views=None, n=1, tmp=FAKE: lib.hgs_tsdf_sparse_extract_plan(C.byref(v), 1.0, tmp, totals, None, 0), True),
        "extract_apply": (lambda v, views=None, n=1, tmp=FAKE: lib.hgs_tsdf_sparse_extract_apply(C.byref(v), tmp, FAKE, FAKE, None, FAKE, FAKE, None, 0), True),
    }


def test_every_call_refuses_a_bad_volume_by_name():
    for name, (call, committed) in sparse_calls().items():
        B = dict(n_blocks=3) if committed else dict(n_blocks=-1)
        _refused(call(_sparse(nx=0, **B)), "bad sizes")
        _refused(call(_sparse(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=8, **B)), "block grid", "2^31 - 1")
        _refused(call(_sparse(nx=16384 * 8, ny=16384 * 8, nz=65, **B)), "block grid")
        for bad in (0.0, -1.0, math.inf, math.nan):
            _refused(call(_sparse(voxel=bad, **B)), "voxel")
            _refused(call(_sparse(trunc=bad, **B)), "trunc")
        for bad in (0.0, -2.0, math.nan):
            _refused(call(_sparse(max_weight=bad, **B)), "max_weight")
        _refused(call(_sparse(table=None, **B)), "null", "table")
        _refused(call(_sparse(table=FAKE + 64, **B)), "table", "aligned")
        if committed:
            _refused(call(_sparse(n_blocks=-1)), "not committed")                # integrate or extract before commit
            _refused(call(_sparse(n_blocks=4, capacity=3)), "slot arrays")         # a slot array shorter than B
            _refused(call(_sparse(n_blocks=28, capacity=28)), "exceeds the block grid")
            _refused(call(_sparse(block_of_slot=None)), "null", "block_of_slot")
        else:
            _refused(call(_sparse(n_blocks=0)), "committed")                       # mark after commit
            _refused(call(_sparse(n_blocks=3)), "committed")
        if name in ("commit_plan", "commit_apply", "extract_plan", "extract_apply"):
            _refused(call(_sparse(**B), tmp=None), "null", "tmp")
            _refused(call(_sparse(**B), tmp=FAKE + 4), "tmp", "aligned")
        if name in ("integrate", "extract_plan", "extract_apply"):
            _refused(call(_sparse(tsdf=None)), "null", "tsdf")
            _refused(call(_sparse(weight=None)), "null", "weight")
            _refused(call(_sparse(tsdf=FAKE + 4)), "16-byte")
            _refused(call(_sparse(colour=FAKE + 8)), "16-byte")
        if name in ("mark", "integrate"):
            for n in (0, 9, -1):
                _refused(call(_sparse(**B), n=n), "n_views")
            _refused(call(_sparse(**B), views=_views(W=0)), "view 0", "pixels")
            _refused(call(_sparse(**B), views=_views(depth=None)), "null", "depth")
            two = _views(2)
            two[1].depth = None
            _refused(call(_sparse(**B), views=two, n=2), "depth of view 1")
    lib = _lib.lib()
    _refused(lib.hgs_tsdf_sparse_integrate(C.byref(_sparse()), _views(rgb=FAKE), 1, None, 0), "rgb", "colour")
    _refused(lib.hgs_tsdf_sparse_integrate(None, _views(), 1, None, 0), "null")
    _refused(lib.hgs_tsdf_sparse_mark(C.byref(_sparse(n_blocks=-1)), None, 1, None, 0), "null")
    # marking alone: the field of view the bound was written for, and a band of more steps than the march takes
    _refused(lib.hgs_tsdf_sparse_mark(C.byref(_sparse(n_blocks=-1)), _views(tanfovx=1.6), 1, None, 0), "field of view")
    _refused(lib.hgs_tsdf_sparse_mark(C.byref(_sparse(n_blocks=-1)), _views(tanfovy=0.0), 1, None, 0), "field of view")
    _refused(lib.hgs_tsdf_sparse_mark(C.byref(_sparse(n_blocks=-1, trunc=500.0)), _views(), 1, None, 0), "4096 voxels")
    # extraction alone
    totals = (C.c_int64 * 2)()
    big = _sparse(nx=4096, ny=4096, nz=4096, n_blocks=2796203, capacity=2796203)
    _refused(lib.hgs_tsdf_sparse_extract_plan(C.byref(big), 1.0, FAKE, totals, None, 0), "32-bit")
    for bad in (0.0, -1.0, math.inf, math.nan):
        _refused(lib.hgs_tsdf_sparse_extract_plan(C.byref(_sparse()), bad, FAKE, totals, None, 0), "min_weight")
    _refused(lib.hgs_tsdf_sparse_extract_plan(C.byref(_sparse()), 1.0, FAKE, None, None, 0), "null", "totals_host")
    _refused(lib.hgs_tsdf_sparse_commit_plan(C.byref(_sparse(n_blocks=-1)), FAKE, None, None, 0), "null", "n_blocks_host")
    apply_ = lambda v, ve=FAKE, c=None, f=FAKE, ce=FAKE: lib.hgs_tsdf_sparse_extract_apply(C.byref(v), FAKE, ve, FAKE, c, f, ce, None, 0)
    _refused(apply_(_sparse(), c=FAKE), "colours", "no colour")
    _refused(apply_(_sparse(), ve=None), "null")
    _refused(apply_(_sparse(), ce=None), "null", "cells")
    _refused(apply_(_sparse(), f=FAKE + 2), "4-byte")
    _refused(apply_(_sparse()), "hgs_tsdf_sparse_extract_plan")                  # no plan on this (device, tmp)
    _refused(lib.hgs_tsdf_sparse_commit_apply(C.byref(_sparse()), FAKE, None, 0), "hgs_tsdf_sparse_commit_plan")


def test_the_size_queries_need_no_gpu():
    lib = _lib.lib()
    up = lambda b: (b + 255) // 256 * 256
    layout = (C.c_int64 * 4)()
    for dims in ((1, 1, 1), (8, 8, 8), (9, 9, 9), (65, 7, 9), (4096, 4096, 512), (2 ** 31 - 1, 8, 8), (8192, 8192, 1024)):
        g = sp.block_grid(dims)
        G = g[0] * g[1] * g[2]
        assert lib.hgs_tsdf_sparse_table_layout(*dims, layout) == 0
        assert list(layout) == [G, up(4 * G), up(4 * G) + up(G), up(4 * G) + up(G) + 256], dims
        nblk = (G + 255) // 256
        chunks = max(1, (nblk + 8191) // 8192)
        assert lib.hgs_tsdf_sparse_commit_tmp_bytes(*dims) == up(4 * (nblk + 1)) + up(8 * chunks), dims
    assert layout[3] < 0.011 * 8192 * 8192 * 1024                     # 5 bytes per block: 0.01 bytes per virtual sample
    _refused(lib.hgs_tsdf_sparse_table_layout(0, 4, 4, layout), "bad sizes")
    _refused(lib.hgs_tsdf_sparse_table_layout(2 ** 31 - 1, 2 ** 31 - 1, 1, layout), "block grid")
    _refused(lib.hgs_tsdf_sparse_table_layout(4, 4, 4, None), "null")
    assert lib.hgs_tsdf_sparse_commit_tmp_bytes(4, -1, 4) == 0 and lib.hgs_tsdf_sparse_commit_tmp_bytes(2 ** 31 - 1, 2 ** 31 - 1, 1) == 0
    for B in (0, 1, 27, 8193, 2796202):
        b = max(B, 1)
        chunks = max(1, (b + 8191) // 8192)
        assert lib.hgs_tsdf_sparse_extract_tmp_bytes(B) == up(1024 * b) + up(512 * b) + 2 * up(4 * (b + 1)) + 2 * up(8 * chunks), B
    assert lib.hgs_tsdf_sparse_extract_tmp_bytes(-1) == 0 and lib.hgs_tsdf_sparse_extract_tmp_bytes(2796203) == 0


def test_the_struct_layout_matches_the_header():
    S = _lib.TsdfSparse
    assert C.sizeof(S) == 88 and S.table.offset == 32 and S.lo.offset == 40 and S.voxel.offset == 52
    assert S.nx.offset == 56 and S.trunc.offset == 68 and S.n_blocks.offset == 76 and S.capacity.offset == 80


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_the_class_checks_its_arguments_before_it_asks_for_a_gpu():
    from hgs.meshing import Mesh, SparseTsdfVolume
    with pytest.raises(ValueError, match="voxel"):
        SparseTsdfVolume((0, 0, 0), (1, 1, 1), 0.0)
    with pytest.raises(ValueError, match="lo <= hi"):
        SparseTsdfVolume((0, 0, 0), (1, -1, 1), 0.1)
    with pytest.raises(ValueError, match="trunc"):
        SparseTsdfVolume((0, 0, 0), (1, 1, 1), 0.1, trunc=-1.0)
    with pytest.raises(ValueError, match="max_weight"):
        SparseTsdfVolume((0, 0, 0), (1, 1, 1), 0.1, max_weight=0.0)
    with pytest.raises(ValueError, match="2\\^31 - 1 blocks"):
        SparseTsdfVolume((0, 0, 0), (2000, 2000, 2000), 0.05)           # 40001^3 samples: 1.25e11 blocks
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            SparseTsdfVolume((0, 0, 0), (400, 400, 50), 0.05)           # 8001 x 8001 x 1001 samples are fine
    assert Mesh(None, None, None, None).cells is None                   # the optional trailing field
