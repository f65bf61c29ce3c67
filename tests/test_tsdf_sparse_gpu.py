"""The sparse TSDF volume on the GPU (csrc/tsdf_sparse.hip): hgs_tsdf_sparse_mark, _commit_*,
_integrate and _extract_* against the numpy spec tests/tsdf_sparse_spec.py BIT FOR BIT -- the table, the block list, the
blocks, the mesh and its cells, in the kernels' own order -- on the scenes of tests/test_tsdf_sparse_cpu.py, every array
the kernels touch between guard words (tests/ws_guard.py), the table and both workspaces included; against the dense path
(hgs.meshing.TsdfVolume) on the same inputs; on a virtual lattice of 4096 x 4096 x 512 samples that no dense volume can
hold; and the Python layers built on them (hgs.meshing.SparseTsdfVolume, fuse_hierarchy, python -m hgs.mesh_hierarchy
--sparse)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import contribution_cases as cc
import tsdf_sparse_spec as sp
import tsdf_spec as ts
import ws_guard as wg
from hgs import _lib, synth
from test_tsdf_sparse_cpu import SCENES, assert_same_mesh, bits, fused, scene

pytestmark = pytest.mark.gpu
F = np.float32


# ---- the C ABI on guarded arrays -----------------------------------------------------------------------------------------------
def device_views(views, dev):
    keep, out = [], (_lib.TsdfView * 8)()
    for k, v in enumerate(views):
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d, w, rgb = up(v.depth), up(v.weight), up(v.rgb)
        keep += [d, w, rgb]
        out[k] = _lib.TsdfView(d.data_ptr(), None if w is None else w.data_ptr(), None if rgb is None else rgb.data_ptr(),
                               v.W, v.H, (C.c_float * 12)(*v.view.tolist()), float(v.tanfovx), float(v.tanfovy),
                               float(v.z_min))
    return out, keep


def garbage(g, dev):
    g.body.copy_(torch.randint(0, 256, (g.nbytes,), dtype=torch.uint8, device=dev))
    return g


class DeviceSparse:
    """A sparse volume driven through the C ABI, every array between guards.  ``tmp``: one workspace for the commit and the
    extraction both (handed in to be reused), filled with garbage when it is made here."""

    def __init__(self, s, dev, tmp=None):
        self.s, self.dev, self.lib = s, dev, _lib.lib()
        self.layout = (C.c_int64 * 4)()
        assert self.lib.hgs_tsdf_sparse_table_layout(*s["dims"], self.layout) == 0
        self.table = wg.guarded(self.layout[3], dev, 0x00, "table")
        self.tmp = tmp
        self.B, self.arrays = -1, {}
        self.stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def struct(self, **kw):
        s, a = self.s, self.arrays
        addr = lambda k: a[k].addr if k in a else None
        f = dict(tsdf=addr("tsdf"), weight=addr("weight"), colour=addr("colour"), block_of_slot=addr("block_of_slot"),
                 table=self.table.addr, lo=(C.c_float * 3)(*np.asarray(s["lo"], F).tolist()), voxel=float(s["voxel"]),
                 nx=s["dims"][0], ny=s["dims"][1], nz=s["dims"][2], trunc=float(s["trunc"]), max_weight=float(F(s["max_weight"])),
                 n_blocks=self.B, capacity=max(self.B, 0))
        f.update(kw)
        return _lib.TsdfSparse(**f)

    def workspace(self, nbytes):
        if self.tmp is None or self.tmp.nbytes < nbytes:
            self.tmp = garbage(wg.guarded(nbytes, self.dev, 0xFF, "tmp"), self.dev)
        return self.tmp

    def mark(self, views, per_call=8):
        for g0 in range(0, len(views), per_call):
            arr, keep = device_views(views[g0:g0 + per_call], self.dev)
            v = self.struct()
            _lib.check(self.lib.hgs_tsdf_sparse_mark(C.byref(v), arr, len(keep) // 3, self.stream, 0), "mark")
            torch.cuda.synchronize()
        return self

    def commit(self):
        tmp = self.workspace(max(self.lib.hgs_tsdf_sparse_commit_tmp_bytes(*self.s["dims"]), 256))
        total = C.c_int64(-7)
        v = self.struct()
        _lib.check(self.lib.hgs_tsdf_sparse_commit_plan(C.byref(v), tmp.addr, C.byref(total), self.stream, 0), "commit_plan")
        self.B = B = int(total.value)
        for name, per, fill in (("tsdf", 2048, 1.0), ("weight", 2048, 0.0), ("colour", 6144, 0.0)):
            if name == "colour" and not self.s["colour"]:
                continue
            g = wg.guarded(per * B, self.dev, 0x00, name)
            g.view(torch.float32).fill_(fill)
            self.arrays[name] = g
        self.arrays["block_of_slot"] = wg.guarded(4 * B, self.dev, 0xFF, "block_of_slot")
        v = self.struct()
        _lib.check(self.lib.hgs_tsdf_sparse_commit_apply(C.byref(v), tmp.addr, self.stream, 0), "commit_apply")
        return self

    def integrate(self, views, per_call=8):
        for g0 in range(0, len(views), per_call):
            arr, keep = device_views(views[g0:g0 + per_call], self.dev)
            v = self.struct()
            _lib.check(self.lib.hgs_tsdf_sparse_integrate(C.byref(v), arr, len(keep) // 3, self.stream, 0), "integrate")
            torch.cuda.synchronize()
        return self

    def extract(self, min_weight=1.0):
        tmp = self.workspace(self.lib.hgs_tsdf_sparse_extract_tmp_bytes(self.B))
        totals = (C.c_int64 * 2)(-7, -7)
        v = self.struct()
        _lib.check(self.lib.hgs_tsdf_sparse_extract_plan(C.byref(v), float(min_weight), tmp.addr, totals, self.stream, 0), "extract_plan")
        V, Q = int(totals[0]), int(totals[1])
        out = dict(vertices=wg.guarded(12 * V, self.dev, 0xFF, "vertices"), normals=wg.guarded(12 * V, self.dev, 0xFF, "normals"),
                   faces=wg.guarded(24 * Q, self.dev, 0xFF, "faces"), cells=wg.guarded(12 * V, self.dev, 0xFF, "cells"))
        if self.s["colour"]:
            out["colours"] = wg.guarded(12 * V, self.dev, 0xFF, "colours")
        _lib.check(self.lib.hgs_tsdf_sparse_extract_apply(C.byref(v), tmp.addr, out["vertices"].addr, out["normals"].addr,
                                                          out["colours"].addr if "colours" in out else None, out["faces"].addr,
                                                          out["cells"].addr, self.stream, 0), "extract_apply")
        self.check(*out.values())
        mesh = {k: g.body.cpu().numpy().view(np.int32 if k in ("faces", "cells") else F).reshape(-1, 3) for k, g in out.items()}
        mesh.setdefault("colours", None)
        return mesh

    def check(self, *more):
        wg.check(self.table, *self.arrays.values(), *([self.tmp] if self.tmp is not None else []), *more)

    def read(self):
        G, gx, gy, gz = self.layout[0], *sp.block_grid(self.s["dims"])
        t = self.table.body.cpu().numpy()
        out = dict(slots=t[:4 * G].view(np.int32).reshape(gz, gy, gx), marks=t[self.layout[1]:self.layout[1] + G].reshape(gz, gy, gx) != 0,
                   refusal=int(t[self.layout[2]:self.layout[2] + 4].view(np.uint32)[0]))
        for k, g in self.arrays.items():
            a = g.body.cpu().numpy()
            out[k] = a.view(np.int32) if k == "block_of_slot" else a.view(F).reshape((self.B, 8, 8, 8) + ((3,) if k == "colour" else ()))
        return out


def run_scene(s, dev, per_call=8, tmp=None):
    d = DeviceSparse(s, dev, tmp).mark(s["views"], per_call).commit().integrate(s["views"])
    d.check()
    mesh = d.extract()
    d.check()
    return d, d.read(), mesh


def assert_equals_the_spec(got, mesh, sv, smesh, colour):
    assert np.array_equal(got["marks"], sv.marks) and got["refusal"] == 0
    assert np.array_equal(got["slots"], sv.slots)
    assert np.array_equal(got["block_of_slot"], sv.block_of_slot)
    for k in ("tsdf", "weight") + (("colour",) if colour else ()):
        assert np.array_equal(bits(got[k]), bits(getattr(sv, k))), (k, int((bits(got[k]) != bits(getattr(sv, k))).sum()))
    assert mesh["vertices"].shape == smesh.vertices.shape and mesh["faces"].shape == smesh.faces.shape
    assert np.array_equal(mesh["cells"], smesh.cells)
    assert np.array_equal(bits(mesh["vertices"]), bits(smesh.vertices))
    assert np.array_equal(bits(mesh["normals"]), bits(smesh.normals))
    assert np.array_equal(mesh["faces"], smesh.faces)
    if colour:
        assert np.array_equal(bits(mesh["colours"]), bits(smesh.colours))


@pytest.mark.parametrize("name", SCENES)
def test_the_kernels_equal_the_spec_bit_for_bit(gpu, name):
    """Mark, commit, integrate, extract: every array against the spec; then the same with one mark call per view and with
    the first run's workspace reused instead of a fresh one full of garbage: identical bytes."""
    s, _, sv = fused(name)
    smesh = sp.extract(sv, 1.0)
    d, got, mesh = run_scene(s, gpu)
    assert d.B == sv.n_blocks
    assert_equals_the_spec(got, mesh, sv, smesh, s["colour"])
    print(f"{name}: {d.B} blocks, {mesh['vertices'].shape[0]} vertices, {mesh['faces'].shape[0]} faces")
    d2, got2, mesh2 = run_scene(s, gpu, per_call=1, tmp=d.tmp)
    for k in got:
        assert np.array_equal(np.atleast_1d(got[k]).view(np.uint8), np.atleast_1d(got2[k]).view(np.uint8)), k
    for k in mesh:
        assert (mesh[k] is None and mesh2[k] is None) or np.array_equal(mesh[k].view(np.uint32), mesh2[k].view(np.uint32)), k
    if d.B == 0:            # nothing was written anywhere
        assert not got["marks"].any() and (got["slots"] == -1).all()
        assert all(mesh[k].shape == (0, 3) for k in ("vertices", "normals", "faces", "cells"))


def test_another_min_weight_and_a_view_that_was_not_allocated(gpu):
    """Extraction at min_weight 3 of the nine-view sphere; then a volume allocated from a strip of one view and fused from
    all nine: the allocated blocks carry the spec's bits, and the dense ones."""
    s, dense, sv = fused("nine")
    d = DeviceSparse(s, gpu).mark(s["views"]).commit().integrate(s["views"])
    want = sp.extract(sv, 3.0)
    mesh = d.extract(3.0)
    assert 0 < want.vertices.shape[0] < sp.extract(sv, 1.0).vertices.shape[0]
    assert np.array_equal(bits(mesh["vertices"]), bits(want.vertices)) and np.array_equal(mesh["faces"], want.faces)
    full = s["views"][0]
    first = int(np.nonzero((full.depth > 0).any(0))[0][0])
    strip = ts.View(np.where(np.arange(full.W)[None, :] < first + 3, full.depth, F(0)), full.view, full.tanfovx, full.tanfovy,
                    full.z_min)
    part = sp.new_sparse(s["lo"], s["voxel"], s["dims"], trunc=s["trunc"], colour=True, max_weight=s["max_weight"])
    sp.integrate(sp.commit(sp.mark(part, [strip])), s["views"])
    d = DeviceSparse(s, gpu).mark([strip]).commit().integrate(s["views"])
    d.check()
    got = d.read()
    assert 0 < d.B == part.n_blocks < sv.n_blocks
    for k in ("tsdf", "weight", "colour"):
        assert np.array_equal(bits(got[k]), bits(getattr(part, k))), k
    back, allocated = sp.to_dense(part)
    assert np.array_equal(bits(back.tsdf)[allocated], bits(dense.tsdf)[allocated])


# ---- against the dense path ------------------------------------------------------------------------------------------------------
def python_volumes(s, dev):
    """The scene through hgs.meshing on both paths: (SparseTsdfVolume, TsdfVolume), fused."""
    from hgs.meshing import SparseTsdfVolume, TsdfVolume
    dims = np.array(s["dims"])
    hi = s["lo"].astype(np.float64) + float(s["voxel"]) * (dims - 1) + 0.25 * float(s["voxel"])
    cams = s["cams"]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    kw = dict(trunc=float(s["trunc"]), colour=s["colour"], max_weight=float(F(s["max_weight"])), device=dev)
    depths, images = [t(v.depth) for v in s["views"]], [t(v.rgb) for v in s["views"]]
    sparse = SparseTsdfVolume(s["lo"], hi, float(s["voxel"]), **kw)
    assert sparse.dims == s["dims"]
    half = len(cams) // 2
    sparse.allocate(depths[:half], cams[:half]).allocate(depths[half:], cams[half:])
    sparse.commit().integrate(depths, cams, images=images if s["colour"] else None)
    dense = TsdfVolume(s["lo"], hi, float(s["voxel"]), **kw)
    dense.integrate(depths, cams, images=images if s["colour"] else None)
    return sparse, dense


def camera_scene(name):
    """A scene with cameras for the Python layer (the views of ``scene`` carry matrices only)."""
    s = dict(scene(name))
    if s["cams"] is None:
        assert name in ("seam", "border")
        s["cams"] = [synth.make_camera(80, 60)]
        s["views"] = [ts.view_of(s["cams"][0], s["views"][0].depth)]          # (z_min = the camera's znear)
    else:
        s["views"] = [ts.view_of(c, v.depth, rgb=v.rgb) for c, v in zip(s["cams"], s["views"])]
    return s


@pytest.mark.parametrize("name", ["seam", "sphere", "nine", "border"])
def test_the_sparse_path_equals_the_dense_path(gpu, name):
    """hgs.meshing.SparseTsdfVolume against hgs.meshing.TsdfVolume on the same depth maps: every allocated in-lattice sample
    has the dense bits, to_dense() equals the dense arrays wherever it is allocated, the meshes are equal."""
    s = camera_scene(name)
    sparse, dense = python_volumes(s, gpu)
    back, allocated = sparse.to_dense(return_allocated=True)
    allocated = allocated.cpu().numpy()
    a, b = back.numpy(), dense.numpy()
    assert allocated.any() and not allocated.all() or name in ("seam", "border")
    for k in ("tsdf", "weight") + (("colour",) if s["colour"] else ()):
        assert np.array_equal(bits(a[k])[allocated], bits(b[k])[allocated]), k
        fresh = np.ones_like(a[k]) if k == "tsdf" else np.zeros_like(a[k])
        assert np.array_equal(bits(a[k])[~allocated], bits(fresh)[~allocated]), k
    # the blocks themselves, through numpy(): the spec's on the same inputs
    sv = sp.new_sparse(s["lo"], s["voxel"], s["dims"], trunc=s["trunc"], colour=s["colour"], max_weight=s["max_weight"])
    sp.integrate(sp.commit(sp.mark(sv, s["views"])), s["views"])
    got = sparse.numpy()
    assert sparse.n_blocks == sv.n_blocks and np.array_equal(got["slots"], sv.slots)
    assert np.array_equal(got["block_of_slot"], sv.block_of_slot) and np.array_equal(bits(got["tsdf"]), bits(sv.tsdf))
    # the meshes; the dense mesh has no cells: its vertices are in ascending cell order, the cells from the spec
    sm, dm = sparse.extract(), dense.extract()
    assert dm.cells is None and sm.cells is not None and sm.vertices.shape[0] > 0
    spec_dense = ts.Volume(s["lo"], s["voxel"], s["trunc"], F(s["max_weight"]), b["tsdf"], b["weight"], b.get("colour"))
    dmesh = dict(dm.numpy(), cells=ts.extract(spec_dense, 1.0).cells)
    dmesh.setdefault("colours", None)
    smesh = sm.numpy()
    smesh.setdefault("colours", None)
    assert_same_mesh(dmesh, smesh, s["dims"])
    print(f"{name}: {sparse.n_blocks} blocks = {sparse.nbytes} bytes against {sum(v.nbytes for v in b.values() if hasattr(v, 'nbytes'))} dense; "
          f"{sm.vertices.shape[0]} vertices")


# ---- a lattice the dense path cannot hold ----------------------------------------------------------------------------------------
def test_a_virtual_lattice_of_more_than_two_to_the_31_samples(gpu):
    """4096 x 4096 x 512 samples (a 67 MB table): a plane patch far from the origin corner under the middle of an 80 x 60
    view.  Slots, block list, blocks and mesh equal the spec; the cells' linear indices lie above 2^31."""
    from hgs.meshing import SparseTsdfVolume, TsdfVolume
    voxel, dims = 0.05, (4096, 4096, 512)
    lo = np.array([-102.4, -102.4, 0.0], F)
    hi = lo.astype(np.float64) + voxel * (np.array(dims) - 1) + 0.25 * voxel
    cam = synth.make_camera(80, 60)
    depth = ts.plane_depth(cam, (0.0, 0.0, 1.0), 20.02).astype(F)
    depth[:, :30] = 0
    depth[:, 50:] = 0
    depth[:22] = 0
    depth[38:] = 0
    view = ts.view_of(cam, depth)
    vol = SparseTsdfVolume(lo, hi, voxel, device=gpu)
    assert vol.dims == dims and np.prod(dims, dtype=np.int64) > 2 ** 31
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        TsdfVolume(lo, hi, voxel, device=gpu)
    vol.allocate([torch.from_numpy(depth)], [cam]).commit().integrate([torch.from_numpy(depth)], [cam])
    with pytest.raises(ValueError, match="dense volume holds at most"):
        vol.to_dense()
    sv = sp.new_sparse(lo, voxel, dims)
    sp.integrate(sp.commit(sp.mark(sv, [view])), [view])
    assert sp.pixel_sub(view, sv.trunc, sv.voxel)[1].max() > 1           # sub-pixel positions at this distance
    got = vol.numpy()
    assert vol.n_blocks == sv.n_blocks > 100
    assert np.array_equal(got["marks"] != 0, sv.marks) and np.array_equal(got["slots"], sv.slots)
    assert np.array_equal(got["block_of_slot"], sv.block_of_slot)
    assert np.array_equal(bits(got["tsdf"]), bits(sv.tsdf)) and np.array_equal(bits(got["weight"]), bits(sv.weight))
    mesh, want = vol.extract().numpy(), sp.extract(sv, 1.0)
    assert np.array_equal(mesh["cells"], want.cells) and np.array_equal(mesh["faces"], want.faces)
    assert np.array_equal(bits(mesh["vertices"]), bits(want.vertices)) and np.array_equal(bits(mesh["normals"]), bits(want.normals))
    c = mesh["cells"].astype(np.int64)
    linear = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    print(f"{dims}: {vol.n_blocks} blocks, {vol.nbytes} bytes held, {c.shape[0]} vertices, linear sample indices from {linear.min()}")
    assert c.shape[0] > 1000 and linear.min() > 2 ** 31
    assert np.abs(mesh["vertices"][:, 2] - 20.02).max() < voxel


def wide_plane():
    """A thin plane over a wide, flat lattice: 608 x 608 x 16 samples under an 80 x 60 view, two layers of 76 x 76
    blocks, the plane in the upper one: more than 8192 blocks, the vertices in those past the first scan chunk."""
    voxel, dims = 0.01, (608, 608, 16)
    lo = np.array([-3.04, -3.04, 4.885], F)              # the plane between the samples 11 and 12 along z
    cam = synth.make_camera(80, 60)
    depth = ts.plane_depth(cam, (0.0, 0.0, 1.0), 5.0).astype(F)
    return voxel, dims, lo, cam, depth


def test_extraction_where_the_block_scan_takes_a_second_chunk(gpu):
    """More than 8192 allocated blocks: the chained scan over the per-block vertex and quad counts runs over two chunks.
    Blocks, block list and mesh against the spec."""
    from hgs.meshing import SparseTsdfVolume
    voxel, dims, lo, cam, depth = wide_plane()
    hi = lo.astype(np.float64) + voxel * (np.array(dims) - 1) + 0.25 * voxel
    view = ts.view_of(cam, depth)
    sv = sp.new_sparse(lo, voxel, dims)
    sp.integrate(sp.commit(sp.mark(sv, [view])), [view])
    assert sv.n_blocks > 8192
    vol = SparseTsdfVolume(lo, hi, voxel, device=gpu)
    assert vol.dims == dims
    vol.allocate([torch.from_numpy(depth)], [cam]).commit().integrate([torch.from_numpy(depth)], [cam])
    got = vol.numpy()
    assert vol.n_blocks == sv.n_blocks and np.array_equal(got["block_of_slot"], sv.block_of_slot)
    assert np.array_equal(bits(got["tsdf"]), bits(sv.tsdf)) and np.array_equal(bits(got["weight"]), bits(sv.weight))
    mesh, want = vol.extract().numpy(), sp.extract(sv, 1.0)
    print(f"{dims}: {vol.n_blocks} blocks, {want.vertices.shape[0]} vertices, {want.faces.shape[0]} faces")
    assert want.vertices.shape[0] > 100000
    assert np.array_equal(mesh["cells"], want.cells) and np.array_equal(mesh["faces"], want.faces)
    assert np.array_equal(bits(mesh["vertices"]), bits(want.vertices)) and np.array_equal(bits(mesh["normals"]), bits(want.normals))
    b = mesh["cells"] >> 3
    assert sv.slots[b[:, 2], b[:, 1], b[:, 0]].max() >= 8192             # vertices from blocks of the second chunk


# ---- refusals on real arrays ---------------------------------------------------------------------------------------------------
def test_refusals_leave_every_array_untouched(gpu):
    s, _, sv = fused("9x9x9")
    lib = _lib.lib()
    d = DeviceSparse(s, gpu)
    arr, keep = device_views(s["views"], gpu)
    n = len(s["views"])
    refused = lambda rc, *words: (rc == 1 and all(w in lib.hgs_last_error().decode() for w in words)) or \
        pytest.fail(f"{rc}: {lib.hgs_last_error().decode()}")
    tmp = d.workspace(4096)
    # before the commit: no integrate, no extract, no commit apply
    v = d.struct()
    totals = (C.c_int64 * 2)()
    refused(lib.hgs_tsdf_sparse_integrate(C.byref(v), arr, n, None, 0), "not committed")
    refused(lib.hgs_tsdf_sparse_extract_plan(C.byref(v), 1.0, tmp.addr, totals, None, 0), "not committed")
    refused(lib.hgs_tsdf_sparse_commit_apply(C.byref(v), tmp.addr, None, 0), "not committed")
    wide = device_views([ts.View(s["views"][0].depth, s["views"][0].view, F(1.6), F(1.0), F(0.05))], gpu)
    refused(lib.hgs_tsdf_sparse_mark(C.byref(v), wide[0], 1, None, 0), "field of view")
    torch.cuda.synchronize()
    assert bool((d.table.body == 0).all())
    d.mark(s["views"]).commit()
    before = {k: g.raw.clone() for k, g in list(d.arrays.items()) + [("table", d.table)]}
    # after it: no mark, no second plan; a slot array shorter than B; an apply without its plan
    v = d.struct()
    total = C.c_int64()
    refused(lib.hgs_tsdf_sparse_mark(C.byref(v), arr, n, None, 0), "committed")
    refused(lib.hgs_tsdf_sparse_commit_plan(C.byref(v), tmp.addr, C.byref(total), None, 0), "committed")
    short = d.struct(capacity=d.B - 1)
    refused(lib.hgs_tsdf_sparse_integrate(C.byref(short), arr, n, None, 0), "slot arrays")
    refused(lib.hgs_tsdf_sparse_extract_plan(C.byref(short), 1.0, tmp.addr, totals, None, 0), "slot arrays")
    other = d.struct(n_blocks=d.B - 1)
    refused(lib.hgs_tsdf_sparse_commit_apply(C.byref(other), tmp.addr, None, 0), "hgs_tsdf_sparse_commit_plan")
    out = wg.guarded(4096, gpu, 0xFF, "out")
    refused(lib.hgs_tsdf_sparse_extract_apply(C.byref(v), tmp.addr, out.addr, out.addr, None, out.addr, out.addr, None, 0),
            "hgs_tsdf_sparse_extract_plan")
    refused(lib.hgs_tsdf_sparse_extract_plan(C.byref(d.struct(table=d.table.addr + 64)), 1.0, tmp.addr, totals, None, 0), "table")
    refused(lib.hgs_tsdf_sparse_extract_plan(C.byref(v), 1.0, tmp.addr + 8, totals, None, 0), "tmp")
    d.check(out)
    assert bool((out.body == 0xFF).all())
    for k, g in list(d.arrays.items()) + [("table", d.table)]:
        assert torch.equal(g.raw, before[k]), k


def test_a_pixel_beyond_the_sub_pixel_cap_refuses_the_commit(gpu):
    """Found on the device, reported by the commit plan's one wait: a footprint of more than 16 x 2 voxels."""
    from hgs.meshing import SparseTsdfVolume
    cam = synth.make_camera(8, 8)
    depth = torch.ones((8, 8))
    depth[7, 7] = 50.0
    vol = SparseTsdfVolume((0, 0, 0), (0.63, 0.63, 1.99), 0.01, device=gpu).allocate([depth], [cam])
    with pytest.raises(RuntimeError, match="sub-pixel grid"):
        vol.commit()
    assert vol.n_blocks is None
    with pytest.raises(RuntimeError, match="before commit"):
        vol.integrate([depth], [cam])
    wide = synth.make_camera(8, 8, fovy_deg=120.0)
    with pytest.raises(ValueError, match="field of view"):
        SparseTsdfVolume((0, 0, 0), (1, 1, 1), 0.1, device=gpu).allocate([depth], [wide])
    ok = SparseTsdfVolume((0, 0, 0), (1, 1, 1), 0.1, device=gpu).commit()
    assert ok.n_blocks == 0 and ok.extract().vertices.shape == (0, 3) and ok.extract().cells.shape == (0, 3)
    with pytest.raises(RuntimeError, match="after commit"):
        ok.allocate([depth], [cam])


# ---- end to end ------------------------------------------------------------------------------------------------------------------
ROI_LO, ROI_HI, VOXEL = (-2.0, -1.5, 2.0), (2.0, 1.5, 8.0), 0.125


def e2e_cameras():
    return [synth.orbit_camera(96, 64, k, 6) for k in range(6)]


@pytest.fixture(scope="module")
def hier(gpu):
    return cc.on_device(cc.hier2000(), gpu)


def test_fuse_hierarchy_into_a_sparse_volume_equals_the_dense_fuse(gpu, hier):
    from hgs.meshing import SparseTsdfVolume, TsdfVolume, fuse_hierarchy
    cams = e2e_cameras()
    dense = fuse_hierarchy(hier, cams, TsdfVolume(ROI_LO, ROI_HI, VOXEL, colour=True, device=gpu))
    sparse = SparseTsdfVolume(ROI_LO, ROI_HI, VOXEL, colour=True, device=gpu)
    assert fuse_hierarchy(hier, cams, sparse) is sparse and sparse.n_blocks > 0
    again = fuse_hierarchy(hier, cams, SparseTsdfVolume(ROI_LO, ROI_HI, VOXEL, colour=True, device=gpu), keep_depth_bytes=0)
    assert torch.equal(again.tsdf, sparse.tsdf) and torch.equal(again.colour, sparse.colour)      # rendered again: the same
    back, allocated = sparse.to_dense(return_allocated=True)
    for k in ("tsdf", "weight", "colour"):
        assert torch.equal(getattr(back, k)[allocated], getattr(dense, k)[allocated]), k
    sm, dm = sparse.extract(), dense.extract()
    b = dense.numpy()
    spec_dense = ts.Volume(b["lo"], b["voxel"], b["trunc"], b["max_weight"], b["tsdf"], b["weight"], b["colour"])
    dmesh = dict(dm.numpy(), cells=ts.extract(spec_dense, 1.0).cells)
    assert dm.vertices.shape[0] > 0
    assert_same_mesh(dmesh, sm.numpy(), dense.dims)
    with pytest.raises(RuntimeError, match="not committed"):
        fuse_hierarchy(hier, cams, sparse)


def test_the_command_meshes_sparsely(gpu, hier, tmp_path, capsys):
    from gaussian_hierarchy._C import write_hierarchy
    from hgs import mesh_hierarchy as mh
    from test_tsdf_cpu import read_ply
    host = cc.hier2000()
    path, cams = tmp_path / "in.hier", tmp_path / "cameras.json"
    write_hierarchy(str(path), *[getattr(host, k) for k in cc.FIELDS])
    cams.write_text(json.dumps([cc.camera_entry(c) for c in e2e_cameras()]))
    args = [str(path), "--cameras", str(cams), "--voxel", str(VOXEL), "--roi"] + [str(v) for v in ROI_LO + ROI_HI]
    dense_out, sparse_out, vout = tmp_path / "dense.ply", tmp_path / "sparse.ply", tmp_path / "v.npz"
    assert mh.main(args[:1] + [str(dense_out)] + args[1:]) == 0
    capsys.readouterr()
    assert mh.main(args[:1] + [str(sparse_out)] + args[1:] + ["--sparse", "--volume-out", str(vout)]) == 0
    text = capsys.readouterr().out
    a, b = read_ply(dense_out), read_ply(sparse_out)
    V, Fc = b["vertices"].shape[0], b["faces"].shape[0]
    assert V > 0 and f"{V} vertices, {Fc} faces" in text and "sparse: " in text and "blocks of 512 allocated" in text
    assert a["vertices"].shape == b["vertices"].shape and a["faces"].shape == b["faces"].shape
    order = lambda v: v[np.lexsort(v.T[::-1])]
    assert np.array_equal(bits(order(a["vertices"])), bits(order(b["vertices"])))
    z = np.load(vout)
    assert z["tsdf"].shape[1:] == (8, 8, 8) and z["slots"].shape == (7, 4, 5) and f"sparse: {z['tsdf'].shape[0]} blocks" in text
    assert mh.parse_args(["a", "b", "--cameras", "c", "--voxel", "1", "--roi-root", "--sparse"])["sparse"] is True
    assert mh.parse_args(["a", "b", "--cameras", "c", "--voxel", "1", "--roi-root", "--sparse", "--sparse"]) is None
    # a region no dense volume holds is taken with --sparse (and refused, the voxel named, without)
    assert mh.checked_region((0, 0, 0, 100, 100, 100), 0.0625, sparse=True)[2] == (1601, 1601, 1601)
    with pytest.raises(ValueError, match="fits"):
        mh.checked_region((0, 0, 0, 100, 100, 100), 0.0625)
    with pytest.raises(ValueError, match="blocks"):
        mh.checked_region((0, 0, 0, 1000, 1000, 1000), 0.01, sparse=True)
