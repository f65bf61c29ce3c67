"""hgs_tsdf_integrate and hgs_tsdf_extract_plan / _apply on the GPU against the numpy spec (tests/tsdf_spec.py), BIT FOR
BIT, and the Python layers built on them (hgs/meshing.py, python -m hgs.mesh_hierarchy).

Volumes 1x1x1 .. 65x7x9 are off the 4-sample vector, off the wave and off 16-byte row alignment (a row of 65, 37 or 5
floats starts 16-byte aligned every fourth row only; one case also starts the arrays 4 bytes past the alignment);
images 1x1 .. 80x60; 1, 2, 8 views per call and 9 through Python.  Every array the kernels write sits between guard words
(tests/ws_guard.py)."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import contribution_cases as cc
import tsdf_spec as ts
import ws_guard as wg
from hgs import _lib, synth
from test_tsdf_cpu import SPHERE_C, SPHERE_R, read_ply, sphere_scene

pytestmark = pytest.mark.gpu
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- the C ABI on guarded arrays ---------------------------------------------------------------------------------------------
class DeviceVolume:
    """A spec volume's arrays on the device, each between guards; ``shift`` floats past the 256-byte alignment."""

    def __init__(self, vol: ts.Volume, dev, shift=0):
        self.vol, self.dev, self.shift = vol, dev, shift
        self.guards = {}
        for name in ("tsdf", "weight", "colour"):
            a = getattr(vol, name)
            if a is None:
                continue
            g = wg.guarded(a.nbytes + 4 * shift, dev, 0x00, name)
            if shift:
                g.raw[g.off:g.off + 4 * shift] = wg.PATTERN            # (the shifted-over bytes belong to the guard)
            g.raw[g.off + 4 * shift:g.off + g.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8)).to(dev)
            self.guards[name] = g

    def addr(self, name):
        return None if name not in self.guards else self.guards[name].addr + 4 * self.shift

    def struct(self):
        v = self.vol
        nx, ny, nz = v.dims
        return _lib.TsdfVolume(self.addr("tsdf"), self.addr("weight"), self.addr("colour"), (C.c_float * 3)(*v.lo.tolist()),
                               float(v.voxel), nx, ny, nz, float(v.trunc), float(v.max_weight))

    def read(self, name):
        g = self.guards[name]
        raw = g.raw[g.off + 4 * self.shift:g.off + g.nbytes].cpu().numpy()
        return raw.view(F).reshape(getattr(self.vol, name).shape)

    def check(self):
        wg.check(*self.guards.values())
        for g in self.guards.values():
            assert bool((g.raw[g.off:g.off + 4 * self.shift] == wg.PATTERN).all()), f"{g.name}: bytes before the array written"


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


def integrate_on_device(dv: DeviceVolume, views, per_call=8):
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream(dv.dev).cuda_stream)
    for g0 in range(0, len(views), per_call):
        group = views[g0:g0 + per_call]
        arr, keep = device_views(group, dv.dev)
        vol = dv.struct()
        _lib.check(lib.hgs_tsdf_integrate(C.byref(vol), arr, len(group), stream, 0), "hgs_tsdf_integrate")
        torch.cuda.synchronize()
        del keep


# ---- integrate ------------------------------------------------------------------------------------------------------------------
def random_views(rng, n, W, H, centre_z, trunc, weight, colour):
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
        views.append(ts.view_of(cam, depth, w, rgb, z_min=0.05))
    return views


def make_volume(rng, dims, colour, prior, z0, max_weight):
    nx, ny, nz = dims
    voxel = F(1.3 / max(dims)) if max(dims) > 1 else F(0.1)
    lo = (F(-0.5) * voxel * F(nx - 1) + F(0.013), F(-0.5) * voxel * F(ny - 1) - F(0.007), F(z0))
    vol = ts.new_volume(lo, voxel, dims, trunc=F(2.5) * voxel, colour=colour, max_weight=max_weight)
    if prior:                # a volume that has seen views before
        vol.tsdf[:] = (2 * rng.random(vol.tsdf.shape) - 1).astype(F)
        vol.weight[:] = (3 * rng.random(vol.weight.shape)).astype(F)
        if colour:
            vol.colour[:] = rng.random(vol.colour.shape).astype(F)
    return vol


#        dims          image     views weight colour prior  z0    max_weight shift
CASES = [((1, 1, 1), (1, 1), 1, False, False, False, 1.0, np.inf, 0),
         ((1, 1, 1), (7, 5), 2, True, True, True, 1.0, 2.5, 0),
         ((2, 2, 2), (7, 5), 2, True, True, False, 1.0, np.inf, 0),
         ((2, 2, 2), (80, 60), 8, False, False, True, -0.05, 3.5, 1),
         ((5, 3, 2), (33, 17), 8, False, True, False, 1.0, 2.5, 0),
         ((5, 3, 2), (1, 1), 1, True, False, True, 0.5, np.inf, 3),
         ((37, 21, 13), (80, 60), 8, True, True, True, 0.9, 4.0, 0),
         ((37, 21, 13), (33, 17), 1, False, False, False, -0.1, np.inf, 0),
         ((64, 64, 8), (80, 60), 8, True, False, False, 1.0, 3.0, 0),
         ((64, 64, 8), (7, 5), 2, False, True, True, 1.0, np.inf, 1),
         ((65, 7, 9), (33, 17), 2, False, True, False, 1.0, np.inf, 0),
         ((65, 7, 9), (80, 60), 8, True, True, True, -0.2, 2.0, 2)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])) + "_" + "x".join(map(str, c[1])) + f"_v{c[2]}")
def test_integrate_equals_the_spec_bit_for_bit(gpu, case):
    dims, (W, H), n_views, weight, colour, prior, z0, max_weight, shift = case
    rng = np.random.default_rng(abs(hash((dims, W, n_views))) % 2 ** 31)
    vol = make_volume(rng, dims, colour, prior, z0, max_weight)
    centre_z = float(z0) + 0.5 * float(vol.voxel) * dims[2]
    views = random_views(rng, n_views, W, H, max(centre_z, 0.6), float(vol.trunc), weight, colour)
    init = vol.copy()
    dv = DeviceVolume(vol, gpu, shift)
    integrate_on_device(dv, views)
    dv.check()
    seen = ts.integrate(vol, views)
    names = ("tsdf", "weight") + (("colour",) if colour else ())
    for name in names:
        got, want = dv.read(name), getattr(vol, name)
        assert np.array_equal(bits(got), bits(want)), (name, int((bits(got) != bits(want)).sum()))
        assert np.array_equal(bits(got)[~seen], bits(getattr(init, name))[~seen]), name       # untouched where unseen
    changed = bits(vol.weight) != bits(init.weight)
    print(f"{dims}: {int(seen.sum())} of {seen.size} samples seen, {int(changed.sum())} updated, "
          f"{int((vol.weight == vol.max_weight).sum())} at max_weight")
    if n_views > 1:          # one call with V views = V calls
        one = DeviceVolume(init, gpu, shift)
        integrate_on_device(one, views, per_call=1)
        one.check()
        for name in names:
            assert np.array_equal(bits(one.read(name)), bits(dv.read(name))), name


def test_the_cases_cover_every_branch_of_the_rule():
    """Over CASES (spec only): unseen samples behind the camera and outside the image, holes, NaN depths, zero weights,
    sdf on both sides of -trunc, clipping at 1, max_weight binding, ragged and unaligned rows."""
    tally = dict(behind=0, outside=0, hole=0, nan=0, noweight=0, beyond=0, inband=0, clipped=0, capped=0)
    for dims, (W, H), n_views, weight, colour, prior, z0, max_weight, shift in CASES:
        rng = np.random.default_rng(abs(hash((dims, W, n_views))) % 2 ** 31)
        vol = make_volume(rng, dims, colour, prior, z0, max_weight)
        centre_z = float(z0) + 0.5 * float(vol.voxel) * dims[2]
        views = random_views(rng, n_views, W, H, max(centre_z, 0.6), float(vol.trunc), weight, colour)
        nx, ny, nz = dims
        x = (ts.lattice(vol.lo[0], vol.voxel, nx)[None, None, :], ts.lattice(vol.lo[1], vol.voxel, ny)[None, :, None],
             ts.lattice(vol.lo[2], vol.voxel, nz)[:, None, None])
        for v in views:
            ok, z, px, py = ts.project(*x, v)
            ok, z = np.broadcast_to(ok, (nz, ny, nx)), np.broadcast_to(z, (nz, ny, nx))
            d = v.depth[py, px]
            w = v.weight[py, px] if v.weight is not None else np.ones_like(d)
            with np.errstate(invalid="ignore"):
                sdf = d - z
                tally["behind"] += int((z <= v.z_min).sum())
                tally["outside"] += int(((z > v.z_min) & ~ok).sum())
                tally["hole"] += int((ok & (d == 0)).sum())
                tally["nan"] += int((ok & np.isnan(d)).sum())
                tally["noweight"] += int((ok & (d > 0) & (w == 0)).sum())
                tally["beyond"] += int((ok & (d > 0) & (w > 0) & (sdf < -vol.trunc)).sum())
                tally["inband"] += int((ok & (d > 0) & (w > 0) & (sdf >= -vol.trunc) & (sdf < vol.trunc)).sum())
                tally["clipped"] += int((ok & (d > 0) & (w > 0) & (sdf >= vol.trunc)).sum())
            ts.integrate(vol, [v])
        tally["capped"] += int((vol.weight == vol.max_weight).sum())
    print(tally)
    assert all(n > 0 for n in tally.values()), tally


def test_nine_views_through_python_are_split_into_eight_and_one(gpu):
    from hgs.meshing import TsdfVolume
    rng = np.random.default_rng(5)
    dims, voxel = (37, 21, 13), 0.04
    lo = np.array([-0.7, -0.4, 1.0], F)
    hi = lo.astype(np.float64) + voxel * (np.array(dims) - 1) + 1e-4
    cams = [synth.orbit_camera(33, 17, k, 9, radius=0.3, tilt=0.1) for k in range(9)]
    views = random_views(rng, 9, 33, 17, 1.3, 4 * voxel, True, True)
    views = [ts.view_of(cam, v.depth, v.weight, v.rgb) for cam, v in zip(cams, views)]
    vol = TsdfVolume(lo, hi, voxel, colour=True, max_weight=5.0, device=gpu)
    assert vol.dims == dims and vol.trunc == float(F(4) * F(voxel))
    t = lambda a: None if a is None else torch.from_numpy(a)
    vol.integrate([t(v.depth) for v in views], cams, weights=[t(v.weight) for v in views], images=[t(v.rgb) for v in views])
    spec = ts.new_volume(lo, voxel, dims, colour=True, max_weight=5.0)
    ts.integrate(spec, views)
    got = vol.numpy()
    for name in ("tsdf", "weight", "colour"):
        assert np.array_equal(bits(got[name]), bits(getattr(spec, name))), name
    assert float(spec.weight.max()) > 1.0


# ---- extraction -------------------------------------------------------------------------------------------------------------------
def extract_on_device(vol: ts.Volume, dev, min_weight=1.0, colours=True):
    """Plan + apply through the C ABI on guarded arrays, tmp filled with garbage -> (totals, arrays, output guards)."""
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    dv = DeviceVolume(vol, dev)
    nx, ny, nz = vol.dims
    tmp = wg.guarded(lib.hgs_tsdf_extract_tmp_bytes(nx, ny, nz), dev, 0xFF, "tmp")
    tmp.body.copy_(torch.randint(0, 256, (tmp.nbytes,), dtype=torch.uint8, device=dev))
    totals = (C.c_int64 * 2)()
    s = dv.struct()
    _lib.check(lib.hgs_tsdf_extract_plan(C.byref(s), float(min_weight), tmp.addr, totals, stream, 0), "hgs_tsdf_extract_plan")
    V, Q = int(totals[0]), int(totals[1])
    colours = colours and vol.colour is not None
    out = dict(vertices=wg.guarded(12 * V, dev, 0xFF, "vertices"), normals=wg.guarded(12 * V, dev, 0xFF, "normals"),
               faces=wg.guarded(24 * Q, dev, 0xFF, "faces"))
    if colours:
        out["colours"] = wg.guarded(12 * V, dev, 0xFF, "colours")
    _lib.check(lib.hgs_tsdf_extract_apply(C.byref(s), tmp.addr, out["vertices"].addr, out["normals"].addr,
                                          out["colours"].addr if colours else None, out["faces"].addr, stream, 0),
               "hgs_tsdf_extract_apply")
    wg.check(tmp, *out.values())
    dv.check()
    arrays = {k: g.body.cpu().numpy().view(np.int32 if k == "faces" else F).reshape(-1, 3) for k, g in out.items()}
    return (V, Q), arrays, out


def noise_volume(rng, dims, colour=True):
    """Smoothed noise: many active cells and quads of every orientation, unobserved samples, exact zeros."""
    nx, ny, nz = dims
    vol = ts.new_volume((0.3, -1.1, 2.0), 0.07, dims, colour=colour)
    t = rng.normal(size=(nz, ny, nx))
    for axis in range(3):
        if t.shape[axis] > 2:
            t = t + np.roll(t, 1, axis) + np.roll(t, -1, axis)
    vol.tsdf[:] = np.clip(t / 3.0, -1, 1).astype(F)
    vol.tsdf[rng.random(t.shape) < 0.02] = 0.0
    vol.weight[:] = (4 * rng.random(t.shape)).astype(F)
    vol.weight[rng.random(t.shape) < 0.7] += 1.0
    if colour:
        vol.colour[:] = rng.random(vol.colour.shape).astype(F)
    return vol


def compare_mesh(totals, arrays, spec: ts.SpecMesh):
    V, Q = totals
    assert (V, Q) == (spec.vertices.shape[0], spec.faces.shape[0] // 2)
    assert np.array_equal(bits(arrays["vertices"]), bits(spec.vertices))
    assert np.array_equal(bits(arrays["normals"]), bits(spec.normals))
    if "colours" in arrays:
        assert np.array_equal(bits(arrays["colours"]), bits(spec.colours))
    assert np.array_equal(arrays["faces"], spec.faces)


@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 3, 2), (37, 21, 13), (64, 64, 8), (65, 7, 9)], ids=lambda d: "x".join(map(str, d)))
def test_extraction_equals_the_spec_bit_for_bit(gpu, dims):
    rng = np.random.default_rng(sum(dims))
    vol = noise_volume(rng, dims)
    if dims == (2, 2, 2):
        vol.weight[:] = 2.0
        vol.tsdf[0] = -0.5
        vol.tsdf[1] = 0.25
    spec = ts.extract(vol, 1.0)
    totals, arrays, _ = extract_on_device(vol, gpu)
    print(f"{dims}: {totals[0]} vertices, {totals[1]} quads")
    assert totals[0] > 0 and (totals[1] > 0 or min(dims) < 3)
    compare_mesh(totals, arrays, spec)
    again = extract_on_device(vol, gpu)              # other garbage in tmp: identical bytes
    assert again[0] == totals and all(np.array_equal(again[1][k].view(np.uint32), arrays[k].view(np.uint32)) for k in arrays)
    no_colour = extract_on_device(vol, gpu, colours=False)
    assert "colours" not in no_colour[1] and np.array_equal(no_colour[1]["faces"], arrays["faces"])


def test_extraction_of_a_fused_sphere(gpu):
    """The spec's volume of tests/test_tsdf_cpu.py's sphere, at another min_weight as well."""
    vol, views, _ = sphere_scene(colour=True)
    ts.integrate(vol, views)
    for min_weight in (1.0, 3.0):
        spec = ts.extract(vol, min_weight)
        totals, arrays, _ = extract_on_device(vol, gpu, min_weight)
        compare_mesh(totals, arrays, spec)
        assert totals[0] > 50
    err = np.abs(np.linalg.norm(arrays["vertices"].astype(np.float64) - np.array(SPHERE_C), axis=1) - SPHERE_R)
    assert err.max() <= math.sqrt(3.0) * float(vol.voxel) + ts.e_pix([v.depth for v in views])


def test_extraction_where_the_scan_takes_a_second_chunk(gpu):
    """More than 8192 workgroups of 256 samples: both scans chain over two chunks.  An analytic sphere, written straight
    into the volume."""
    dims = (130, 128, 130)
    vol = ts.new_volume((-1.0, -1.0, -1.0), 2.0 / 129, dims, colour=False)
    assert (vol.tsdf.size + 255) // 256 > 8192
    nx, ny, nz = dims
    x, y, z = (ts.lattice(vol.lo[a], vol.voxel, n) for a, n in zip(range(3), dims))
    r = np.sqrt(x[None, None, :] ** 2 + y[None, :, None] ** 2 + z[:, None, None] ** 2)
    vol.tsdf[:] = np.clip((r - F(0.8)) / vol.trunc, -1, 1).astype(F)
    vol.weight[:] = 2.0
    vol.weight[:, :, :40] = 0.5                       # a part nobody has seen
    spec = ts.extract(vol, 1.0)
    totals, arrays, _ = extract_on_device(vol, gpu)
    print(f"{dims}: {totals[0]} vertices, {totals[1]} quads")
    compare_mesh(totals, arrays, spec)
    assert totals[0] > 10000


def test_a_volume_without_a_sign_change_extracts_nothing(gpu):
    for dims in ((1, 1, 1), (5, 3, 2), (37, 21, 13)):
        vol = ts.new_volume((0, 0, 0), 0.1, dims, colour=True)
        vol.weight[:] = 2.0
        totals, arrays, guards = extract_on_device(vol, gpu)
        assert totals == (0, 0) and all(a.shape == (0, 3) for a in arrays.values())
    # unobserved samples on either side of the only sign change
    vol = ts.new_volume((0, 0, 0), 0.1, (6, 5, 4))
    vol.weight[:] = 2.0
    vol.tsdf[:, :, :3] = -1.0
    vol.weight[:, :, 2:4] = 0.5
    assert extract_on_device(vol, gpu)[0] == (0, 0)
    # room for outputs that must stay untouched
    lib = _lib.lib()
    dv = DeviceVolume(vol, gpu)
    tmp = wg.guarded(lib.hgs_tsdf_extract_tmp_bytes(6, 5, 4), gpu, 0xFF, "tmp")
    totals = (C.c_int64 * 2)(7, 7)
    s = dv.struct()
    _lib.check(lib.hgs_tsdf_extract_plan(C.byref(s), 1.0, tmp.addr, totals, None, 0), "plan")
    assert list(totals) == [0, 0]
    outs = [wg.guarded(4096, gpu, 0xFF, n) for n in ("vertices", "normals", "faces")]
    _lib.check(lib.hgs_tsdf_extract_apply(C.byref(s), tmp.addr, outs[0].addr, outs[1].addr, None, outs[2].addr, None, 0), "apply")
    wg.check(*outs)
    assert all(bool((g.body == 0xFF).all()) for g in outs)
    # apply on another workspace, or for other dimensions, has no plan to follow
    other = wg.guarded(tmp.nbytes, gpu, 0xFF, "other")
    assert lib.hgs_tsdf_extract_apply(C.byref(s), other.addr, outs[0].addr, outs[1].addr, None, outs[2].addr, None, 0) == 1
    assert b"hgs_tsdf_extract_plan" in lib.hgs_last_error()
    s.nx = 5
    assert lib.hgs_tsdf_extract_apply(C.byref(s), tmp.addr, outs[0].addr, outs[1].addr, None, outs[2].addr, None, 0) == 1


# ---- end to end -------------------------------------------------------------------------------------------------------------------
ROI_LO, ROI_HI, VOXEL = (-2.0, -1.5, 2.0), (2.0, 1.5, 8.0), 0.125


def e2e_cameras():
    return [synth.orbit_camera(96, 64, k, 6) for k in range(6)]


@pytest.fixture(scope="module")
def hier(gpu):
    return cc.on_device(cc.hier2000(), gpu)


def test_fuse_hierarchy_equals_the_hand_composition_and_gives_a_mesh_inside_the_roi(gpu, hier):
    from hgs.importance import render_hierarchy
    from hgs.meshing import TsdfVolume, fuse_hierarchy, surface_depth
    from hgs.picking import read_hierarchy_view
    cams = e2e_cameras()
    vol = TsdfVolume(ROI_LO, ROI_HI, VOXEL, colour=True, device=gpu)
    assert fuse_hierarchy(hier, cams, vol) is vol
    hand = TsdfVolume(ROI_LO, ROI_HI, VOXEL, colour=True, device=gpu)
    depths, images = [], []
    for cam in cams:
        r = read_hierarchy_view(hier, cam, want=("alpha", "median_depth"))
        d = r.median_depth.clone()
        d[r.alpha < 0.5] = 0.0
        assert torch.equal(d, surface_depth(r, 0.5))
        depths.append(d)
        images.append(render_hierarchy(hier, cam))
    hand.integrate(depths, cams, images=images)
    a, b = vol.numpy(), hand.numpy()
    for name in ("tsdf", "weight", "colour"):
        assert np.array_equal(bits(a[name]), bits(b[name])), name
    # ... and both equal the spec on the same maps
    spec = ts.new_volume(ROI_LO, VOXEL, vol.dims, colour=True)
    views = [ts.view_of(cam, d.cpu().numpy(), rgb=i.cpu().numpy()) for cam, d, i in zip(cams, depths, images)]
    ts.integrate(spec, views)
    for name in ("tsdf", "weight", "colour"):
        assert np.array_equal(bits(a[name]), bits(getattr(spec, name))), name
    mesh = vol.extract()
    m = mesh.numpy()
    want = ts.extract(spec, 1.0)
    compare_mesh((m["vertices"].shape[0], m["faces"].shape[0] // 2), m, want)
    V = m["vertices"].shape[0]
    print(f"end to end: volume {vol.dims}, {int((a['weight'] >= 1).sum())} samples observed, {V} vertices, {m['faces'].shape[0]} faces")
    assert V > 0
    assert (m["vertices"] >= np.array(ROI_LO, F)).all() and (m["vertices"] <= np.array(ROI_HI, F)).all()
    assert m["faces"].min(initial=0) >= 0 and m["faces"].max(initial=0) < V
    # every active cell has a sample that some view places behind its surface, inside the band
    nx, ny, nz = vol.dims
    x = (ts.lattice(spec.lo[0], spec.voxel, nx)[None, None, :], ts.lattice(spec.lo[1], spec.voxel, ny)[None, :, None],
         ts.lattice(spec.lo[2], spec.voxel, nz)[:, None, None])
    behind = np.zeros((nz, ny, nx), bool)
    for v in views:
        ok, z, px, py = ts.project(*x, v)
        d = v.depth[py, px]
        sdf = d - z
        behind |= ok & (d > 0) & (sdf >= -spec.trunc) & (sdf < 0)
    assert ts.corners(behind).any(-1)[want.active].all()
    # without colour: the same geometry
    plain = TsdfVolume(ROI_LO, ROI_HI, VOXEL, colour=False, device=gpu)
    fuse_hierarchy(hier, cams, plain)
    pm = plain.extract()
    assert pm.colours is None and torch.equal(pm.vertices, mesh.vertices) and torch.equal(pm.faces, mesh.faces)


def test_the_command_writes_a_ply_with_the_printed_counts(gpu, hier, tmp_path, capsys):
    from gaussian_hierarchy._C import write_hierarchy
    from hgs import mesh_hierarchy as mh
    from hgs.meshing import TsdfVolume, fuse_hierarchy
    from hgs.score_hierarchy import read_cameras
    host = cc.hier2000()
    path, cams = tmp_path / "in.hier", tmp_path / "cameras.json"
    write_hierarchy(str(path), *[getattr(host, k) for k in cc.FIELDS])
    cams.write_text(json.dumps([cc.camera_entry(c) for c in e2e_cameras()]))
    out, vout = tmp_path / "o" / "mesh.ply", tmp_path / "o" / "v.npz"
    rc = mh.main([str(path), str(out), "--cameras", str(cams), "--voxel", str(VOXEL), "--volume-out", str(vout), "--roi"]
                 + [str(v) for v in ROI_LO + ROI_HI])
    text = capsys.readouterr().out
    assert rc == 0 and text.startswith("mesh_hierarchy: N = 3999 nodes, 6 views at 0 px; volume 33 x 25 x 49 = 40425 samples")
    ply = read_ply(out)
    V, Fc = ply["vertices"].shape[0], ply["faces"].shape[0]
    assert V > 0 and f"{V} vertices, {Fc} faces" in text and ply["colours"] is not None
    vol = TsdfVolume(ROI_LO, ROI_HI, VOXEL, colour=True, device=gpu)
    mesh = fuse_hierarchy(hier, read_cameras(str(cams)), vol).extract().numpy()
    assert np.array_equal(bits(ply["vertices"]), bits(mesh["vertices"])) and np.array_equal(ply["faces"], mesh["faces"])
    z = np.load(vout)
    assert np.array_equal(bits(z["tsdf"]), bits(vol.numpy()["tsdf"])) and z["tsdf"].shape == (49, 25, 33)
    # the root's box as the region, no colour, a coarser cut
    rc = mh.main([str(path), str(out), "--cameras", str(cams), "--voxel", "0.5", "--roi-root", "--no-colour", "--tau-px", "2"])
    text = capsys.readouterr().out
    ply = read_ply(out)
    assert rc == 0 and ply["colours"] is None and f"{ply['vertices'].shape[0]} vertices, {ply['faces'].shape[0]} faces, no colour" in text
