"""The PRODUCT's TSDF rules (csrc/tsdf_rule.h: the lattice, the projection, the update, the cell vertex, normal and
colour, the quad winding -- what the kernels of csrc/tsdf.hip run) compiled for the HOST with g++ and -ffp-contract=off
and held against the numpy spec tests/tsdf_spec.py BIT FOR BIT -- no GPU.  The header is copied unchanged at test time
and compiled against tests/harness/host_math/common.h, as tests/test_hier_refit_rule_on_host.py does.  Every operation
of the rule (+ - x / sqrt floor) is correctly rounded on both sides and the order is written out, so the bound is zero."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import tsdf_spec as ts
from hgs.synth import make_camera, orbit_camera

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "host_math")
F = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsdf_rule")
    for f in (os.path.join(HARNESS, "common.h"), os.path.join(HARNESS, "tsdf_host.cpp"),
              os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc", "tsdf_rule.h")):
        shutil.copy(f, d)
    so = os.path.join(d, "libtsdfrule.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "include"), "-I", str(d), os.path.join(d, "tsdf_host.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(so)


p = lambda a: a.ctypes.data_as(C.c_void_p)
bits = lambda a: np.ascontiguousarray(a, dtype=F).view(np.uint32)


def host_samples(host, ijk, lo, voxel, view, d, w, rgb, tsdf, weight, colour, trunc, max_weight, use_colour, use_rgb):
    n = ijk.shape[0]
    words = np.concatenate([view.view, [view.tanfovx, view.tanfovy, view.z_min, F(view.W), F(view.H)]]).astype(F)
    views = np.ascontiguousarray(np.tile(words, (n, 1)))
    seen, applied = np.zeros(n, np.int32), np.zeros(n, np.int32)
    z, pix = np.zeros(n, F), np.zeros((n, 2), np.int32)
    tsdf, weight, colour = tsdf.copy(), weight.copy(), colour.copy()
    lo = np.ascontiguousarray(lo, F)
    host.host_tsdf_samples(p(ijk), C.c_int64(n), p(lo), C.c_float(voxel), p(views), p(d), p(w), p(rgb),
                           int(use_colour), int(use_rgb), C.c_float(trunc), C.c_float(max_weight), p(seen), p(z), p(pix),
                           p(tsdf), p(weight), p(colour), p(applied))
    return seen != 0, z, pix, tsdf, weight, colour, applied != 0


def random_view(rng, k, W, H):
    cam = orbit_camera(W, H, k, 5, radius=0.4, tilt=0.2) if k else make_camera(W, H)
    depth = (1.5 + rng.random((H, W))).astype(F)
    depth[rng.random((H, W)) < 0.1] = 0.0               # holes
    depth[rng.random((H, W)) < 0.05] = np.nan
    depth[rng.random((H, W)) < 0.03] = -1.0
    weight = rng.random((H, W)).astype(F)
    weight[rng.random((H, W)) < 0.1] = 0.0
    rgb = rng.random((3, H, W)).astype(F)
    return ts.view_of(cam, depth, weight, rgb, z_min=0.2)


@pytest.mark.parametrize("use_weight, use_colour, use_rgb", [(True, True, True), (False, False, False), (False, True, False)])
def test_the_integrate_step_against_the_spec(host, use_weight, use_colour, use_rgb):
    rng = np.random.default_rng(11)
    lo, voxel, trunc, max_weight = np.array([-1.5, -1.1, -0.6], F), F(0.043), F(0.15), F(1.7)
    branches = np.zeros(7, np.int64)
    for k, (W, H) in enumerate(((1, 1), (7, 5), (33, 17), (80, 60), (64, 48))):
        view = random_view(rng, k, W, H)
        n = 6000
        ijk = np.ascontiguousarray(rng.integers(0, 70, size=(n, 3)).astype(np.int32))       # z from -0.6 to 2.4
        tsdf = (rng.random(n) * 2 - 1).astype(F)
        weight = (rng.random(n) * 1.5).astype(F)
        colour = rng.random((n, 3)).astype(F)
        x = [ts.lattice(lo[a], voxel, 70)[ijk[:, a]] for a in range(3)]
        ok, z, px, py = ts.project(x[0], x[1], x[2], view)
        d = np.ascontiguousarray(view.depth[py, px])
        # some depths exactly at the truncation edge and just beyond it, whatever the map holds
        edge = ok & (rng.random(n) < 0.1)
        d[edge] = (z - trunc)[edge]
        d[edge & (np.arange(n) % 2 == 0)] = np.nextafter((z - trunc)[edge & (np.arange(n) % 2 == 0)], F(-np.inf))
        w = np.ascontiguousarray(view.weight[py, px]) if use_weight else np.ones(n, F)
        rgb = np.ascontiguousarray(np.moveaxis(view.rgb[:, py, px], 0, -1))
        want_t, want_w, want_c, applied = ts.update(tsdf, weight, colour if use_colour else None, ok, z, d, w,
                                                    rgb if use_rgb else None, trunc, max_weight)
        got = host_samples(host, ijk, lo, voxel, view, d, w, rgb, tsdf, weight, colour, trunc, max_weight, use_colour,
                           use_rgb)
        assert np.array_equal(got[0], ok)
        assert np.array_equal(bits(got[1])[ok], bits(z)[ok])
        assert np.array_equal(got[2][ok], np.stack([px, py], -1)[ok])
        assert np.array_equal(got[6], applied)
        assert np.array_equal(bits(got[3]), bits(want_t)) and np.array_equal(bits(got[4]), bits(want_w))
        assert np.array_equal(bits(got[5]), bits(want_c if use_colour and use_rgb else colour))
        with np.errstate(invalid="ignore"):
            sdf = d - z
            branches += [int((~ok).sum()), int((ok & ~(d > 0)).sum()), int((ok & (d > 0) & ~(w > 0)).sum()),
                         int((ok & (d > 0) & (sdf < -trunc)).sum()), int((applied & (sdf == -trunc)).sum()),
                         int((applied & (sdf > trunc)).sum()), int((applied & (weight + w > max_weight)).sum())]
    print("not seen, no depth, no weight, behind the band, on its edge, clipped to 1, max_weight binds:", branches.tolist())
    assert (branches[[0, 1, 3, 4, 5, 6]] > 0).all() and (branches[2] > 0) == use_weight


def test_each_projection_refusal(host):
    """Behind the camera, at z_min exactly, off each image border, and NaN coordinates."""
    cam = make_camera(8, 6)
    view = ts.view_of(cam, np.full((6, 8), 2.0, F), z_min=0.5)
    lo, voxel = np.zeros(3, F), F(0.5)
    ijk = np.array([[0, 0, 4], [0, 0, 1], [0, 0, 0], [0, 0, 2], [40, 0, 4], [0, 40, 4], [3, 2, 4]], np.int32)
    n = ijk.shape[0]
    x = [ts.lattice(lo[a], voxel, 64)[ijk[:, a]] for a in range(3)]
    ok, z, px, py = ts.project(x[0], x[1], x[2], view)
    assert ok.tolist() == [True, False, False, True, False, False, True]      # z = 0.5 is not > z_min
    one, zero3 = np.ones(n, F), np.zeros((n, 3), F)
    got = host_samples(host, ijk, lo, voxel, view, 2 * one, one, zero3, one, 0 * one, zero3, F(1), F(np.inf), False, False)
    assert np.array_equal(got[0], ok) and np.array_equal(got[2][ok], np.stack([px, py], -1)[ok])
    nan_lo = np.array([np.nan, 0, 0], F)
    got = host_samples(host, ijk, nan_lo, voxel, view, 2 * one, one, zero3, one, 0 * one, zero3, F(1), F(np.inf), False, False)
    assert not got[0].any() and not got[6].any()


def random_blocks(rng, n):
    t = (rng.random((n, 8)) * 2 - 1).astype(F)
    t[: n // 8] = np.abs(t[: n // 8])                    # no sign change
    t[n // 8: n // 4, :] *= (rng.random((n // 4 - n // 8, 8)) < 0.5)     # exact zeros (outside: not < 0)
    checker = np.array([1 - 2 * ((s ^ (s >> 1) ^ (s >> 2)) & 1) for s in range(8)], F)
    t[n // 4: n // 4 + 50] = checker * F(0.25)           # a checkerboard: the gradient cancels on every axis
    w = (rng.random((n, 8)) * 4).astype(F)
    w[n // 2:] += 1.0
    w[n // 4: n // 4 + 50] = 2.0
    return t, w


def test_the_cell_rules_against_the_spec(host):
    rng = np.random.default_rng(12)
    n = 20000
    t, w = random_blocks(rng, n)
    c = rng.random((n, 3, 8)).astype(F)
    ijk = rng.integers(0, 500, size=(n, 3)).astype(np.int32)
    lo, voxel, min_weight = np.array([-3.1, 0.7, 11.3], F), F(0.037), F(1.0)
    active, local, normal, colour, world = (np.zeros(n, np.int32), np.zeros((n, 3), F), np.zeros((n, 3), F),
                                            np.zeros((n, 3), F), np.zeros((n, 3), F))
    host.host_tsdf_cells(p(t), p(w), p(c), p(ijk), C.c_int64(n), p(lo), C.c_float(voxel), C.c_float(min_weight),
                         p(active), p(local), p(normal), p(colour), p(world))
    ins = t < 0
    want_active = (w >= min_weight).all(-1) & ins.any(-1) & ~ins.all(-1)
    assert np.array_equal(active != 0, want_active) and 1000 < want_active.sum() < n - 1000
    a = want_active
    want_local, want_normal = ts.cell_vertex(t[a])
    assert np.array_equal(bits(local[a]), bits(want_local))
    assert np.array_equal(bits(normal[a]), bits(want_normal))
    assert np.array_equal(bits(colour[a]), bits(ts.cell_colour(c[a])))
    assert np.array_equal(bits(world[a]), bits(lo[None] + voxel * (ijk[a].astype(F) + want_local)))
    # the vertex lies in its cell, the normal is unit or zero, and zero only for a zero gradient
    assert (want_local >= 0).all() and (want_local <= 1).all()
    length = np.linalg.norm(want_normal.astype(np.float64), axis=-1)
    assert ((np.abs(length - 1) < 1e-6) | (length == 0)).all() and (length == 0).any()


def test_the_quad_winding(host):
    """For each axis and each side: the cells are those of the spec, and on a lattice of vertices at the cell centres the
    face normal of both triangles points from the inside sample to the outside one."""
    for axis in range(3):
        for lower_inside in (0, 1):
            v = np.array([10, 11, 12, 13], np.int32)
            cells, faces = np.zeros((4, 3), np.int32), np.zeros((2, 3), np.int32)
            host.host_tsdf_quad(axis, p(v), lower_inside, p(cells), p(faces))
            assert cells.tolist() == ts.quad_cells(axis)
            assert np.array_equal(faces, ts.quad_faces(v, np.bool_(lower_inside)))
            centre = {10 + q: cells[q] + 0.5 for q in range(4)}
            for tri in faces:
                assert len(set(tri.tolist())) == 3
                a, b, c = (centre[int(q)] for q in tri)
                nrm = np.cross(b - a, c - a)
                e = np.zeros(3)
                e[axis] = 1.0 if lower_inside else -1.0
                assert nrm @ e > 0 and np.allclose(np.cross(nrm, e), 0)
