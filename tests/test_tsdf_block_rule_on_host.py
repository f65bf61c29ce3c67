"""The PRODUCT's sparse-volume allocation rule (csrc/tsdf_block_rule.h: the depth steps, the sub-pixel grid, the
unprojection, the block of a point -- what tsdf_sparse_mark_kernel runs) compiled for the HOST with g++ and
-ffp-contract=off, as a program of its own, and held against the numpy spec tests/tsdf_sparse_spec.py BIT FOR BIT: the
same marks and, as a multiset, the same block for every marched point -- no GPU.  The headers are copied unchanged at test
time and compiled against tests/harness/host_math/common.h, as tests/test_tsdf_rule_on_host.py does."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tsdf_sparse_spec as sp
import tsdf_spec as ts
from hgs.synth import make_camera, orbit_camera

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "host_math")
CSRC = os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc")
F = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsdf_block_rule")
    for f in (os.path.join(HARNESS, "common.h"), os.path.join(HARNESS, "tsdf_block_host.cpp"),
              os.path.join(CSRC, "tsdf_rule.h"), os.path.join(CSRC, "tsdf_block_rule.h")):
        shutil.copy(f, d)
    exe = os.path.join(d, "tsdf_block_host")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                        "-I", os.path.join(ROOT, "include"), "-I", str(d), os.path.join(d, "tsdf_block_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, d


def run_host(program, view: ts.View, lo, voxel, trunc, dims):
    exe, d = program
    head = np.array([view.W, view.H, *dims, int(view.weight is not None)], np.int32)
    par = np.concatenate([view.view, [view.tanfovx, view.tanfovy, view.z_min], np.asarray(lo, F), [voxel, trunc]]).astype(F)
    assert par.size == 20
    src, dst = os.path.join(d, "job.bin"), os.path.join(d, "out.bin")
    with open(src, "wb") as f:
        f.write(head.tobytes() + par.tobytes() + np.ascontiguousarray(view.depth, F).tobytes())
        if view.weight is not None:
            f.write(np.ascontiguousarray(view.weight, F).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(dst, "rb").read()
    S, refused, gx, gy, gz = np.frombuffer(raw, np.int32, 5)
    marks = np.frombuffer(raw, np.uint8, gx * gy * gz, 20).reshape(gz, gy, gx) != 0
    n = int(np.frombuffer(raw, np.int32, 1, 20 + gx * gy * gz)[0])
    points = np.frombuffer(raw, np.int32, 5 * n, 24 + gx * gy * gz).reshape(n, 5)
    return int(S), bool(refused), marks, points


def spec_marking(view, lo, voxel, trunc, dims):
    sv = sp.new_sparse(lo, voxel, dims, trunc=trunc)
    rows = []
    for inside, block, px, py, _ in sp.marched_points(sv, view):
        b = block[inside]
        sv.marks[b[:, 2], b[:, 1], b[:, 0]] = True
        rows.append(np.concatenate([px[inside, None], py[inside, None], b], -1))
    rows = np.concatenate(rows) if rows else np.zeros((0, 5), np.int64)
    return sp.steps(trunc, voxel), sv.refused, sv.marks, rows.astype(np.int32)


def sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def noisy_view(rng, k, W, H, centre, spread, weight, z_min):
    cam = orbit_camera(W, H, k, 5, radius=0.4, tilt=0.2) if k else make_camera(W, H)
    depth = (centre + spread * (2 * rng.random((H, W)) - 1)).astype(F)
    if W * H > 4:
        depth[rng.random((H, W)) < 0.1] = 0.0
        depth[rng.random((H, W)) < 0.05] = np.nan
        depth[rng.random((H, W)) < 0.03] = -1.0
        depth[rng.random((H, W)) < 0.02] = np.inf
    w = None
    if weight:
        w = rng.random((H, W)).astype(F)
        w[rng.random((H, W)) < 0.15] = 0.0
    return ts.view_of(cam, depth, w, z_min=z_min)


#         image      dims             voxel   trunc (voxels) centre spread weight z_min
CASES = [((1, 1), (1, 1, 1), 0.1, 4.0, 0.2, 0.0, False, 0.01),
         ((7, 5), (8, 8, 8), 0.1, 4.0, 0.6, 0.3, True, 0.05),
         ((33, 17), (65, 7, 9), 0.03, 2.5, 0.4, 0.3, False, 0.3),         # z_min cuts into the bands
         ((80, 60), (37, 21, 13), 0.043, 3.7, 0.7, 0.5, True, 0.05),
         ((4, 3), (170, 130, 90), 0.012, 4.0, 0.6, 0.3, False, 0.05),      # fine voxels under large pixels: M > 1
         ((64, 48), (4096, 4096, 512), 0.01, 4.0, 2.0, 1.0, True, 0.05)]   # a virtual lattice


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])) + "_" + "x".join(map(str, c[1])))
def test_the_marking_equals_the_spec_bit_for_bit(program, case):
    (W, H), dims, voxel, trunc_v, centre, spread, weight, z_min = case
    rng = np.random.default_rng(W * 1000 + dims[0])
    voxel = F(voxel)
    trunc = F(trunc_v) * voxel
    lo = np.array([F(-0.5) * voxel * F(min(dims[0], 200)), F(-0.5) * voxel * F(min(dims[1], 200)), F(0.1)], F)
    seen_m, total = set(), 0
    for k in range(3):
        view = noisy_view(rng, k, W, H, centre, spread, weight, z_min)
        got = run_host(program, view, lo, voxel, trunc, dims)
        want = spec_marking(view, lo, voxel, trunc, dims)
        assert got[0] == want[0] and got[1] == want[1] and not got[1]
        assert np.array_equal(got[2], want[2])
        assert np.array_equal(sorted_rows(got[3]), sorted_rows(want[3]))
        _, M, _ = sp.pixel_sub(view, trunc, voxel)
        seen_m |= set(np.unique(M).tolist())
        total += got[3].shape[0]
        # every marked block holds a marched point and the other way round
        b = np.unique(got[3][:, 2:], axis=0)
        assert int(got[2].sum()) == b.shape[0]
    print(f"{dims}: S = {got[0]}, M in {sorted(seen_m)}, {total} marched points that mark a block, {int(got[2].sum())} blocks marked by the last view")
    if (W, H) == (4, 3):
        assert max(seen_m) > 1


def test_the_steps_and_the_refusals(program):
    """S at and around whole numbers of voxels; a pixel whose footprint asks for more than 16 sub-positions sets the
    refusal word and marks nothing."""
    for trunc, voxel in ((0.4, 0.1), (0.25, 0.1), (0.05, 0.1), (1.0, 1.0), (0.3, 0.1), (409.6, 0.1), (409.7, 0.1)):
        S = sp.steps(F(trunc), F(voxel))
        assert S >= 1 and (S > sp.MAX_STEPS or F(2) * F(trunc) / F(S) <= F(2) * F(voxel))
        assert S == 1 or S > sp.MAX_STEPS or F(2) * F(trunc) / F(S - 1) > F(2) * F(voxel)
    cam = make_camera(8, 8)
    depth = np.ones((8, 8), F)
    depth[7, 7] = 50.0
    view = ts.view_of(cam, depth, z_min=0.05)
    voxel, lo = F(0.01), np.zeros(3, F)
    got = run_host(program, view, lo, voxel, F(0.04), (64, 64, 200))
    want = spec_marking(view, lo, voxel, F(0.04), (64, 64, 200))
    assert got[1] and want[1]
    assert np.array_equal(got[2], want[2]) and np.array_equal(sorted_rows(got[3]), sorted_rows(want[3]))
    assert got[3].shape[0] > 0 and not ((got[3][:, 0] == 7) & (got[3][:, 1] == 7)).any()     # pixel (7, 7) marched nothing
