"""The PRODUCT's box rules (csrc/hier_refit_rule.h: the two leaf rules, the union, the extent and the leaf test that
hr_plan_kernel, hr_leaf_kernel and hr_level_kernel run) compiled for the HOST and held against the numpy spec
hgs.hierarchy.leaf_boxes -- no GPU.  The header is copied unchanged at test time and compiled with g++ against
tests/harness/host_math/common.h, as tests/test_hier_nodes_on_host.py does with hier_nodes.h.  Bound: one float32 ulp
per leaf coordinate -- the one operation libm and numpy may round differently is the double exp; every other one
(+ - x / sqrt) is correctly rounded on both sides, and the sums run in the same order."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from hgs import hierarchy
from test_hier_refit_cpu import built, merged

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "host_math")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("hier_refit_rule")
    for f in (os.path.join(HARNESS, "common.h"), os.path.join(HARNESS, "hier_refit_host.cpp"),
              os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc", "hier_refit_rule.h")):
        shutil.copy(f, d)
    so = os.path.join(d, "libhierrefit.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "include"), "-I", str(d), os.path.join(d, "hier_refit_host.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(so)


def leaves(host, xyz, ls, q, mode):
    n = xyz.shape[0]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    xyz, ls, q = (np.ascontiguousarray(a, dtype=np.float32) for a in (xyz, ls, q))
    lo, hi, ext, ok = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    host.host_refit_leaves(p(xyz), p(ls), p(q), C.c_int64(n), {"cube": 1, "ellipsoid": 2}[mode], p(lo), p(hi), p(ext), p(ok))
    return lo, hi, ext, ok


def ulps(a, b):
    o = lambda x: (lambda i: np.where(i < 0, -(i & 0x7FFFFFFF), i))(x.view(np.int32).astype(np.int64))
    return np.abs(o(np.ascontiguousarray(a)) - o(np.ascontiguousarray(b)))


@pytest.mark.parametrize("mode", ("cube", "ellipsoid"))
def test_the_leaf_rules_against_the_spec(host, mode):
    for h in (built(1000), built(2000), merged(3)):
        x, ls, q = h.xyz.numpy(), h.log_scales.numpy(), h.rots.numpy()
        lo, hi, ext, ok = leaves(host, x, ls, q, mode)
        wlo, whi = hierarchy.leaf_boxes(x, ls, q, mode)
        u = np.maximum(ulps(lo, wlo), ulps(hi, whi))
        print(f"{mode}, {x.shape[0]} rows: {int(u.max())} ulp at most, {float((u > 0).mean()):.2e} of the coordinates differ")
        assert int(u.max()) <= 1
        assert ok.all()
        e = hi - lo
        assert np.array_equal(ext.view(np.uint32), np.maximum(np.maximum(e[:, 0], e[:, 1]), e[:, 2]).view(np.uint32))


def test_rows_that_are_not_finite_fail_the_leaf_test(host):
    h = built(5)
    x, ls, q = (a.numpy().copy() for a in (h.xyz, h.log_scales, h.rots))
    x[0, 1] = np.nan
    ls[1, 2] = np.inf
    ls[2, 0] = np.nan                      # (not the largest scale: a maximum by comparisons alone would skip it)
    ls[2, 1:] = 5.0
    ls[3, 0] = 100.0                       # finite in double, not in float32
    q[4] = 0.0
    _, _, _, ok = leaves(host, x, ls, q, "cube")
    assert ok.tolist()[:5] == [0, 0, 0, 0, 1] and ok[5:].all()
    _, _, _, ok = leaves(host, x, ls, q, "ellipsoid")
    assert ok.tolist()[:5] == [0, 0, 0, 0, 0] and ok[5:].all()
    for mode in ("cube", "ellipsoid"):
        wlo, whi = hierarchy.leaf_boxes(x, ls, q, mode)
        spec_ok = np.isfinite(wlo).all(1) & np.isfinite(whi).all(1)
        assert np.array_equal(spec_ok, leaves(host, x, ls, q, mode)[3] != 0), mode


def test_the_union(host):
    rng = np.random.default_rng(5)
    lo = rng.normal(size=(70, 3)).astype(np.float32)
    hi = lo + rng.random((70, 3)).astype(np.float32)
    out_lo, out_hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for n in (1, 2, 70):
        host.host_refit_union(p(lo), p(hi), C.c_int64(n), p(out_lo), p(out_hi))
        assert np.array_equal(out_lo, lo[:n].min(0)) and np.array_equal(out_hi, hi[:n].max(0)), n
