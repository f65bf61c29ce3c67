"""The PRODUCT's merge rule (csrc/hier_merge_rule.h: a child's weight and covariance from its row, the k-child moment
match, the Jacobi eigen tail and its parametrisation -- what hb_merge_kernel and hp_remerge_kernel run) compiled for the
HOST and held against the float64 numpy spec hgs.hierarchy.merge_rows -- no GPU.  The header is copied unchanged at test
time and compiled with g++ against tests/harness/host_math/common.h, as tests/test_hier_refit_rule_on_host.py does with
hier_refit_rule.h.  Bounds: the builder's own contract (tests/test_hier_build_gpu.py) -- mean, SH and opacity within
parity.assert_stats at 1e-5, covariance within 1e-5 Frobenius per node, quaternions unit to 1e-6, eigenvalues
ascending; frames are not compared (the frame of a near-isotropic covariance is free)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import parity as pa
from hgs import hierarchy

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness")
W = 48


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    d = tmp_path_factory.mktemp("hier_merge_rule")
    for f in (os.path.join(HARNESS, "host_math", "common.h"), os.path.join(HARNESS, "hier_merge_rule_host.cpp"),
              os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc", "hier_merge_rule.h")):
        shutil.copy(f, d)
    flags = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
             "-I", str(d), os.path.join(d, "hier_merge_rule_host.cpp")]
    so, exe = os.path.join(d, "libhiermerge.so"), os.path.join(d, "hier_merge_rule_host")
    for extra in (["-shared", "-fPIC", "-o", so], ["-o", exe]):
        r = subprocess.run(flags + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(so), exe


def host_merge(lib, rows, counts, weights=None):
    xyz, shs, alpha, ls, q = (np.ascontiguousarray(a, dtype=np.float32) for a in rows)
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    n = counts.shape[0]
    out = dict(xyz=np.zeros((n, 3), np.float32), shs=np.zeros((n, W), np.float32), alpha=np.zeros(n, np.float32),
               log_scales=np.zeros((n, 3), np.float32), rots=np.zeros((n, 4), np.float32), cov=np.zeros((n, 6)))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    wts = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    lib.host_merge_rows(p(xyz), p(shs), p(alpha), p(ls), p(q), None if wts is None else p(wts), p(counts), C.c_int64(n), C.c_int64(W), p(out["xyz"]),
                        p(out["shs"]), p(out["alpha"]), p(out["log_scales"]), p(out["rots"]), p(out["cov"]))
    c = out["cov"]
    out["cov"] = np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], 1)
    return out


def children(n, k, seed):
    """n nodes of k children each: float32 rows (xyz, shs, alpha, log_scales, rots), rots of any norm near 1."""
    g = np.random.default_rng(seed)
    m = n * k
    q = g.normal(size=(m, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * (1 + 1e-3 * g.normal(size=(m, 1)))
    return [a.astype(np.float32) for a in (3 * g.normal(size=(m, 3)), g.normal(size=(m, W)), g.random(m),
                                           0.6 * g.normal(size=(m, 3)) - 1.5, q)]


def cov_of_row(log_scales, rots):
    q = rots.astype(np.float64)
    R = hierarchy._rot_from_quat(q / np.linalg.norm(q, axis=1, keepdims=True))
    s2 = np.exp(2.0 * log_scales.astype(np.float64))
    return (R * s2[:, None, :]) @ R.transpose(0, 2, 1)


def assert_builders_bounds(name, got, want):
    """got: float32 rows of the product; want: hierarchy.merge_rows' float64 dict."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    stats = {k: pa.err_stats(t(got[k]), t(want[k])) for k in ("xyz", "shs", "alpha")}
    print(name, {k: (v["maxrel"], v["l2"]) for k, v in stats.items()})
    pa.assert_stats(name, stats, rel_tol=1e-5)
    norms = np.linalg.norm(got["rots"].astype(np.float64), axis=1)
    assert float(np.abs(norms - 1).max()) <= 1e-6, name
    ls = got["log_scales"]
    assert (ls[:, 0] <= ls[:, 1]).all() and (ls[:, 1] <= ls[:, 2]).all(), name
    # the covariance the written row stands for against the spec's moment match (floored where the spec's eigenvalues
    # are: a rank-deficient covariance comes back with 1e-12 on its null directions)
    ev, vec = np.linalg.eigh(want["cov"])
    floored = (vec * np.maximum(ev, 1e-12)[:, None, :]) @ vec.transpose(0, 2, 1)
    rel = np.linalg.norm(cov_of_row(ls, got["rots"]) - floored, axis=(1, 2)) / np.linalg.norm(floored, axis=(1, 2))
    print(name, "covariance", float(rel.max()))
    assert float(rel.max()) <= 1e-5, (name, float(rel.max()), int(rel.argmax()))


@pytest.mark.parametrize("k", (1, 2, 3, 7))
def test_k_children_against_the_spec(build, k):
    rows = children(300, k, seed=k)
    counts = np.full(300, k)
    want = hierarchy.merge_rows(*rows, counts)
    got = host_merge(build[0], rows, counts)
    assert_builders_bounds(f"k = {k}", got, want)
    # the double covariance before the eigen tail is the spec's moment match
    rel = np.linalg.norm(got["cov"] - want["cov"], axis=(1, 2)) / np.linalg.norm(want["cov"], axis=(1, 2))
    assert float(rel.max()) <= 1e-12, float(rel.max())


def test_one_child_gives_the_child(build):
    rows = children(50, 1, seed=9)
    got = host_merge(build[0], rows, np.ones(50, dtype=np.int64))
    assert np.array_equal(got["xyz"], rows[0]) and np.array_equal(got["shs"], rows[1]) and np.array_equal(got["alpha"], rows[2])
    rel = np.linalg.norm(cov_of_row(got["log_scales"], got["rots"]) - cov_of_row(rows[3], rows[4]), axis=(1, 2)) / \
        np.linalg.norm(cov_of_row(rows[3], rows[4]), axis=(1, 2))
    assert float(rel.max()) <= 1e-2            # (the stored quaternion's norm, ~1e-3 off one, scales the child's covariance)
    q = rows[4].astype(np.float64)
    stored = (hierarchy._rot_from_quat(q) * np.exp(2.0 * rows[3].astype(np.float64))[:, None, :]) @ hierarchy._rot_from_quat(q).transpose(0, 2, 1)
    rel = np.linalg.norm(cov_of_row(got["log_scales"], got["rots"]) - stored, axis=(1, 2)) / np.linalg.norm(stored, axis=(1, 2))
    assert float(rel.max()) <= 1e-5


def test_mixed_counts_in_one_call(build):
    counts = np.array([1, 2, 3, 7, 2, 1, 7, 3] * 20)
    rows = children(int(counts.sum()), 1, seed=21)
    assert_builders_bounds("mixed", host_merge(build[0], rows, counts), hierarchy.merge_rows(*rows, counts))


def test_carried_weights_replace_the_rows_own(build):
    """Children that are merged nodes themselves: the weight is what was carried up from their leaves, not alpha s0 s1 s2."""
    counts = np.array([2, 3, 1, 7] * 25)
    rows = children(int(counts.sum()), 1, seed=33)
    w = np.random.default_rng(34).random(int(counts.sum())) * 3.0
    got, want = host_merge(build[0], rows, counts, w), hierarchy.merge_rows(*rows, counts, weights=w)
    assert_builders_bounds("carried weights", got, want)
    own = hierarchy.merge_rows(*rows, counts)
    assert float(np.abs(want["xyz"] - own["xyz"]).max()) > 0.1          # (the two rules are different rules)
    sums = np.add.reduceat(w, np.concatenate([[0], np.cumsum(counts)[:-1]]))
    assert np.allclose(want["weight"], sums, rtol=1e-15)


def test_two_children_of_equal_covariance(build):
    rows = children(200, 2, seed=4)
    rows[3][1::2], rows[4][1::2] = rows[3][0::2], rows[4][0::2]
    counts = np.full(200, 2)
    assert_builders_bounds("equal covariance", host_merge(build[0], rows, counts), hierarchy.merge_rows(*rows, counts))
    # ... and at the same place with the same weight: the parent is the child (an isotropic pair included)
    rows[0][1::2], rows[2][1::2] = rows[0][0::2], rows[2][0::2]
    rows[3][:20] = -1.0
    rows[3][1::2] = rows[3][0::2]
    got, want = host_merge(build[0], rows, counts), hierarchy.merge_rows(*rows, counts)
    assert_builders_bounds("same child twice", got, want)
    assert np.array_equal(got["xyz"], rows[0][0::2])


def test_a_child_of_zero_weight_and_all_weights_zero(build):
    rows = children(100, 3, seed=6)
    rows[2][1::3] = 0.0                                   # the middle child weighs nothing
    counts = np.full(100, 3)
    got, want = host_merge(build[0], rows, counts), hierarchy.merge_rows(*rows, counts)
    assert_builders_bounds("zero-weight child", got, want)
    two = [np.delete(a, np.arange(1, 300, 3), axis=0) for a in rows]
    pair = host_merge(build[0], two, np.full(100, 2))
    for key in ("xyz", "shs", "alpha", "log_scales", "rots"):
        assert np.array_equal(got[key], pair[key]), key   # ... exactly nothing
    rows[2][:] = 0.0                                      # all weights zero: the sum is clamped at 1e-30, every share is 0
    got, want = host_merge(build[0], rows, counts), hierarchy.merge_rows(*rows, counts)
    assert not got["xyz"].any() and not got["shs"].any() and not got["alpha"].any()
    assert not want["xyz"].any() and not want["cov"].any()
    assert np.allclose(got["log_scales"], np.log(np.sqrt(1e-12)), rtol=1e-6, atol=0)
    assert float(np.abs(np.linalg.norm(got["rots"].astype(np.float64), axis=1) - 1).max()) <= 1e-6


def test_the_stand_alone_program_passes(build):
    r = subprocess.run([build[1]], capture_output=True, text=True)
    assert r.returncode == 0 and "hier_merge_rule_host: ok" in r.stdout, r.stdout + r.stderr


def test_the_builder_and_the_pruner_include_the_header():
    csrc = os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc")
    for name in ("hier_build.hip", "hier_prune.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "hier_merge_rule.h"' in text and "merge_cov_to_row(" in text, name
        assert "jacobi_rotate(" not in text and "void jacobi_rotate" not in text, name
