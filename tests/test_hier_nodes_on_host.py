"""The PRODUCT's layout checks (csrc/hier_nodes.h: node_layout, the one text hm_nodes_kernel and ht_plan_kernel run)
compiled for the HOST and held against hgs.hierarchy.layout_check_masks / trim_layout_checks -- no GPU.  The header is
copied unchanged at test time and compiled with g++ against tests/harness/host_math/common.h, as
tests/test_device_math_on_host.py does with gaussian_math.h; tests/hier_nodes_cases.py holds the corrupted arrays, which
tests/test_hier_nodes_gpu.py feeds to the two kernels."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hier_nodes_cases as hc
from hgs import hierarchy

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "host_math")
BITS = (1, 2, 4)          # kBadRow, kBadChildren, kBadParent
IN_RANGE = 8              # kParentInRange


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("hier_nodes")
    for f in (os.path.join(HARNESS, "common.h"), os.path.join(HARNESS, "hier_nodes_host.cpp"),
              os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc", "hier_nodes.h")):
        shutil.copy(f, d)
    so = os.path.join(d, "libhiernodes.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", str(d), os.path.join(d, "hier_nodes_host.cpp"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(so)


def verdict(host, nodes):
    nodes = np.ascontiguousarray(nodes, dtype=np.int32)
    N = nodes.shape[0]
    v, first = np.zeros(N, np.uint32), np.zeros(3, np.int32)
    host.host_node_layout(nodes.ctypes.data_as(C.c_void_p), N, v.ctypes.data_as(C.c_void_p), first.ctypes.data_as(C.c_void_p))
    return v, first.tolist()


def test_the_record_width(host):
    assert host.host_node_ints() == 7 == hc.built(2).nodes.shape[1]


@pytest.mark.parametrize("P", hc.LEAVES)
def test_every_verdict_and_the_first_offenders_equal_the_numpy_checks(host, P):
    table = hc.cases(P)
    N = 2 * P - 1
    assert table[0][0] == "clean" and table[0][1].shape == (N, 7)
    for label, nodes in table:
        v, first = verdict(host, nodes)
        masks = hierarchy.layout_check_masks(nodes)
        for bit, mask in zip(BITS, masks):
            assert np.array_equal((v & bit) != 0, mask), (label, bit)
        parent = nodes[:, hc.PARENT].astype(np.int64)
        in_range = (np.arange(N) > 0) & (parent >= 0) & (parent < N)
        assert np.array_equal((v & IN_RANGE) != 0, in_range), label
        assert first == hc.expected(nodes), label
        assert not (v >> 4).any(), label
    assert verdict(host, table[0][1])[1] == [-1, -1, -1]                       # the clean array: no offender


def test_the_table_holds_what_it_names():
    """The corruptions do what their names say (so the comparison above is not between two empty sets): on N = 513 nodes,
    at node 256, which checks fire."""
    clean = hc.built(257).nodes.numpy().astype(np.int32)
    want = {"start != i": [256, -1, -1], "leafs + merged = 0": [256, -1, -1], "leafs + merged = 2": [256, -1, -1],
            "cc = -1": [-1, 256, None], "cc > 0 with sc = 0": [-1, 256, None], "sc + cc = N (legal)": [-1, -1, None],
            "sc + cc = N + 1": [-1, 256, None], "sc = 2^31 - 1 with cc = 1": [-1, 256, None],
            "parent = -1": [-1, -1, 256], "parent = N": [-1, -1, 256],
            "a parent in range that does not claim the node": [-1, -1, 256],
            "leafs + merged = 1 - 2^32": [256, -1, -1], "the parent's cc = 2^31 - 1": [-1, None, -1]}
    for name, exp in want.items():
        nd = clean.copy()
        hc.CORRUPTIONS[name][0](nd, 256)
        got = hierarchy.trim_layout_checks(nd)
        # (a changed children range orphans or adopts other nodes: the parent check is then the orphans', not asserted)
        assert all(e is None or g == e for g, e in zip(got, exp)), (name, got)
    nd = clean.copy()
    hc.CORRUPTIONS["node 0 with parent = 0"][0](nd, 0)
    assert hierarchy.trim_layout_checks(nd) == [-1, -1, 0]
