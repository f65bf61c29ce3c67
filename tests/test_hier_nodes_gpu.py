"""The three layout checks on the device: hm_nodes_kernel (hgs_hier_merge_place) and ht_plan_kernel (hgs_hier_trim_plan)
run ONE text, csrc/hier_nodes.h node_layout, so both must report the same first offenders for the same node array -- and
these must be hgs.hierarchy.trim_layout_checks'.  The arrays are tests/hier_nodes_cases.py's (the table
tests/test_hier_nodes_on_host.py runs through the header on the host) at N = 1, 257 and 513: offenders on either side
of a 256-thread workgroup boundary, alone and in pairs.  Merge reports and returns HGS_OK (its caller refuses the chunk);
trim refuses with the message of the first failing check."""
import ctypes as C

import pytest
import torch

import hier_nodes_cases as hc
from hgs import _lib, hierarchy
from test_hier_trim_cpu import ARRAYS
from test_hier_trim_gpu import AbiRun, _args, _stream, to_dev

pytestmark = pytest.mark.gpu


def _view(h, G, N, M):
    return _lib.HierView(G, N, M, 0, *(getattr(h, k).data_ptr() for k in ARRAYS))


@pytest.mark.parametrize("P", [1, 129, 257])
def test_merge_and_trim_report_the_first_offenders_of_the_numpy_checks(gpu, P):
    lib = _lib.lib()
    h = hc.built(P)
    N, M = h.num_nodes, h.shs.shape[1]
    # merge: the array as the one chunk of k = 1 -> merged N + 1 nodes, the chunk's nodes 1 .. N - 1 from base 2
    chunk = to_dev(h, gpu)
    merged = hierarchy.Hierarchy(*(torch.empty(N + 1, *getattr(h, k).shape[1:], dtype=getattr(h, k).dtype, device=gpu)
                                   for k in ARRAYS))
    tmp = torch.empty(_lib.HIER_MERGE_TMP_BYTES, dtype=torch.uint8, device=gpu)
    run = AbiRun(h, gpu)                   # trim: the hierarchy in guarded allocations; the node array is overwritten
    table = hc.cases(P)
    assert len(table) > 10 and table[0][0] == "clean"
    seen = set()
    for label, nodes in table:
        want = hc.expected(nodes)
        seen.update(c for c in range(3) if want[c] >= 0)
        dev_nodes = torch.from_numpy(nodes).to(gpu)
        chunk.nodes.copy_(dev_nodes)
        run.inputs["nodes"].body[:N * 28] = dev_nodes.reshape(-1).view(torch.uint8)
        rep = _lib.HierMergeReport()
        rc = lib.hgs_hier_merge_place(C.byref(_view(chunk, N, N, M)), 0, 1, 2, C.byref(_view(merged, N + 1, N + 1, M)),
                                      tmp.data_ptr(), C.byref(rep), _stream(), gpu.index or 0)
        assert rc == 0, (label, lib.hgs_last_error())                 # a failing chunk is reported, not refused
        assert list(rep.first_bad) == want, label
        rc, trim = run.plan(_args(0.0))                               # (floor 0: every node passes, closure cannot fail)
        assert list(trim.first_bad) == want + [-1], label
        if want == [-1, -1, -1]:
            assert rc == 0 and trim.kept == N, label
        else:
            c = next(c for c in range(3) if want[c] >= 0)
            msg = (f"not a hierarchy that can be trimmed: {hierarchy.TRIM_CHECKS[c]} (first offending node {want[c]}); "
                   f"nothing was written")
            assert rc == 1 and lib.hgs_last_error().decode() == msg, label
    run.guards()
    assert hc.expected(table[0][1]) == [-1, -1, -1] and seen == {0, 1, 2}
