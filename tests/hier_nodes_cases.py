"""Node arrays with broken layouts, for the tests of the three layout checks (csrc/hier_nodes.h node_layout, restated by
hgs.hierarchy.layout_check_masks): tests/test_hier_nodes_on_host.py compiles the header for the host,
tests/test_hier_nodes_gpu.py feeds the same table to hgs_hier_merge_place and hgs_hier_trim_plan.  The arrays come from
the numpy builder; every corruption is applied alone at nodes 0, 255, 256 and N - 1 where they exist (255 | 256: the two
sides of a 256-thread workgroup boundary), and at two nodes at once so that the minimum over offenders is exercised."""
import functools

import numpy as np

from hgs import hierarchy, synth

CAM = synth.make_camera(256, 160)
LEAVES = (1, 2, 129, 257)            # N = 2 P - 1 = 1, 3, 257, 513
DEPTH, PARENT, START, LEAFS, MERGED, SC, CC = range(7)
INT_MAX = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def built(P):
    """The numpy builder's hierarchy over P leaves (host tensors; do not modify)."""
    return hierarchy.build_hierarchy(synth.make_scene(P, CAM, seed=P))


def _set(**cols):
    def apply(nd, n):
        for name, v in cols.items():
            nd[n, globals()[name]] = v(nd, n) if callable(v) else v
    return apply


# name -> (corruption of row n in place, the nodes it applies to: None = any)
CORRUPTIONS = {
    "start != i": (_set(START=lambda nd, n: n + 1), None),
    "leafs + merged = 0": (_set(LEAFS=0, MERGED=0), None),
    "leafs + merged = 2": (_set(LEAFS=1, MERGED=1), None),
    "cc = -1": (_set(CC=-1), None),
    "cc > 0 with sc = 0": (_set(SC=0, CC=1), None),
    "sc + cc = N (legal)": (_set(SC=lambda nd, n: nd.shape[0] - 1, CC=1), None),
    "sc + cc = N + 1": (_set(SC=lambda nd, n: nd.shape[0] - 1, CC=2), None),
    "sc = 2^31 - 1 with cc = 1": (_set(SC=INT_MAX, CC=1), None),
    "parent = -1": (_set(PARENT=-1), lambda n: n != 0),
    "parent = N": (_set(PARENT=lambda nd, n: nd.shape[0]), None),
    "a parent in range that does not claim the node": (_set(PARENT=lambda nd, n: nd.shape[0] - 1), lambda n: n != 0),
    "node 0 with parent = 0": (_set(PARENT=0), lambda n: n == 0),
    # beyond the list above, the two other sums that 32-bit arithmetic would get wrong: 1 - 2^32 wraps to 1, and a parent
    # whose start_children + 2^31 - 1 wraps to a negative end of its range (it claims the node in 64 bits)
    "leafs + merged = 1 - 2^32": (_set(LEAFS=-INT_MAX - 1, MERGED=-INT_MAX), None),
    "the parent's cc = 2^31 - 1": (lambda nd, n: nd.__setitem__((nd[n, PARENT], CC), INT_MAX), lambda n: n != 0),
}


def targets(N):
    return sorted({n for n in (0, 255, 256, N - 1) if n < N})


@functools.lru_cache(maxsize=None)
def cases(P):
    """-> [(label, int32 nodes [N,7])]: the clean array first, then every corruption alone, then pairs."""
    clean = built(P).nodes.numpy().astype(np.int32)
    N = clean.shape[0]
    at = targets(N)
    out = [("clean", clean)]

    def make(*edits):
        nd = clean.copy()
        for name, n in edits:
            CORRUPTIONS[name][0](nd, n)
        return ", ".join(f"{name} at {n}" for name, n in edits), nd

    ok = lambda name, n: CORRUPTIONS[name][1] is None or CORRUPTIONS[name][1](n)
    for name in CORRUPTIONS:
        nodes = [n for n in at if ok(name, n)]
        out += [make((name, n)) for n in nodes]
        if len(nodes) >= 2:                       # the same check at two nodes, the later one listed first
            out.append(make((name, nodes[-1]), (name, nodes[-2])))
    if N > 1:                                     # different checks at two nodes, either order of the indices
        a, b = at[-2], at[-1]
        for first, second in (("start != i", "cc = -1"), ("cc = -1", "parent = N"), ("parent = N", "leafs + merged = 2")):
            out += [make((first, b), (second, a)), make((first, a), (second, b))]
        out.append(make(("start != i", b), ("cc = -1", b), ("parent = N", b), ("sc + cc = N + 1", a)))
    return out


def expected(nodes):
    """hgs.hierarchy.trim_layout_checks: [first offending node or -1] x 3."""
    return hierarchy.trim_layout_checks(nodes)
