"""The cut of a hierarchy whose boxes nest, without a loop over its entries: what ``frustum_spec.cut_view_spec`` returns,
from the per-node sizes of ``budget_cut_spec.View``.  ``oracle.lod_oracle.expand_to_size`` walks the tree and then appends
every entry in Python, which is no reference at a million entries; when the sizes never grow from parent to child, "all
ancestors are too coarse" is "the parent is too coarse" and every node decides for itself (csrc/lod_cut.h, cut_count).
tests/test_big_cut_spec_cpu.py holds the two together, every array and the weights' bit patterns.  TEST INFRASTRUCTURE
ONLY."""
from __future__ import annotations

import numpy as np

from oracle import lod_oracle as lo

F = np.float32


def nested_cut_spec(view, tau):
    """``view``: a ``budget_cut_spec.View`` (its ``kept`` is the cull: all True without planes).
    -> dict(n, n_unculled, render_indices, parent_indices, node_indices, weights, kids, culled)."""
    assert view.nested(), "nested_cut_spec: a child is larger than its parent from this viewpoint -- use the looped oracle"
    nodes = view.nodes
    N = nodes.shape[0]
    tau = F(tau)
    coarse = view.s >= tau
    reached = view.s_par >= tau
    count = np.where(reached, np.where(coarse, view.L, view.L + view.M), 0).astype(np.int64)
    ni = np.repeat(np.arange(N, dtype=np.int64), count)             # ascending node order
    first = np.cumsum(count) - count
    k = np.arange(ni.shape[0], dtype=np.int64) - np.repeat(first, count)
    r = nodes[ni, 2].astype(np.int64) + k
    par = nodes[ni, 1].astype(np.int64)
    pg = np.where(par >= 0, nodes[np.maximum(par, 0), 2].astype(np.int64), -1)
    p = np.where(pg >= 0, pg, r)
    if ni.shape[0]:
        with np.errstate(over="ignore"):                            # (2 tau at a huge tau)
            w, kids = lo.get_interpolation_weights(ni, tau, nodes, view.boxes, view.viewpoint)
    else:
        w, kids = np.zeros(0, np.float32), np.zeros(0, np.int32)
    keep = view.kept[ni]
    i32 = lambda a: a.astype(np.int32)
    return dict(n=int(keep.sum()), n_unculled=int(ni.shape[0]), render_indices=i32(r[keep]), parent_indices=i32(p[keep]),
                node_indices=i32(ni[keep]), weights=w[keep], kids=kids[keep], culled=~keep)
