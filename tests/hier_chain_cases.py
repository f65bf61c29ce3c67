"""Shared cases of the tool-chain tests (test_hier_chain_cpu.py, test_hier_chain_gpu.py): a helper module, not a test.

Every hierarchy tool and every cut is tested elsewhere on what the numpy builder makes (a complete binary tree in BFS
order) and on three built chunks under one root.  Here the tools' OUTPUTS are the inputs: nodes with a single child
(prune), leaves at mixed depths (trim), nodes with three children below the root (a merge of merges), rows that went
through half precision (compress).  Four bases, eight tools with fixed arguments -- the spec and the device function of
a tool receive the very same ones -- and six kinds of derived hierarchies, all made with the numpy specs and never
modified afterwards."""
import functools

import numpy as np
import torch

import half_rows_cases as hc
from hgs import hierarchy, residency
from oracle import lod_oracle as lo
from test_hier_prune_cpu import removal_mask
from test_hier_prune_gpu import with_width          # (the module imports without a GPU)
from test_hier_refit_cpu import built
from test_hier_transform_cpu import general
from test_hier_trim_cpu import ARRAYS, merged_case

BASES = ("built129", "built257", "merged", "built129_sh4")
TOOLS = ("prune", "prune_under1", "trim", "trim_to_views", "refit", "align", "transform", "merge")
PAIRS = [(a, b) for a in TOOLS for b in TOOLS]
KINDS = ("pruned", "pruned_trimmed", "trimmed_pruned", "pruned_refit", "pruned_half")
DERIVED = [(kind, b) for b in BASES for kind in KINDS] + [("merged_of_merged", "merged")]
PRUNED_KINDS = ("pruned", "pruned_trimmed", "trimmed_pruned", "pruned_refit", "pruned_half")

# trim_to_views: two view points in front of and beside the scenes, one granularity
VIEW_POINTS = ((0.0, 0.0, -5.0), (30.0, 2.0, 10.0))
VIEW_TAU = 0.5
# the fixed cut of the CPU tests
CUT_TAU, CUT_VIEW = 0.02, (0.0, 0.0, -5.0)


@functools.lru_cache(maxsize=None)
def base(name):
    """One of BASES: built(129) and built(257), one on each side of a 256-node workgroup; three chunks under a root with
    k = 3; built(129) with four SH coefficients per row."""
    return {"built129": lambda: built(129), "built257": lambda: built(257), "merged": lambda: merged_case()[0],
            "built129_sh4": lambda: with_width(built(129), 4)}[name]()


def view_regions():
    return hierarchy.view_regions(points=VIEW_POINTS)


def median_extent(h):
    """The float32 median of the extents of the nodes with children."""
    ext = h.boxes.reshape(-1, 2, 4)[:, 0, 3].numpy()[h.nodes[:, 6].numpy() > 0]
    return float(np.float32(np.median(ext)))


def tool_args(tool, h):
    """(positional, keyword) arguments of ``tool`` on the host hierarchy ``h``: what the spec function and the device
    function both receive (the device one behind the uploaded hierarchy)."""
    if tool == "prune":
        return (), dict(remove=removal_mask(h, "every_second_leaf"), remerge="dirty")
    if tool == "prune_under1":
        return (), dict(remove=removal_mask(h, "under_node_1"))
    if tool == "trim":
        return (), dict(min_extent=median_extent(h))
    if tool == "trim_to_views":
        return (view_regions(), VIEW_TAU), {}
    if tool == "refit":
        return (), dict(leaf="cube")
    if tool == "align":
        return (), {}
    if tool == "transform":
        return (general(),), {}
    if tool == "merge":
        return ([h, hierarchy.transform_hierarchy(h, general())],), {}
    raise ValueError(tool)


SPEC = {"prune": hierarchy.prune_hierarchy, "prune_under1": hierarchy.prune_hierarchy, "trim": hierarchy.trim_hierarchy,
        "trim_to_views": hierarchy.trim_to_views, "refit": hierarchy.refit_boxes, "align": hierarchy.align_hierarchy,
        "transform": hierarchy.transform_hierarchy}


def spec(tool, h):
    """The numpy spec of ``tool`` on ``h`` with ``tool_args`` -> what the spec returns (a result object or a Hierarchy).
    A refusal (``hierarchy.HierarchyCheckError``) is raised, not hidden."""
    args, kw = tool_args(tool, h)
    if tool == "merge":
        return hierarchy.merge_hierarchies(*args)
    return SPEC[tool](h, *args, **kw)


def hier(result):
    """The Hierarchy of a spec's or a device function's return value."""
    return result if isinstance(result, hierarchy.Hierarchy) else result.hierarchy


@functools.lru_cache(maxsize=None)
def after(tool, base_name):
    """``spec(tool, base)``, once; the raised refusal where the spec refuses."""
    try:
        return spec(tool, base(base_name))
    except hierarchy.HierarchyCheckError as e:
        return e


def half_round_trip(h):
    """Every row but the mean narrowed to half (hgs.residency.narrow_to_half) and widened through the table of
    half_rows_cases: what hgs.compress_hierarchy stores, as the loader gives it back."""
    rt = lambda t: torch.from_numpy(hc.widen(residency.narrow_to_half(t.numpy().reshape(-1))).reshape(tuple(t.shape)).copy())
    return hierarchy.Hierarchy(h.xyz.clone(), rt(h.shs), rt(h.alpha), rt(h.log_scales), rt(h.rots), h.nodes.clone(), h.boxes.clone())


@functools.lru_cache(maxsize=None)
def derived_result(kind, base_name):
    """The last spec call behind ``derived(kind, base_name)`` (a PruneResult, TrimResult or Hierarchy)."""
    b = base(base_name)
    if kind in ("pruned", "pruned_half"):
        return spec("prune", b)
    if kind == "pruned_trimmed":
        return spec("trim", derived("pruned", base_name))
    if kind == "trimmed_pruned":
        return spec("prune", hier(spec("trim", b)))
    if kind == "pruned_refit":
        return spec("refit", derived("pruned", base_name))
    if kind == "merged_of_merged":
        return spec("merge", b)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def derived(kind, base_name):
    """One of DERIVED as a host Hierarchy; do not modify."""
    h = hier(derived_result(kind, base_name))
    return half_round_trip(h) if kind == "pruned_half" else h


def structure(h):
    """dict(single_child, wide_below_root, early_leaves, max_depth): the nodes with exactly one child; the nodes other
    than node 0 with three or more; the leaves above the deepest level; the largest depth."""
    nd = h.nodes.numpy()
    depth, cc = nd[:, 0], nd[:, 6]
    return dict(single_child=int((cc == 1).sum()), wide_below_root=int((cc[1:] >= 3).sum()),
                early_leaves=int(((cc == 0) & (depth < depth.max())).sum()), max_depth=int(depth.max()))


def oracle_cut(h, tau=CUT_TAU, v=CUT_VIEW):
    """(render, parent, node indices, weights, kids) of oracle/lod_oracle.py."""
    nd, bx = h.nodes.numpy(), h.boxes.numpy().reshape(-1, 2, 4)
    ri, pi, ni = lo.expand_to_size(nd, bx, tau, v)
    w, kids = lo.get_interpolation_weights(ni, tau, nd, bx, v)
    return ri, pi, ni, w, kids


def two_children_cut(h, tau=CUT_TAU, v=CUT_VIEW):
    """The cut and weights a WRONG kernel would give: one that takes every node with children to have exactly two, at
    start_children and start_children + 1 (a child index past the last node is dropped), and every sibling count to be
    2.  What the builder makes cannot tell it from the oracle; the cases here must."""
    nd, bx = h.nodes.numpy(), h.boxes.numpy().reshape(-1, 2, 4)
    N = nd.shape[0]
    fake = nd.copy()
    inner = fake[:, 6] > 0
    fake[inner, 6] = np.minimum(2, N - fake[inner, 5])
    ri, pi, ni = lo.expand_to_size(fake, bx, tau, v)
    w, kids = lo.get_interpolation_weights(ni, tau, fake, bx, v)
    return ri, pi, ni, w, np.where(nd[ni, 1] >= 0, 2, 1).astype(np.int32)


def same_cut(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[:3] + a[4:], b[:3] + b[4:])) and \
        np.array_equal(np.asarray(a[3], dtype=np.float32).view(np.uint32), np.asarray(b[3], dtype=np.float32).view(np.uint32))


def clone(h):
    return hierarchy.Hierarchy(*(getattr(h, k).clone() for k in ARRAYS))
