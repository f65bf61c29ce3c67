"""Frustum-culled hierarchy cut (opt-in; csrc/lod_frustum.hip, include/hgs.h "Frustum-culled cut").

``gaussian_hierarchy._C.expand_to_size`` selects by granularity only: a camera inside a scene gets the cut of the whole
sphere around it.  Here every node carries a view-independent ball around its own rows, and an entry is dropped when one
of five widened frustum planes has both the node's ball and its parent's outside -- a rule under which nothing the
rasterizer would draw is lost::

    bounds = cull_bounds(nodes, means3D, scales)                        # once per hierarchy (activated scales)
    planes, rs = frustum_planes(cam.world_view_transform, tanfovx, tanfovy, W, H)
    cut = cut_view(nodes, boxes, bounds, tau, cam.camera_center, planes, rs)
    # cut.render_indices / parent_indices / weights / kids go to GaussianRasterizationSettings as the outputs of
    # expand_to_size + get_interpolation_weights do

The kept entries are exactly those of the unculled cut, in its order, with its parents, weights and sibling counts.

``cut_to_budget`` (csrc/lod_budget.hip, include/hgs.h "Budget-exact cut") is the same cut at the finest granularity
``tau* >= tau_min`` whose cost -- entries, or the rows a budgeted viewer has to hold -- is at most ``budget``: one call,
no trial cuts::

    bc = cut_to_budget(nodes, boxes, bounds, budget_rows, cam.camera_center, planes, rs, tau_min=tau)
    # bc.tau is what was rendered, bc.cost <= budget_rows; the other fields are those of cut_view at bc.tau

``cut_views`` (csrc/lod_views.hip, include/hgs.h "Cut for several views") is ``cut_view`` for several views at once --
a batch of training views with a granularity each, a stereo pair, the current camera and a predicted one: one pass over
the nodes and one host wait for all of them, every view's result bit for bit what ``cut_view`` gives it::

    cuts = cut_views(nodes, boxes, bounds, taus, centers, planes, radius_scales)     # cuts[v] is a CutView"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

NEAR_Z = 0.2        # the rasterizer's near cull (view z)
_K1_CLAMP = 1.3     # the rasterizer's clamp on t.x / t.z, in units of tanfov
_PAD_PX = 36.0      # the widened plane leaves (fov_scale - 1) W / 2 >= 18 px for dilation, ceil and tile rounding


@dataclass
class CutView:
    """One culled cut.  The tensors are views of the output buffers (``out``, or freshly allocated ones)."""
    n: int                          # kept entries
    n_unculled: int                 # entries of the cut without the cull (what expand_to_size returns)
    render_indices: torch.Tensor    # int32 [n]
    parent_indices: torch.Tensor    # int32 [n]
    node_indices: torch.Tensor      # int32 [n]
    weights: torch.Tensor           # f32 [n]
    kids: torch.Tensor              # int32 [n]


class CutBuffers:
    """Preallocated outputs of ``cut_view`` (``out=``): ri, pi, ni (int32), w (float32), ns (int32), ``cap`` entries each.
    Any object with these five attributes will do."""

    def __init__(self, cap, device):
        i32 = dict(dtype=torch.int32, device=device)
        self.ri = torch.zeros(cap, **i32); self.pi = torch.zeros(cap, **i32); self.ni = torch.zeros(cap, **i32)
        self.w = torch.zeros(cap, dtype=torch.float32, device=device)
        self.ns = torch.zeros(cap, **i32)


def frustum_planes(world_view_transform, tanfovx, tanfovy, width, height, scale_modifier=1.0, near=NEAR_Z):
    """-> (planes float32 CPU [5,4], radius_scale).  Row k = (a, d), |a| = 1, a . x + d >= 0 inside: the left, right,
    -y and +y side planes through the camera centre at tangents ``fov_scale * tanfov`` with
    ``fov_scale = max(1.3, 1 + 36 / min(width, height))``, then the near plane view z = ``near``.  Built in double from
    the stored (row-vector) ``world_view_transform`` (view = [x 1] @ M), rounded once.
    ``radius_scale = max(1, scale_modifier) * sqrt((1 + 1.69 (tx^2 + ty^2)) / (1 + 1.69 min(tx, ty)^2))``."""
    M = np.asarray(torch.as_tensor(world_view_transform).detach().to("cpu", torch.float64).numpy()).reshape(4, 4)
    tx, ty = float(tanfovx), float(tanfovy)
    if not (tx > 0.0 and ty > 0.0 and int(width) > 0 and int(height) > 0):
        raise ValueError("frustum_planes: tanfovx, tanfovy, width and height must be positive")
    fov_scale = max(_K1_CLAMP, 1.0 + _PAD_PX / min(int(width), int(height)))
    wx, wy = fov_scale * tx, fov_scale * ty
    rows = (((1.0, 0.0, wx), 0.0), ((-1.0, 0.0, wx), 0.0), ((0.0, 1.0, wy), 0.0), ((0.0, -1.0, wy), 0.0),
            ((0.0, 0.0, 1.0), -float(near)))
    planes = np.zeros((5, 4), dtype=np.float64)
    for k, (nv, d0) in enumerate(rows):
        a = [sum(M[i, j] * nv[j] for j in range(3)) for i in range(3)]
        d = sum(M[3, j] * nv[j] for j in range(3)) + d0
        ln = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        if not ln > 0.0:
            raise ValueError("frustum_planes: degenerate world_view_transform")
        planes[k] = (a[0] / ln, a[1] / ln, a[2] / ln, d / ln)
    k2 = _K1_CLAMP * _K1_CLAMP
    kappa = math.sqrt((1.0 + k2 * (tx * tx + ty * ty)) / (1.0 + k2 * min(tx, ty) ** 2))
    return torch.from_numpy(planes.astype(np.float32)), max(1.0, float(scale_modifier)) * kappa


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _need(t, name, dtype, shape_ok, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, not {t.dtype}")
    if not shape_ok(t):
        raise ValueError(f"{name} must be {what}, not {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def cull_bounds(nodes, means3D, scales) -> torch.Tensor:
    """float32 [N,4] = (centre, radius) of every node's own rows: the mean of the rows' means and
    max_i(|m_i - c| + 3 max_k s_i,k) on ACTIVATED ``scales``.  View independent; rebuild it when the rows change."""
    _need(nodes, "nodes", torch.int32, lambda t: t.dim() == 2 and t.shape[1] == 7, "[N,7]")
    G = int(means3D.shape[0]) if torch.is_tensor(means3D) and means3D.dim() >= 1 else 0
    _need(means3D, "means3D", torch.float32, lambda t: t.dim() == 2 and t.shape[1] == 3, "[G,3]")
    _need(scales, "scales", torch.float32, lambda t: t.dim() == 2 and tuple(t.shape) == (G, 3), "[G,3]")
    dev = nodes.device
    if means3D.device != dev or scales.device != dev:
        raise ValueError("nodes, means3D and scales must live on one device")
    N = int(nodes.shape[0])
    bounds = torch.empty(N, 4, dtype=torch.float32, device=dev)
    p = _lib.ptr
    _lib.check(_lib.lib().hgs_hier_cull_bounds(p(nodes), N, p(means3D), p(scales), G, p(bounds), _stream(dev),
                                               dev.index or 0), "hgs_hier_cull_bounds")
    return bounds


def _host_floats(t, n, name):
    v = t.detach().to("cpu", torch.float32).reshape(-1) if torch.is_tensor(t) else torch.tensor(t, dtype=torch.float32).reshape(-1)
    if v.numel() != n:
        raise ValueError(f"{name} must hold {n} values, not {v.numel()}")
    return (C.c_float * n)(*[float(x) for x in v])


def _check_hierarchy(nodes, boxes, bounds, planes, cull=True):
    """What cut_view and cut_to_budget ask of their hierarchy -> (N, device, the planes as 20 host floats).  ``cull``
    False: a cut without the frustum cull, ``bounds`` and ``planes`` are not looked at and the planes come back None."""
    _need(nodes, "nodes", torch.int32, lambda t: t.dim() == 2 and t.shape[1] == 7, "[N,7]")
    N = int(nodes.shape[0])
    _need(boxes, "boxes", torch.float32, lambda t: t.numel() == N * 8, "[N,2,4]")
    dev = nodes.device
    if not cull:
        if boxes.device != dev:
            raise ValueError("nodes and boxes must live on one device")
        return N, dev, None
    _need(bounds, "bounds", torch.float32, lambda t: t.dim() == 2 and tuple(t.shape) == (N, 4), "[N,4]")
    if boxes.device != dev or bounds.device != dev:
        raise ValueError("nodes, boxes and bounds must live on one device")
    if torch.is_tensor(planes) and tuple(planes.shape) != (5, 4):
        raise ValueError(f"planes must be [5,4], not {tuple(planes.shape)}")
    return N, dev, _host_floats(planes, 20, "planes")


def _check_out(bufs, dev):
    for name, dtype in (("ri", torch.int32), ("pi", torch.int32), ("ni", torch.int32), ("w", torch.float32),
                        ("ns", torch.int32)):
        _need(getattr(bufs, name), f"out.{name}", dtype, lambda t: t.dim() == 1, "one-dimensional")
        if getattr(bufs, name).device != dev:
            raise ValueError(f"out.{name} must live on the hierarchy's device")


def cut_view(nodes, boxes, bounds, tau, viewpoint, planes, radius_scale, out=None, nested=None) -> CutView:
    """The LOD cut at granularity ``tau`` from ``viewpoint`` minus the entries outside ``planes`` (``frustum_planes``),
    with the kept entries' weights and sibling counts: ``expand_to_size`` + ``get_interpolation_weights`` + the cull in
    one call.  ``viewpoint`` (3 values) and ``planes`` ([5,4]) are read on the host -- pass CPU tensors in a frame loop.
    ``out``: preallocated buffers (``CutBuffers``) -- a cut that does not fit them raises ``_lib.HgsError`` naming the
    count; without it the outputs are allocated to fit.  ``nested``: force the single-pass (True) or level-by-level
    (False) route; default: single pass when the boxes nest, as ``expand_to_size`` decides."""
    N, dev, pl = _check_hierarchy(nodes, boxes, bounds, planes)
    vp = _host_floats(viewpoint, 3, "viewpoint")
    own = out is None
    bufs = CutBuffers(max(N, 1), dev) if own else out
    _check_out(bufs, dev)
    lib = _lib.lib()
    if nested is None:
        from gaussian_hierarchy._C import _boxes_nested
        nested = N > 0 and _boxes_nested(nodes, boxes)
    tmp = torch.empty(lib.hgs_lod_cut_view_tmp_bytes(N), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    for attempt in range(2):
        cap = min(t.numel() for t in (bufs.ri, bufs.pi, bufs.ni, bufs.w, bufs.ns))
        n, n_all = C.c_int32(0), C.c_int32(0)
        rc = lib.hgs_lod_cut_view(p(nodes), p(boxes), p(bounds), N, float(tau), vp, pl, float(radius_scale),
                                  1 if nested else 0, p(bufs.ri), p(bufs.pi), p(bufs.ni), p(bufs.w), p(bufs.ns), cap,
                                  p(tmp), C.byref(n), C.byref(n_all), _stream(dev), dev.index or 0)
        if rc != 0 and own and attempt == 0 and n.value > cap:      # nodes of several rows: allocate what it takes
            bufs = CutBuffers(int(n.value), dev)
            continue
        _lib.check(rc, "hgs_lod_cut_view")
        break
    k = int(n.value)
    return CutView(k, int(n_all.value), bufs.ri[:k], bufs.pi[:k], bufs.ni[:k], bufs.w[:k], bufs.ns[:k])


@dataclass
class BudgetCut(CutView):
    """A ``CutView`` at the granularity ``cut_to_budget`` chose."""
    tau: float = 0.0                # tau*: exactly a float32 value
    cost: int = 0                   # the cost of the cut at tau* under the requested cost (<= budget)


_COSTS = {"entries": _lib.CUT_COST_ENTRIES, "rows": _lib.CUT_COST_ROWS}


def cut_to_budget(nodes, boxes, bounds, budget, viewpoint, planes=None, radius_scale=1.0, tau_min=0.0, cost="rows",
                  out=None) -> BudgetCut:
    """The cut at the finest granularity ``tau* >= tau_min`` that costs at most ``budget``, with weights and sibling
    counts -- what ``cut_view`` returns at ``tau*``, bit for bit -- and ``tau*`` itself, in one call (no trial cuts, one
    host wait).  ``cost``: "entries" (the length of the cut) or "rows" (the entries plus the distinct parent rows that
    entries of weight < 1 read: what ``BudgetedHierarchy.make_resident`` has to hold).  ``tau*`` is ``tau_min`` when the
    request fits; otherwise the result of the radix descent of include/hgs.h: ``cost(tau*) <= budget`` while the next
    float32 below costs more -- the smallest fitting granularity wherever the cost does not rise with tau (always for
    "entries" without planes).  ``bounds`` and ``planes`` are both given (the frustum cull of ``cut_view``) or both
    None.  The boxes must nest (every hierarchy this package builds or merges); a budget below the cost of the coarsest
    cut raises ``_lib.HgsError`` with code ``ERR_CAPACITY`` naming that cost, and nothing is written.  ``out``:
    preallocated buffers of at least ``budget`` entries (``CutBuffers``)."""
    if (bounds is None) != (planes is None):
        raise ValueError("bounds and planes go together: give both or neither")
    N, dev, pl = _check_hierarchy(nodes, boxes, bounds, planes, cull=bounds is not None)
    vp = _host_floats(viewpoint, 3, "viewpoint")
    if cost not in _COSTS:
        raise ValueError(f"cost must be 'entries' or 'rows', not {cost!r}")
    if N < 1:
        raise ValueError("an empty hierarchy has no cut")
    budget, tau_min = int(budget), float(tau_min)
    if budget < 0 or budget > 2 ** 31 - 1:
        raise ValueError(f"budget must be in [0, 2^31), not {budget}")
    if not tau_min >= 0.0:
        raise ValueError(f"tau_min must be >= 0, not {tau_min}")
    from gaussian_hierarchy._C import _boxes_nested
    if not _boxes_nested(nodes, boxes):
        raise ValueError("cut_to_budget needs a hierarchy whose boxes nest (every child's box inside its parent's): "
                         "these do not -- use cut_view / BudgetedHierarchy.select(fit='regulate')")
    if out is None:
        # no cut costs more than every row plus every node: a larger budget asks for the same cut
        rows = int((nodes[:, 3].long() + nodes[:, 4].long()).clamp(min=0).sum()) + N
        budget = min(budget, rows)
        bufs = CutBuffers(max(budget, 1), dev)
    else:
        bufs = out
    _check_out(bufs, dev)
    lib = _lib.lib()
    tmp = torch.empty(lib.hgs_lod_cut_budget_tmp_bytes(N), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    cap = min(t.numel() for t in (bufs.ri, bufs.pi, bufs.ni, bufs.w, bufs.ns))
    n, n_all, tau, cst = C.c_int32(0), C.c_int32(0), C.c_float(0.0), C.c_int32(0)
    _lib.check(lib.hgs_lod_cut_budget(p(nodes), p(boxes), p(bounds), N, tau_min, budget, _COSTS[cost], vp, pl,
                                      float(radius_scale), p(bufs.ri), p(bufs.pi), p(bufs.ni), p(bufs.w), p(bufs.ns),
                                      cap, p(tmp), C.byref(n), C.byref(n_all), C.byref(tau), C.byref(cst), _stream(dev),
                                      dev.index or 0), "hgs_lod_cut_budget")
    k = int(n.value)
    return BudgetCut(k, int(n_all.value), bufs.ri[:k], bufs.pi[:k], bufs.ni[:k], bufs.w[:k], bufs.ns[:k],
                     float(tau.value), int(cst.value))


def _views_floats(x, V, per, shape, name):
    """``x`` = a tensor of shape [V, *shape] or a sequence of V items of ``per`` values -> the V * per host floats."""
    if torch.is_tensor(x):
        if tuple(x.shape) != (V,) + shape:
            raise ValueError(f"{name} must be {list((V,) + shape)}, not {list(x.shape)}")
        return [float(f) for f in x.detach().to("cpu", torch.float32).reshape(-1)]
    items = list(x)
    if len(items) != V:
        raise ValueError(f"{name} must hold one entry per view ({V}), not {len(items)}")
    out = []
    for k, it in enumerate(items):
        if torch.is_tensor(it) and shape and tuple(it.shape) != shape:
            raise ValueError(f"{name}[{k}] must be {list(shape)}, not {list(it.shape)}")
        out += list(_host_floats(it, per, f"{name}[{k}]"))
    return out


def cut_views(nodes, boxes, bounds, taus, viewpoints, planes=None, radius_scales=None, out=None) -> list[CutView]:
    """``cut_view`` for V views in one pass over the nodes: view v is cut at granularity ``taus[v]`` from
    ``viewpoints[v]`` and culled against ``planes[v]`` with ``radius_scales[v]`` (default 1), and ``result[v]`` is bit
    for bit what ``cut_view(..., nested=True)`` returns for it.  ``viewpoints``: [V,3]; ``planes``: [V,5,4] or a
    sequence of [5,4] (``frustum_planes``); all of it is read on the host.  ``bounds`` and ``planes`` are both given or
    both None: without them nothing is culled and every view gets ``expand_to_size`` + ``get_interpolation_weights``.
    The boxes must nest (every hierarchy this package builds or merges).  One call of the library takes 16 views; more
    are processed in groups of 16.  All views share one set of buffers (``out``: a ``CutBuffers``; default: allocated to
    fit): view v's entries start at the sum of the earlier views' counts, each rounded up to 4 entries (16 bytes), and
    the ``CutView``s are slices of them.  Views that do not fit ``out`` raise ``_lib.HgsError`` naming the count."""
    if (bounds is None) != (planes is None):
        raise ValueError("bounds and planes go together: give both or neither")
    cull = bounds is not None
    N, dev, _ = _check_hierarchy(nodes, boxes, bounds, None, cull=False)
    if cull:
        _need(bounds, "bounds", torch.float32, lambda t: t.dim() == 2 and tuple(t.shape) == (N, 4), "[N,4]")
        if bounds.device != dev:
            raise ValueError("nodes, boxes and bounds must live on one device")
    tau = [float(x) for x in (taus.detach().cpu().reshape(-1) if torch.is_tensor(taus) else list(taus))]
    V = len(tau)
    vps = _views_floats(viewpoints, V, 3, (3,), "viewpoints")
    pls = _views_floats(planes, V, 20, (5, 4), "planes") if cull else None
    rss = [1.0] * V if radius_scales is None else _views_floats(radius_scales, V, 1, (), "radius_scales")
    if V == 0:
        return []
    from gaussian_hierarchy._C import _boxes_nested
    if N > 0 and not _boxes_nested(nodes, boxes):
        raise ValueError("cut_views needs a hierarchy whose boxes nest (every child's box inside its parent's): "
                         "these do not -- use cut_view, one view at a time")
    own = out is None
    bufs = CutBuffers(max(N, 1), dev) if own else out
    _check_out(bufs, dev)
    lib = _lib.lib()
    G = _lib.CUT_MAX_VIEWS
    tmp = torch.empty(lib.hgs_lod_cut_views_tmp_bytes(N, min(V, G)), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    floats = lambda v: (C.c_float * len(v))(*v)
    for attempt in range(2):
        names = (bufs.ri, bufs.pi, bufs.ni, bufs.w, bufs.ns)
        cap = min(t.numel() for t in names)
        at, fits, found = 0, True, []                   # `at`: where the next group starts
        for g0 in range(0, V, G):
            g = min(G, V - g0)
            # a group behind one that did not fit is only counted: no room, nothing is written
            room, base = (cap - at, at) if fits and at < cap else (0, 0)
            outs = [C.c_void_p(t.data_ptr() + 4 * base) if t.numel() else None for t in names]
            n, n_all, offs, need = (C.c_int32 * g)(), (C.c_int32 * g)(), (C.c_int32 * g)(), C.c_int64(0)
            rc = lib.hgs_lod_cut_views(p(nodes), p(boxes), p(bounds), N, g, floats(tau[g0:g0 + g]),
                                       floats(vps[3 * g0:3 * (g0 + g)]), floats(pls[20 * g0:20 * (g0 + g)]) if cull else None,
                                       floats(rss[g0:g0 + g]), *outs, room, p(tmp), n, n_all, offs, C.byref(need),
                                       _stream(dev), dev.index or 0)
            if rc != 0 and not need.value > room:
                _lib.check(rc, "hgs_lod_cut_views")
            fits = fits and rc == 0
            found += [(at + int(offs[v]), int(n[v]), int(n_all[v])) for v in range(g)]
            at += sum((int(k) + 3) // 4 * 4 for k in n)
        if fits:
            break
        needed = found[-1][0] + found[-1][1]
        if needed > 2 ** 31 - 1:
            raise _lib.HgsError(f"hgs_lod_cut_views failed: {needed} entries are more than the 2^31 - 1 one set of "
                                f"outputs can index", 1)
        if not own or attempt == 1:
            raise _lib.HgsError(f"hgs_lod_cut_views failed: {needed} entries exceed the output capacity {cap}", 1)
        bufs = CutBuffers(needed, dev)                  # nodes of several rows, or many views: allocate what it takes
    return [CutView(k, k_all, bufs.ri[o:o + k], bufs.pi[o:o + k], bufs.ni[o:o + k], bufs.w[o:o + k], bufs.ns[o:o + k])
            for o, k, k_all in found]
