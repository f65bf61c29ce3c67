"""Gaussian hierarchies for the LOD-cut path (BASELINE.json configs 3 and 5).

The reference builds hierarchies offline with its GaussianHierarchyCreator / Merger tools
(scripts/full_train.py:138-139,188-196,242-250 -- C++ sources absent).  This module defines this
project's own construction rule (``build_hierarchy``, the float64 numpy spec; ``build_hierarchy_gpu``,
the same rule on the device, behind ``python -m hgs.create_hierarchy``): a balanced binary BVH over
Morton-sorted leaves, interior nodes holding a moment-matched merge of their children.  Chunk hierarchies are joined
under one root by ``merge_hierarchies`` (the torch spec) and ``merge_hierarchies_gpu`` (the same rule on the device, one
chunk at a time, behind ``python -m hgs.merge_hierarchies``).  ``align_hierarchy`` (the numpy spec) and ``align_hierarchy_gpu``
(the same rule on the device, behind ``--align`` and ``python -m hgs.align_hierarchy``) re-express every node's rotation
and scales in the frame closest to its parent's, opt-in.  ``trim_hierarchy`` (the numpy spec) and ``trim_hierarchy_gpu``
(the same rule on the device, behind ``python -m hgs.trim_hierarchy``) make a smaller copy: a detail floor, a region, a
node budget; ``trim_to_views`` (the numpy spec, on ``view_reach``) and ``trim_to_views_gpu`` (on the device, behind
``python -m hgs.trim_to_views``) trim to the detail a set of camera positions (``view_regions``) can reach at a
granularity.  ``transform_hierarchy`` (the numpy spec) and ``transform_hierarchy_gpu`` (the same rule on the device, behind
``python -m hgs.transform_hierarchy``) move a hierarchy to another frame by a similarity ``similarity(...)`` builds: means,
rotations, scales, boxes and SH bands follow; ``transform_camera`` moves a camera with it.  ``refit_boxes`` (the numpy
spec) and ``refit_boxes_gpu`` (the same rule on the device, behind ``python -m hgs.refit_hierarchy`` and ``--refit`` on the
transform command) derive every box again from the rows: leaves first, parents as unions of their children.
``prune_hierarchy`` (the numpy spec) and ``prune_hierarchy_gpu`` (the same rule on the device, behind
``python -m hgs.prune_hierarchy``) take leaves out -- boxes, a keep box, an opacity floor, a scale ceiling, a mask --, drop
what dies with them and re-merge only the ancestors that changed.
Layout = DESIGN.md '.hier layout':

  one Gaussian per node, Gaussian index == node index (``start`` = node id)
  nodes int32 [N,7] = depth, parent, start, count_leafs, count_merged, start_children, count_children
  boxes f32 [N,2,4]  = AABB min + extent (max edge), AABB max + 0
Children of a node are contiguous (BFS numbering).
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import time
from dataclasses import dataclass

import numpy as np
import torch


@dataclass
class Hierarchy:
    xyz: torch.Tensor         # [G,3]
    shs: torch.Tensor         # [G,16,3]
    alpha: torch.Tensor       # [G,1] activated opacity
    log_scales: torch.Tensor  # [G,3]
    rots: torch.Tensor        # [G,4]
    nodes: torch.Tensor       # [N,7] int32
    boxes: torch.Tensor       # [N,2,4] float32

    @property
    def num_nodes(self):
        return self.nodes.shape[0]


def _morton(xyz: np.ndarray) -> np.ndarray:
    lo, hi = xyz.min(0), xyz.max(0)
    q = np.clip(((xyz - lo) / np.maximum(hi - lo, 1e-12) * 1023.0), 0, 1023).astype(np.uint64)

    def spread(v):
        v = (v | (v << np.uint64(16))) & np.uint64(0x030000FF)
        v = (v | (v << np.uint64(8))) & np.uint64(0x0300F00F)
        v = (v | (v << np.uint64(4))) & np.uint64(0x030C30C3)
        v = (v | (v << np.uint64(2))) & np.uint64(0x09249249)
        return v
    return spread(q[:, 0]) | (spread(q[:, 1]) << np.uint64(1)) | (spread(q[:, 2]) << np.uint64(2))


def _rot_from_quat(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def _quat_from_rot(R):
    m00, m01, m02 = R[:, 0, 0], R[:, 0, 1], R[:, 0, 2]
    m10, m11, m12 = R[:, 1, 0], R[:, 1, 1], R[:, 1, 2]
    m20, m21, m22 = R[:, 2, 0], R[:, 2, 1], R[:, 2, 2]
    q = np.empty((R.shape[0], 4))
    tr = m00 + m11 + m22
    c0 = tr > 0
    c1 = (~c0) & (m00 >= m11) & (m00 >= m22)
    c2 = (~c0) & (~c1) & (m11 >= m22)
    c3 = ~(c0 | c1 | c2)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(np.maximum(tr + 1.0, 1e-20)) * 2
        q[c0] = np.stack([0.25 * s, (m21 - m12) / s, (m02 - m20) / s, (m10 - m01) / s], 1)[c0]
        s = np.sqrt(np.maximum(1.0 + m00 - m11 - m22, 1e-20)) * 2
        q[c1] = np.stack([(m21 - m12) / s, 0.25 * s, (m01 + m10) / s, (m02 + m20) / s], 1)[c1]
        s = np.sqrt(np.maximum(1.0 + m11 - m00 - m22, 1e-20)) * 2
        q[c2] = np.stack([(m02 - m20) / s, (m01 + m10) / s, 0.25 * s, (m12 + m21) / s], 1)[c2]
        s = np.sqrt(np.maximum(1.0 + m22 - m00 - m11, 1e-20)) * 2
        q[c3] = np.stack([(m10 - m01) / s, (m02 + m20) / s, (m12 + m21) / s, 0.25 * s], 1)[c3]
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def build_hierarchy(scene) -> Hierarchy:
    """scene: hgs.synth.Scene (activated scales / opacities, SH degree-3 storage)."""
    xyz = scene.means3D.double().numpy()
    P = xyz.shape[0]
    assert P >= 1
    order = np.argsort(_morton(xyz), kind="stable")
    # ---- topology: BFS over index ranges of the Morton-sorted leaves ------------------
    lo, hi, depth, parent = [np.array([0])], [np.array([P])], [np.array([0])], [np.array([-1])]
    start_children, count_children = [], []
    first_id = [0]
    next_id = 1
    while True:
        l, h = lo[-1], hi[-1]
        interior = (h - l) > 1
        n_int = int(interior.sum())
        sc = np.zeros(l.shape[0], dtype=np.int64)
        cc = np.where(interior, 2, 0)
        sc[interior] = next_id + 2 * np.arange(n_int)
        start_children.append(sc)
        count_children.append(cc)
        if n_int == 0:
            break
        mid = (l[interior] + h[interior]) // 2
        ids = first_id[-1] + np.nonzero(interior)[0]
        lo.append(np.stack([l[interior], mid], 1).reshape(-1))
        hi.append(np.stack([mid, h[interior]], 1).reshape(-1))
        depth.append(np.full(2 * n_int, len(lo) - 1))
        parent.append(np.repeat(ids, 2))
        first_id.append(next_id)
        next_id += 2 * n_int
    N = next_id
    lo_a, hi_a = np.concatenate(lo), np.concatenate(hi)
    depth_a, parent_a = np.concatenate(depth), np.concatenate(parent)
    sc_a, cc_a = np.concatenate(start_children), np.concatenate(count_children)
    is_leaf = cc_a == 0

    # ---- attributes ---------------------------------------------------------------------
    mu = np.zeros((N, 3)); cov = np.zeros((N, 3, 3)); w = np.zeros(N)
    sh = np.zeros((N, 16, 3)); op = np.zeros(N)
    bmin = np.zeros((N, 3)); bmax = np.zeros((N, 3))
    src = order[lo_a[is_leaf]]
    s_leaf = scene.scales.double().numpy()[src]
    R_leaf = _rot_from_quat(scene.rotations.double().numpy()[src])
    Lm = R_leaf * s_leaf[:, None, :]
    mu[is_leaf] = xyz[src]
    cov[is_leaf] = Lm @ Lm.transpose(0, 2, 1)
    op[is_leaf] = scene.opacities.double().numpy().reshape(-1)[src]
    w[is_leaf] = op[is_leaf] * np.prod(s_leaf, axis=1)
    M = scene.shs.shape[1]
    sh[is_leaf, :M] = scene.shs.double().numpy()[src]
    ext = 3.0 * s_leaf.max(axis=1, keepdims=True)
    bmin[is_leaf] = xyz[src] - ext
    bmax[is_leaf] = xyz[src] + ext
    for lvl in range(len(lo) - 1, -1, -1):                     # bottom-up merge
        a, b = first_id[lvl], first_id[lvl] + lo[lvl].shape[0]
        ids = np.arange(a, b)[~is_leaf[a:b]]
        if ids.size == 0:
            continue
        c0, c1 = sc_a[ids], sc_a[ids] + 1
        ws = np.maximum(w[c0] + w[c1], 1e-30)
        f0, f1 = (w[c0] / ws)[:, None], (w[c1] / ws)[:, None]
        m = f0 * mu[c0] + f1 * mu[c1]
        d0, d1 = mu[c0] - m, mu[c1] - m
        cov[ids] = f0[:, :, None] * (cov[c0] + d0[:, :, None] * d0[:, None, :]) + \
            f1[:, :, None] * (cov[c1] + d1[:, :, None] * d1[:, None, :])
        mu[ids] = m
        sh[ids] = f0[:, :, None] * sh[c0] + f1[:, :, None] * sh[c1]
        op[ids] = np.clip(f0[:, 0] * op[c0] + f1[:, 0] * op[c1], 0.0, 1.0)
        w[ids] = ws
        bmin[ids] = np.minimum(bmin[c0], bmin[c1])
        bmax[ids] = np.maximum(bmax[c0], bmax[c1])
    evals, evecs = np.linalg.eigh(cov)
    evals = np.maximum(evals, 1e-12)
    flip = np.linalg.det(evecs) < 0
    evecs[flip, :, 0] *= -1
    quat = _quat_from_rot(evecs)
    scales = np.sqrt(evals)
    # leaves keep their exact input parametrisation
    quat[is_leaf] = scene.rotations.double().numpy()[src]
    scales[is_leaf] = s_leaf

    nodes = np.stack([depth_a, parent_a, np.arange(N), is_leaf.astype(np.int64), (~is_leaf).astype(np.int64),
                      np.where(is_leaf, 0, sc_a), cc_a], 1).astype(np.int32)
    boxes = np.zeros((N, 2, 4), dtype=np.float32)
    boxes[:, 0, :3] = bmin
    boxes[:, 1, :3] = bmax
    boxes[:, 0, 3] = (boxes[:, 1, :3] - boxes[:, 0, :3]).max(axis=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return Hierarchy(xyz=t(mu), shs=t(sh), alpha=t(op[:, None]), log_scales=t(np.log(scales)), rots=t(quat),
                     nodes=torch.from_numpy(nodes), boxes=torch.from_numpy(boxes))


# ---- what the *_gpu wrappers share ----------------------------------------------------------------------------------------
_ROWS = ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes")      # the order of hgs_hier_view
_ROW_WIDTH = {"xyz": 3, "alpha": 1, "log_scales": 3, "rots": 4, "nodes": 7, "boxes": 8}


def _need_gpu(who, spec_name, spec_kind="numpy spec", device=None):
    """-> (libhgs.so, ``device`` or the current GPU); raises without either: the ``*_gpu`` functions have no CPU fallback."""
    global _lib                 # the binding module, for every helper and wrapper behind this call (not imported at
    from . import _lib          # module level: tests/golden/make_upstream_golden.py loads this file on its own)
    lib = _lib.lib()
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} needs a GPU (there is no CPU fallback; {spec_name} is the {spec_kind})")
    return lib, torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _device_rows(h, names, who, in_place_rows=None):
    """-> the device of ``h.nodes``, after checking that every tensor ``names`` of ``h`` is contiguous, of its dtype (nodes
    int32, the rest float32) and on that device.  ``in_place_rows`` = N (a tool that rewrites ``h``): each also holds at
    least N whole rows, and the message says that ``who`` works in place."""
    dev = h.nodes.device
    why = "" if in_place_rows is None else f" ({who} works in place)"
    for name in names:
        t = getattr(h, name)
        want = torch.int32 if name == "nodes" else torch.float32
        if not (t.is_cuda and t.device == dev and t.dtype == want and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {want} tensor on {dev}{why}")
        if in_place_rows is not None:
            width = _ROW_WIDTH[name]
            if t.numel() % width or t.numel() // width < in_place_rows:
                raise ValueError(f"{name} has {t.numel()} values; at least {in_place_rows} rows of {width} expected")
    return dev


def _hier_view(h, G, N, M):
    return _lib.HierView(G, N, M, 0, h.xyz.data_ptr(), h.shs.data_ptr(), h.alpha.data_ptr(), h.log_scales.data_ptr(),
                         h.rots.data_ptr(), h.nodes.data_ptr(), h.boxes.data_ptr())


def _empty_hierarchy(dev, n, shs_shape, alpha_shape=(1,)) -> Hierarchy:
    """n uninitialised rows and nodes on ``dev``; shs [n, *shs_shape], alpha [n, *alpha_shape]."""
    e = lambda *shape, dtype=torch.float32: torch.empty(n, *shape, dtype=dtype, device=dev)
    return Hierarchy(xyz=e(3), shs=e(*shs_shape), alpha=e(*alpha_shape), log_scales=e(3), rots=e(4),
                     nodes=e(7, dtype=torch.int32), boxes=e(2, 4))


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _device_events:
    """Two device events around the block on the current stream -> the pair.  With ``stats``, a block that ends without
    raising waits for the second event and stores the milliseconds between them in ``stats[key]``."""
    __slots__ = ("stats", "key", "pair")

    def __init__(self, stats=None, key=None):
        self.stats, self.key, self.pair = stats, key, [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def __enter__(self):
        self.pair[0].record()
        return self.pair

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.pair[1].record()
            if self.stats is not None:
                self.pair[1].synchronize()
                self.stats[self.key] = self.pair[0].elapsed_time(self.pair[1])


def _raise_first_bad(checks, first_bad, make_error):
    """A report's ``first_bad`` walked in the order of ``checks``: raises make_error(check, node) at the first offender."""
    for check, node in zip(checks, first_bad):
        if node >= 0:
            raise make_error(check, int(node))


def build_hierarchy_gpu(scene, device=None, align=False) -> Hierarchy:
    """``build_hierarchy`` on the GPU (csrc/hier_build.hip, hgs_hier_build): same input (an hgs.synth.Scene of activated
    rows, M in {1, 4, 9, 16} SH coefficients), same topology, numbering and merge rule, a ``Hierarchy`` of tensors on
    ``device`` (default: the current GPU).  nodes, boxes and the leaf rows of xyz / shs / alpha / rots are bit-exact
    against ``build_hierarchy``; interior rows agree to rounding.  ``align`` (opt-in): run
    ``align_hierarchy_gpu`` on the result.  No CPU fallback: raises without libhgs.so or a GPU."""
    lib, dev = _need_gpu("build_hierarchy_gpu", "build_hierarchy", device=device)
    P = int(scene.means3D.shape[0])
    M = int(scene.shs.shape[1])
    if P < 1:
        raise ValueError("build_hierarchy_gpu needs at least one Gaussian")
    if M not in (1, 4, 9, 16):
        raise ValueError(f"M = {M} SH coefficients; 1, 4, 9 or 16 expected")
    f = lambda t, *shape: t.detach().to(dev, torch.float32).reshape(*shape).contiguous()
    xyz, scales, rots = f(scene.means3D, P, 3), f(scene.scales, P, 3), f(scene.rotations, P, 4)
    opacity, shs = f(scene.opacities, P), f(scene.shs, P, M, 3)
    N = 2 * P - 1
    out = _empty_hierarchy(dev, N, (16, 3))
    tmp = torch.empty(lib.hgs_hier_build_tmp_bytes(P), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(lib.hgs_hier_build(p(xyz), p(scales), p(rots), p(opacity), p(shs), P, M,
                                      *(p(getattr(out, name)) for name in _ROWS), p(tmp), _stream(dev), dev.index or 0),
                   "hgs_hier_build")
    return align_hierarchy_gpu(out) if align else out


def build_hierarchy_on_device(P, cam, device, seed=0, sh_degree=3, s_px=(0.5, 4.0), z_range=(2.0, 20.0)) -> Hierarchy:
    """Scale-test generator (BASELINE config 5: tens of millions of nodes): same topology and layout as
    ``build_hierarchy`` over the same leaf distribution as ``hgs.synth.make_scene``, but built with torch ops on
    ``device`` in float32, and interior nodes are AXIS-ALIGNED moment matches (scales = sqrt of the merged covariance's
    diagonal, identity rotation) instead of eigen-decomposed ones.  2 P - 1 nodes; everything stays on ``device``."""
    import math
    g = torch.Generator(device=device).manual_seed(seed)
    U = lambda *s: torch.rand(*s, generator=g, device=device)
    N_ = lambda *s: torch.randn(*s, generator=g, device=device)
    z = z_range[0] + (z_range[1] - z_range[0]) * U(P)
    xyz = torch.stack([z * cam.tanfovx * (2 * U(P) - 1), z * cam.tanfovy * (2 * U(P) - 1), z], 1)
    fx = cam.image_width / (2.0 * cam.tanfovx)
    spx = torch.exp(math.log(s_px[0]) + (math.log(s_px[1]) - math.log(s_px[0])) * U(P))
    s_leaf = (z * spx / fx)[:, None] * (0.3 + 0.7 * U(P, 3))
    q_leaf = torch.nn.functional.normalize(N_(P, 4), dim=1)
    o_leaf = 0.05 + 0.9 * U(P)
    M = (sh_degree + 1) ** 2
    # Morton order of the leaves
    lo_, hi_ = xyz.min(0).values, xyz.max(0).values
    qi = ((xyz - lo_) / (hi_ - lo_).clamp_min(1e-12) * 1023.0).clamp(0, 1023).long()

    def spread(v):
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        v = (v | (v << 2)) & 0x09249249
        return v
    order = torch.argsort(spread(qi[:, 0]) | (spread(qi[:, 1]) << 1) | (spread(qi[:, 2]) << 2), stable=True)
    del qi
    # ---- topology (BFS over index ranges; children contiguous) ------------------------------------------
    lo, hi = [torch.zeros(1, dtype=torch.int64, device=device)], [torch.full((1,), P, dtype=torch.int64, device=device)]
    parent = [torch.full((1,), -1, dtype=torch.int64, device=device)]
    start_children, first_id, next_id = [], [0], 1
    while True:
        l, h = lo[-1], hi[-1]
        interior = (h - l) > 1
        n_int = int(interior.sum())
        sc = torch.zeros_like(l)
        sc[interior] = next_id + 2 * torch.arange(n_int, device=device)
        start_children.append(sc)
        if n_int == 0:
            break
        mid = (l[interior] + h[interior]) // 2
        ids = first_id[-1] + interior.nonzero().flatten()
        lo.append(torch.stack([l[interior], mid], 1).reshape(-1))
        hi.append(torch.stack([mid, h[interior]], 1).reshape(-1))
        parent.append(ids.repeat_interleave(2))
        first_id.append(next_id)
        next_id += 2 * n_int
    N = next_id
    lo_a = torch.cat(lo)
    sc_a = torch.cat(start_children)
    depth_a = torch.cat([torch.full((t.shape[0],), d, dtype=torch.int64, device=device) for d, t in enumerate(lo)])
    parent_a = torch.cat(parent)
    is_leaf = sc_a == 0
    is_leaf[0] = P == 1
    # ---- attributes -----------------------------------------------------------------------------------------
    f32 = dict(dtype=torch.float32, device=device)
    mu = torch.zeros(N, 3, **f32); var = torch.zeros(N, 3, **f32); w = torch.zeros(N, **f32)
    op = torch.zeros(N, **f32); sh = torch.zeros(N, 16, 3, **f32)
    bmin = torch.zeros(N, 3, **f32); bmax = torch.zeros(N, 3, **f32)
    rots = torch.zeros(N, 4, **f32); rots[:, 0] = 1.0
    leaf_ids = is_leaf.nonzero().flatten()
    src = order[lo_a[leaf_ids]]
    mu[leaf_ids] = xyz[src]
    # axis-aligned second moments of an oriented leaf: diag(R diag(s^2) R^T)
    r, x, y, zq = q_leaf[src].unbind(1)
    R = torch.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - r * zq), 2 * (x * zq + r * y),
                     2 * (x * y + r * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - r * x),
                     2 * (x * zq - r * y), 2 * (y * zq + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    var[leaf_ids] = ((R * R) * (s_leaf[src] ** 2)[:, None, :]).sum(2)
    del R
    op[leaf_ids] = o_leaf[src]
    w[leaf_ids] = o_leaf[src] * s_leaf[src].prod(1)
    sh[leaf_ids, 0] = 0.5 * N_(P, 3)
    if M > 1:
        sh[leaf_ids, 1:M] = 0.05 * N_(P, M - 1, 3)
    ext = 3.0 * s_leaf[src].max(1, keepdim=True).values
    bmin[leaf_ids] = xyz[src] - ext
    bmax[leaf_ids] = xyz[src] + ext
    for lvl in range(len(lo) - 1, -1, -1):
        a, b = first_id[lvl], first_id[lvl] + lo[lvl].shape[0]
        ids = a + (~is_leaf[a:b]).nonzero().flatten()
        if ids.numel() == 0:
            continue
        c0 = sc_a[ids]; c1 = c0 + 1
        ws = (w[c0] + w[c1]).clamp_min(1e-30)
        f0, f1 = (w[c0] / ws)[:, None], (w[c1] / ws)[:, None]
        m = f0 * mu[c0] + f1 * mu[c1]
        var[ids] = f0 * (var[c0] + (mu[c0] - m) ** 2) + f1 * (var[c1] + (mu[c1] - m) ** 2)
        mu[ids] = m
        sh[ids] = f0[:, :, None] * sh[c0] + f1[:, :, None] * sh[c1]
        op[ids] = (f0[:, 0] * op[c0] + f1[:, 0] * op[c1]).clamp(0.0, 1.0)
        w[ids] = ws
        bmin[ids] = torch.minimum(bmin[c0], bmin[c1])
        bmax[ids] = torch.maximum(bmax[c0], bmax[c1])
    scales = var.clamp_min(1e-12).sqrt()
    scales[leaf_ids] = s_leaf[src]
    rots[leaf_ids] = q_leaf[src]
    cc = torch.where(is_leaf, 0, 2)
    nodes = torch.stack([depth_a, parent_a, torch.arange(N, device=device), is_leaf.long(), (~is_leaf).long(),
                         torch.where(is_leaf, 0, sc_a), cc], 1).to(torch.int32).contiguous()
    boxes = torch.zeros(N, 2, 4, **f32)
    boxes[:, 0, :3] = bmin
    boxes[:, 1, :3] = bmax
    boxes[:, 0, 3] = (bmax - bmin).max(1).values
    return Hierarchy(xyz=mu, shs=sh, alpha=op[:, None].contiguous(), log_scales=scales.log(), rots=rots, nodes=nodes,
                     boxes=boxes)


def merge_hierarchies(chunks) -> Hierarchy:
    """Several per-chunk hierarchies under one common root -- the shape the reference's GaussianHierarchyMerger
    produces from its chunks (scripts/full_train.py:240-250; BASELINE config 3 'merged 2-chunk toy hierarchy').
    New numbering: node 0 = the new root, nodes 1..k = the chunks' roots (contiguous children of the new root), then
    every chunk's remaining nodes in their own order, so children stay contiguous and 'Gaussian index == node index'
    still holds.  The new root's Gaussian is the moment-matched merge of the chunk roots (weights alpha * volume) with
    an axis-aligned covariance; its box is the union.  Works on whatever device the chunks live on."""
    k = len(chunks)
    assert k >= 1
    dev = chunks[0].nodes.device
    sizes = [int(c.num_nodes) for c in chunks]
    bases, b = [], 1 + k
    for n in sizes:
        bases.append(b)
        b += n - 1
    N = b

    def remap(c, ids):           # old node id of chunk c -> new id (negative ids stay negative)
        out = torch.where(ids == 0, torch.full_like(ids, 1 + c), ids + (bases[c] - 1))
        return torch.where(ids < 0, ids, out)

    new_of = [remap(c, torch.arange(sizes[c], device=dev, dtype=torch.int64)) for c in range(k)]
    perm = torch.empty(N, dtype=torch.int64, device=dev)         # new id -> row of the concatenated chunk arrays
    offs = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    for c in range(k):
        perm[new_of[c]] = torch.arange(sizes[c], device=dev, dtype=torch.int64) + int(offs[c])
    perm[0] = 0                                                   # placeholder row, overwritten below
    cat = lambda name: torch.cat([getattr(c, name) for c in chunks])[perm].clone()
    xyz, shs, alpha, log_scales, rots = (cat(n) for n in ("xyz", "shs", "alpha", "log_scales", "rots"))
    boxes = cat("boxes")
    nodes = torch.zeros(N, 7, dtype=torch.int32, device=dev)
    for c, ch in enumerate(chunks):
        nd = ch.nodes.to(torch.int64)
        ids = new_of[c]
        row = torch.stack([nd[:, 0] + 1,                                              # one level deeper
                           torch.where(nd[:, 1] < 0, torch.zeros_like(nd[:, 1]), remap(c, nd[:, 1])),
                           ids, nd[:, 3], nd[:, 4],
                           torch.where(nd[:, 6] > 0, remap(c, nd[:, 5]), torch.zeros_like(nd[:, 5])), nd[:, 6]], 1)
        nodes[ids] = row.to(torch.int32)
    nodes[0] = torch.tensor([0, -1, 0, 0, 1, 1, k], dtype=torch.int32, device=dev)
    # the new root's Gaussian and box
    r = torch.arange(1, 1 + k, device=dev)
    sc = log_scales[r].double().exp()
    w = (alpha[r, 0].double() * sc.prod(1)).clamp_min(1e-30)
    f = (w / w.sum())[:, None]
    m = (f * xyz[r].double()).sum(0)
    # axis-aligned second moments of the children: diag(R diag(s^2) R^T) + spread of the means
    q = rots[r].double()
    q = q / q.norm(dim=1, keepdim=True)
    qr, qx, qy, qz = q.unbind(1)
    R = torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qr * qz), 2 * (qx * qz + qr * qy),
                     2 * (qx * qy + qr * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qr * qx),
                     2 * (qx * qz - qr * qy), 2 * (qy * qz + qr * qx), 1 - 2 * (qx * qx + qy * qy)], 1).reshape(-1, 3, 3)
    var = ((R * R) * (sc ** 2)[:, None, :]).sum(2)
    var = (f * (var + (xyz[r].double() - m) ** 2)).sum(0)
    xyz[0] = m.float()
    log_scales[0] = var.clamp_min(1e-12).sqrt().log().float()
    rots[0] = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev)
    shs[0] = (f[:, :, None] * shs[r].double()).sum(0).float()
    alpha[0, 0] = float((f[:, 0] * alpha[r, 0].double()).sum().clamp(0.0, 1.0))
    boxes[0, 0, :3] = boxes[r, 0, :3].min(0).values
    boxes[0, 1, :3] = boxes[r, 1, :3].max(0).values
    boxes[0, 0, 3] = (boxes[0, 1, :3] - boxes[0, 0, :3]).max()
    boxes[0, 1, 3] = 0.0
    return Hierarchy(xyz=xyz, shs=shs, alpha=alpha, log_scales=log_scales, rots=rots, nodes=nodes, boxes=boxes)


HIER_MAGIC = b"HGSHIER1"
HIER_UPSTREAM, HIER_PRIVATE, HIER_UPSTREAM_HALF = 0, 1, 2      # the layouts of include/hgs.h (_lib repeats them)


def read_hier_header(path):
    """-> (G, N, M, layout) of a .hier file from its header and declared sizes, without reading the rows: the three
    layouts ``hgs_hier_load`` accepts (csrc/hier_io.cpp): HGSHIER1 (private, any M), upstream float and upstream half
    (int32 P < 0), the upstream ones only if the file size matches the declared sizes exactly, as the loader requires."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(24)
        if head[:8] == HIER_MAGIC:
            if len(head) < 24:
                raise ValueError(f"{path}: truncated header")
            G, N, M, _ = struct.unpack("<4i", head[8:24])
            if G < 0 or N < 0 or M < 0 or M > 64:
                raise ValueError(f"{path}: corrupt header")
            if size < 24 + G * (12 * M + 44) + N * 60:
                raise ValueError(f"{path}: truncated file (declares G = {G}, N = {N}, M = {M})")
            return G, N, M, HIER_PRIVATE
        bad = ValueError(f"{path} is neither an upstream .hier file (declared sizes do not match the file size) "
                         f"nor an HGSHIER1 file")
        if len(head) < 4:
            raise bad
        P_raw, = struct.unpack("<i", head[:4])
        half = P_raw < 0
        G = -P_raw if half else P_raw
        n_at = 4 + G * (12 + 2 * 56 if half else 236)
        if n_at + 4 > size:
            raise bad
        f.seek(n_at)
        N, = struct.unpack("<i", f.read(4))
        if N < 0 or n_at + 4 + N * 60 != size:
            raise bad
        return G, N, 16, (HIER_UPSTREAM_HALF if half else HIER_UPSTREAM)


class ChunkValidationError(ValueError):
    """A chunk ``merge_hierarchies_gpu`` rejected: ``chunk`` (its path, or ``chunk <index>``), ``check`` (what failed)
    and ``node`` (the first offending node of the chunk, None for the children-count sum)."""

    def __init__(self, chunk, check, node, detail=""):
        at = f"first offending node {node}" if node is not None else detail
        super().__init__(f"{chunk}: not a valid hierarchy: {check} ({at})")
        self.chunk, self.check, self.node = chunk, check, node


# hgs_hier_merge_report.first_bad, in the order they are reported (a bad children range orphans the children it
# should claim: the range is named, not the orphans)
MERGE_CHECKS = ("start != node index or count_leafs + count_merged != 1",
                "children range outside [1, N)",
                "parent outside [0, N) or not claiming the node (node 0: parent != -1)")
MERGE_MAX_NODES = (1 << 31) - 1


def merge_layout(node_counts):
    """-> (bases, N): where chunk c's nodes 1..N_c - 1 start in the merged numbering of ``merge_hierarchies`` (node 0
    the new root, 1..k the chunk roots, then every chunk's other nodes in order), and the merged node count."""
    k = len(node_counts)
    bases, b = [], 1 + k
    for n in node_counts:
        bases.append(b)
        b += int(n) - 1
    return bases, b


def _tensor_sizes(h):
    G, N = int(h.xyz.shape[0]), int(h.nodes.shape[0])
    M = int(h.shs.shape[1]) if h.shs.dim() == 3 else int(h.shs.shape[1]) // 3
    want = {"shs": G * M * 3, "alpha": G, "log_scales": G * 3, "rots": G * 4, "nodes": N * 7, "boxes": N * 8}
    for name, n in want.items():
        if getattr(h, name).numel() != n:
            raise ValueError(f"{name} has {getattr(h, name).numel()} values; {n} expected for G = {G}, N = {N}, M = {M}")
    return G, N, M


def merge_hierarchies_gpu(sources, device=None, stats=None, align=False) -> Hierarchy:
    """``merge_hierarchies`` on the GPU (csrc/hier_merge.hip, hgs_hier_merge_place / hgs_hier_merge_root), applied to
    chunks trimmed to their first N rows: rows at index >= N (a skybox tail, G > N) are dropped.  ``sources``: chunk
    ``Hierarchy``s (host or device tensors) or ``.hier`` paths, in merge order.  The merged tensors are allocated once on
    ``device`` (default: the current GPU); the chunks are placed one at a time, a path loaded, placed and released
    before the next one (host memory holds one chunk, device memory the merged hierarchy and one chunk's nodes).
    nodes, boxes and every non-root row equal ``merge_hierarchies`` on the trimmed chunks bit for bit; the root row
    agrees to float32 rounding.  Each chunk is validated as it is placed: one that fails raises
    ``ChunkValidationError`` naming it, the check and the first offending node.  ``stats`` (a dict, optional) receives
    ``read_s`` (host seconds loading paths) and ``merge_ms`` (device events around the placements and the root).
    ``align`` (opt-in): run ``align_hierarchy_gpu`` on the merged hierarchy once the root is written (``stats`` then
    also receives ``align_ms``).  No CPU fallback: raises without libhgs.so or a GPU."""
    lib, dev = _need_gpu("merge_hierarchies_gpu", "merge_hierarchies", "spec", device)
    sources = list(sources)
    k = len(sources)
    if k < 1:
        raise ValueError("merge_hierarchies_gpu needs at least one chunk")
    is_path = [isinstance(s, (str, os.PathLike)) for s in sources]
    names = [os.fspath(s) if p else f"chunk {c}" for c, (s, p) in enumerate(zip(sources, is_path))]
    sizes = []
    for s, p, name in zip(sources, is_path, names):
        G, N, M = read_hier_header(s)[:3] if p else _tensor_sizes(s)
        if N < 1 or G < N:
            raise ValueError(f"{name}: G = {G} rows, N = {N} nodes; 1 <= N <= G expected")
        sizes.append((G, N, M))
    Ms = {m for _, _, m in sizes}
    if len(Ms) != 1:
        raise ValueError(f"the chunks disagree on the SH coefficients per row: {sorted(Ms)}")
    M = Ms.pop()
    bases, N = merge_layout([n for _, n, _ in sizes])
    if N > MERGE_MAX_NODES:
        raise ValueError(f"the merged hierarchy would have {N} nodes; at most 2^31 - 1")
    out = _empty_hierarchy(dev, N, (M, 3))
    tmp = torch.empty(_lib.HIER_MERGE_TMP_BYTES, dtype=torch.uint8, device=dev)
    merged = _hier_view(out, N, N, M)
    events, read_s = [], 0.0
    with torch.cuda.device(dev):
        stream = _stream(dev)
        for c, (src, path, name) in enumerate(zip(sources, is_path, names)):
            G, n, _ = sizes[c]
            if path:
                from gaussian_hierarchy._C import load_hierarchy
                t0 = time.perf_counter()
                h = Hierarchy(*load_hierarchy(name))
                read_s += time.perf_counter() - t0
                if _tensor_sizes(h) != sizes[c]:
                    raise ValueError(f"{name}: the loaded sizes {_tensor_sizes(h)} differ from the header's {sizes[c]}")
            else:
                h = src

            def arr(t, dtype=torch.float32):      # host tensors stay put (copied H2D in place); another GPU's move here
                t = t.detach()
                if t.is_cuda and t.device != dev:
                    t = t.to(dev)
                return t.to(dtype).contiguous()
            h = Hierarchy(xyz=arr(h.xyz), shs=arr(h.shs), alpha=arr(h.alpha), log_scales=arr(h.log_scales),
                          rots=arr(h.rots), nodes=h.nodes.detach().to(dev, torch.int32).contiguous(), boxes=arr(h.boxes))
            rep, chunk = _lib.HierMergeReport(), _hier_view(h, G, n, M)
            with _device_events() as ev:
                _lib.check(lib.hgs_hier_merge_place(C.byref(chunk), c, k, bases[c], C.byref(merged),
                                                    tmp.data_ptr(), C.byref(rep), stream, dev.index or 0),
                           f"hgs_hier_merge_place ({name})")
            events.append(ev)
            del h
            _raise_first_bad(MERGE_CHECKS, rep.first_bad, lambda check, node: ChunkValidationError(name, check, node))
            if rep.children_sum != n - 1:
                raise ChunkValidationError(name, "children counts do not sum to N - 1", None,
                                           f"they sum to {rep.children_sum}, N = {n}")
        with _device_events() as ev:
            _lib.check(lib.hgs_hier_merge_root(C.byref(merged), k, stream, dev.index or 0), "hgs_hier_merge_root")
        events.append(ev)
    align_stats = {}
    if align:
        align_hierarchy_gpu(out, align_stats)
    if stats is not None:
        events[-1][1].synchronize()
        stats["read_s"] = read_s
        stats["merge_ms"] = sum(a.elapsed_time(b) for a, b in events)
        stats.update(align_stats)
    return out


# ---- rotation alignment: every node's frame re-parametrised to lie close to its parent's -------------------------------
ALIGN_BOUND = (2.0 + 2.0 ** 0.5) / 4.0   # the least |<q_child, q_parent>| (normalised) the best of 24 frames can have
ALIGN_MAX_NODES = (1 << 31) - 1
# hgs_hier_align_report.first_bad, in the order they are reported
ALIGN_CHECKS = ("depth outside [0, 255]",
                "parent outside [0, N) at a node of depth > 0",
                "parent's depth is not the node's depth - 1",
                "more than one node of depth 0")


def align_group():
    """-> (quats float64 [24,4] (w,x,y,z), perms int64 [24,3]): the 24 proper signed permutation matrices M in the
    order of the rule (permutations of (0,1,2) outermost, the signs (1,-1)^3 inside, det(M) > 0 kept), M[perm[k], k] =
    signs[k]: R(q (x) g) = R(q) M has +- column perm[k] of R(q) as its column k.  Element 0 is the identity."""
    import itertools
    quats, perms = [], []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            M = np.zeros((3, 3))
            for k in range(3):
                M[perm[k], k] = signs[k]
            if np.linalg.det(M) > 0:
                quats.append(_quat_from_rot(M[None])[0])
                perms.append(perm)
    return np.array(quats), np.array(perms, dtype=np.int64)


def _quat_mul(a, b):
    """Hamilton product a (x) b, (w,x,y,z), every sum left to right (the order csrc/hier_align.hip repeats)."""
    a0, a1, a2, a3 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    b0, b1, b2, b3 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3,
                     a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                     a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1,
                     a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], -1)


def align_choice(q, qp):
    """The rule at nodes with float32 quaternions ``q`` [n,4] under parents with FINAL quaternions ``qp`` [n,4]:
    -> (j int64 [n], negate bool [n], aligned float32 [n,4]).  Candidates c_j = q (x) g_j and d_j = <c_j, qp> in
    float64, the first j of the largest |d_j|, the sign of d_j folded in (sign(0) = +); j = 0 keeps the input's bits."""
    g, _ = align_group()
    qd, pd = np.asarray(q, dtype=np.float64), np.asarray(qp, dtype=np.float64)
    c = _quat_mul(qd[:, None, :], g[None, :, :])                                    # [n,24,4]
    d = c[..., 0] * pd[:, None, 0] + c[..., 1] * pd[:, None, 1] + c[..., 2] * pd[:, None, 2] + c[..., 3] * pd[:, None, 3]
    j = np.argmax(np.abs(d), axis=1)                                                 # the first maximum
    rows = np.arange(qd.shape[0])
    neg = d[rows, j] < 0
    best = np.where(neg[:, None], -c[rows, j], c[rows, j]).astype(np.float32)
    q32 = np.asarray(q, dtype=np.float32)
    best = np.where((j == 0)[:, None], np.where(neg[:, None], -q32, q32), best)
    return j, neg, best


def align_hierarchy(h: Hierarchy, choice=None) -> Hierarchy:
    """Rotation alignment (the float64 numpy spec; ``align_hierarchy_gpu`` is the same rule on the device): every
    non-root node's (rotation, scales) pair is replaced by the one of its 24 equivalent parametrisations -- the frame's
    axes permuted and negated by a proper signed permutation, the log-scales permuted with them -- whose quaternion
    lies closest to the parent's FINAL quaternion, parents before children (``align_choice``).  The Gaussian a node
    represents does not change; the quaternion norm is kept; the normalised dot with the parent becomes >= ALIGN_BOUND.
    xyz, shs, alpha, nodes, boxes, the root row and rows at index >= N are untouched.  Nodes are levelled by their
    ``depth`` column, so any numbering works (the builder's BFS, the merger's chunks side by side).
    ``choice`` (optional int64 [N] array) receives the chosen group element per node.  -> a new Hierarchy (host)."""
    nodes = h.nodes.cpu().numpy()
    N = nodes.shape[0]
    depth, parent = nodes[:, 0].astype(np.int64), nodes[:, 1].astype(np.int64)
    assert N >= 1 and int((depth == 0).sum()) == 1 and depth.min() >= 0 and depth.max() <= 255
    nonroot = depth > 0
    assert bool(((parent[nonroot] >= 0) & (parent[nonroot] < N)).all())
    assert bool((depth[parent[nonroot]] == depth[nonroot] - 1).all())
    _, perms = align_group()
    rots = h.rots.detach().cpu().numpy().astype(np.float32).copy()
    ls = h.log_scales.detach().cpu().numpy().astype(np.float32).copy()
    if choice is not None:
        choice[:] = 0
    for d in range(1, int(depth.max()) + 1):
        ids = np.nonzero(depth == d)[0]
        j, _, best = align_choice(rots[ids], rots[parent[ids]])
        rots[ids] = best
        ls[ids] = np.take_along_axis(ls[ids], perms[j], axis=1)
        if choice is not None:
            choice[ids] = j
    cp = lambda t: t.detach().cpu().clone()
    return Hierarchy(xyz=cp(h.xyz), shs=cp(h.shs), alpha=cp(h.alpha), log_scales=torch.from_numpy(ls),
                     rots=torch.from_numpy(rots), nodes=cp(h.nodes), boxes=cp(h.boxes))


def alignment_dots(h: Hierarchy):
    """|<q_i, q_parent>| of the normalised quaternions at every node of depth > 0 (float64 numpy [N - 1], node order):
    what the rule maximises; below ALIGN_BOUND the node's frame is more than 62.8 degrees from its parent's."""
    nodes = h.nodes.cpu().numpy()
    N = nodes.shape[0]
    q = h.rots[:N].detach().cpu().numpy().astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    ids = np.nonzero(nodes[:, 0] > 0)[0]
    return np.abs((q[ids] * q[nodes[ids, 1]]).sum(1))


class HierarchyCheckError(ValueError):
    """A hierarchy a tool rejected: ``check`` (what failed) and ``node`` (the first offending node)."""

    def __init__(self, check, node, message):
        super().__init__(message)
        self.check, self.node = check, node


class HierarchyAlignError(HierarchyCheckError):
    """A hierarchy ``align_hierarchy_gpu`` rejected (and left untouched): ``check`` (what failed, one of ALIGN_CHECKS)
    and ``node`` (the first offending node, None when no node has depth 0)."""


def align_hierarchy_gpu(h: Hierarchy, stats=None) -> Hierarchy:
    """``align_hierarchy`` on the GPU (csrc/hier_align.hip, hgs_hier_align), in place: ``h.log_scales`` and ``h.rots``
    (contiguous float32 device tensors of >= N rows; rows behind the N nodes -- a skybox tail -- are not touched) are
    rewritten, nothing else is; -> ``h``.  The choice of frame and the written bits are the spec's (double arithmetic
    in the spec's order).  ``h.nodes`` is validated first (depths in [0, 255], parents in range and one level up, one
    node of depth 0): a hierarchy that fails raises ``HierarchyAlignError`` naming the check and the first offending
    node, and is left untouched.  ``stats`` (a dict, optional) receives ``align_ms`` (device events around the call).
    No CPU fallback: raises without libhgs.so or a GPU."""
    lib, _ = _need_gpu("align_hierarchy_gpu", "align_hierarchy")
    N = int(h.nodes.shape[0])
    if N < 1 or N > ALIGN_MAX_NODES:
        raise ValueError(f"N = {N} nodes; 1 .. 2^31 - 1 expected")
    dev = _device_rows(h, ("nodes", "log_scales", "rots"), "align_hierarchy_gpu", in_place_rows=N)
    tmp = torch.empty(lib.hgs_hier_align_tmp_bytes(N), dtype=torch.uint8, device=dev)
    rep = _lib.HierAlignReport()
    rep.first_bad[:] = [-1] * 4              # (a call that fails its size checks does not fill the report)
    p = _lib.ptr
    with torch.cuda.device(dev), _device_events(stats, "align_ms"):
        rc = lib.hgs_hier_align(p(h.nodes), N, p(h.log_scales), p(h.rots), p(tmp), C.byref(rep), _stream(dev),
                                dev.index or 0)
        if rc != 0:
            msg = (lib.hgs_last_error() or b"?").decode()
            _raise_first_bad(ALIGN_CHECKS, rep.first_bad,
                             lambda check, node: HierarchyAlignError(check, node, f"hgs_hier_align: {msg}"))
            if rc == 1 and "no node of depth 0" in msg:
                raise HierarchyAlignError("no node of depth 0", None, f"hgs_hier_align: {msg}")
            raise _lib.HgsError(f"hgs_hier_align failed (code {rc}): {msg}", rc)
    return h


# ---- trimming: a detail floor, a region, a node budget ------------------------------------------------------------------
# hgs_hier_trim_report.first_bad, in the order they are reported: the merger's three layout checks, then closure
TRIM_CHECKS = MERGE_CHECKS + ("a kept node under a dropped parent (the boxes do not nest, or the extents grow downwards)",)
TRIM_MAX_NODES = (1 << 31) - 1
_FLT_MAX = 3.4028234663852886e38


class HierarchyTrimError(HierarchyCheckError):
    """A hierarchy ``trim_hierarchy`` / ``trim_hierarchy_gpu`` rejected (nothing was written): ``check`` (what failed,
    one of TRIM_CHECKS) and ``node`` (the first offending node)."""


@dataclass
class TrimResult:
    hierarchy: Hierarchy        # the N' kept nodes, in ascending old order
    old_of_new: torch.Tensor    # int32 [N']
    new_of_old: torch.Tensor    # int32 [N], -1 at dropped nodes
    min_extent: float           # the floor that was used (the larger of the given one and the budget's)
    stubs: int                  # kept nodes with children that became leaves
    stub_ids: torch.Tensor      # int32 [stubs]: their NEW indices, ascending

    def exact_for(self, viewpoint, tau) -> bool:
        """Is the cut of ``hierarchy`` from ``viewpoint`` at granularity ``tau`` the original's cut mapped through
        ``new_of_old``, bit for bit?  True iff every stub s has node_size(s, viewpoint) < tau (float32, the operation
        order of csrc/lod_cut.h node_size): the original's cut then stops at s as well."""
        if self.stub_ids.numel() == 0:
            return True
        b = self.hierarchy.boxes.reshape(-1, 2, 4)[self.stub_ids.long()]
        v = torch.as_tensor(viewpoint, dtype=torch.float32).reshape(3).to(b.device)
        mn, mx, ext = b[:, 0, :3], b[:, 1, :3], b[:, 0, 3]
        d = torch.maximum(torch.maximum(mn - v, v - mx), torch.zeros((), dtype=torch.float32, device=b.device))
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        size = torch.where(d2 > 0, ext / d2.sqrt(), torch.full_like(d2, _FLT_MAX))
        return bool((size < torch.tensor(float(np.float32(tau)), dtype=torch.float32, device=b.device)).all())


def _trim_params(min_extent, roi, max_nodes):
    """-> (float32 floor, None or (lo float32 [3], hi float32 [3]), None or int K); NaN and K < 1 refused."""
    e = np.float32(min_extent)
    if np.isnan(e):
        raise ValueError("min_extent is NaN")
    if roi is not None:
        lo, hi = (np.asarray(torch.as_tensor(r).detach().cpu().numpy() if torch.is_tensor(r) else r,
                             dtype=np.float32).reshape(-1) for r in roi)
        if lo.shape != (3,) or hi.shape != (3,) or np.isnan(lo).any() or np.isnan(hi).any():
            raise ValueError("roi is a pair (lo[3], hi[3]) of numbers")
        roi = (lo, hi)
    if max_nodes is not None:
        max_nodes = int(max_nodes)
        if max_nodes < 1:
            raise ValueError(f"max_nodes = {max_nodes}; at least 1 (the root) expected")
    return e, roi, max_nodes


def _trim_test(boxes, e, roi):
    """test(p) at every node (numpy bool [N]): float32 comparisons only."""
    t = boxes[:, 0, 3] >= e
    if roi is not None:
        lo, hi = roi
        t = t & (boxes[:, 0, :3] <= hi[None, :]).all(1) & (boxes[:, 1, :3] >= lo[None, :]).all(1)
    return t


def layout_check_masks(nodes):
    """The merger's three layout checks (csrc/hier_nodes.h node_layout, in numpy) on int32 nodes [N,7] -> the offenders
    of each check, bool [N] x 3: a bad row, a bad children range, a parent that does not claim the node."""
    nd = np.asarray(nodes).astype(np.int64)
    N = nd.shape[0]
    i = np.arange(N)
    parent, start, leafs, merged, sc, cc = nd[:, 1], nd[:, 2], nd[:, 3], nd[:, 4], nd[:, 5], nd[:, 6]
    bad_row = (start != i) | (leafs + merged != 1)
    bad_children = (cc < 0) | ((cc > 0) & ((sc < 1) | (sc + cc > N)))
    in_range = (parent >= 0) & (parent < N)
    ps, pc = sc[np.where(in_range, parent, 0)], cc[np.where(in_range, parent, 0)]
    bad_parent = ~in_range | ~((i >= ps) & (i < ps + pc))
    bad_parent[0] = parent[0] != -1
    return bad_row, bad_children, bad_parent


def trim_layout_checks(nodes):
    """``layout_check_masks`` -> [first offending node or -1] x 3."""
    return [int(np.nonzero(m)[0][0]) if m.any() else -1 for m in layout_check_masks(nodes)]


def trim_budget_extent(nodes, boxes, max_nodes, roi=None):
    """The floor a node budget resolves to (numpy float32): the smallest extent value e among the nodes with children
    (with a region: those meeting it) such that 1 + sum of count_children over {p: test_e(p)} <= max_nodes; nodes of
    equal extent go in together or not at all; +inf if even the root's children do not fit."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 2, 4)
    cc = np.asarray(nodes)[:, 6].astype(np.int64)
    cand = (cc > 0) & _trim_test(boxes, np.float32(-np.inf), roi)      # (a NaN extent never passes a test)
    e, c = boxes[cand, 0, 3], cc[cand]
    if e.size == 0:
        return np.float32(np.inf)
    order = np.argsort(-e, kind="stable")
    e, total = e[order], 1 + np.cumsum(c[order])
    last = np.ones(e.size, dtype=bool)                               # the last node of every run of equal extents
    last[:-1] = e[:-1] != e[1:]
    ok = np.nonzero(last & (total <= int(max_nodes)))[0]
    return np.float32(e[ok[-1]]) if ok.size else np.float32(np.inf)


def trim_hierarchy(h: Hierarchy, min_extent=0.0, roi=None, max_nodes=None) -> TrimResult:
    """Trim a hierarchy to a detail floor, a region and/or a node budget (the numpy spec; ``trim_hierarchy_gpu`` is the
    same rule on the device).  test(p) = extent(p) >= min_extent and, with ``roi`` = (lo[3], hi[3]), box(p) meets the
    closed box: boxes[p,0,a] <= hi[a] and boxes[p,1,a] >= lo[a] on every axis, all in float32.  Node 0 is kept; node
    n > 0 is kept iff test(parent(n)): siblings stay or go together.  ``max_nodes`` = K resolves to a floor first
    (``trim_budget_extent``); the larger of it and ``min_extent`` is used.  The kept nodes are written in ascending old
    order: rows and boxes bit for bit; node records with parent / start / start_children renumbered, depth kept; a kept
    node with children whose own test fails becomes a stub with a leaf's record (1, 0, 0, 0).  Rows at index >= N (a
    skybox tail) are not the function's business: the result has G = N' rows.
    Refused with ``HierarchyTrimError`` (check, first offending node): the merger's three layout checks, and closure --
    a kept node n > 0 whose parent p != 0 is dropped.  -> TrimResult (host tensors)."""
    e, roi, K = _trim_params(min_extent, roi, max_nodes)
    nodes = h.nodes.detach().cpu().numpy().astype(np.int32)
    N = nodes.shape[0]
    G = int(h.xyz.shape[0])
    if N < 1 or G < N or N > TRIM_MAX_NODES:
        raise ValueError(f"G = {G} rows, N = {N} nodes; 1 <= N <= G, N <= 2^31 - 1 expected")
    boxes = h.boxes.detach().cpu().numpy().astype(np.float32).reshape(-1, 2, 4)
    assert boxes.shape[0] == N
    refuse = lambda check, node: HierarchyTrimError(check, node, f"not a hierarchy that can be trimmed: {check} (first "
                                                                 f"offending node {node}); nothing was written")
    _raise_first_bad(TRIM_CHECKS, trim_layout_checks(nodes), refuse)
    if K is not None:
        e = max(e, trim_budget_extent(nodes, boxes, K, roi))
    th, old_of_new, new_of_old, stubs, stub_ids = _trim_by_test(h, nodes, _trim_test(boxes, e, roi), refuse)
    return TrimResult(th, old_of_new, new_of_old, float(e), stubs, stub_ids)


def _trim_by_test(h, nodes, test, refuse):
    """The part of the rule behind test(p) (numpy bool [N]), for ``trim_hierarchy`` and ``trim_to_views``: the keep
    flags, the closure check, both maps, the renumbered records and the copied rows -> (hierarchy, old_of_new,
    new_of_old, stub count, stub_ids) on the host."""
    N = nodes.shape[0]
    parent = nodes[:, 1].astype(np.int64)
    keep = np.ones(N, dtype=bool)
    keep[1:] = test[parent[1:]]
    grand = parent[np.maximum(parent, 0)]
    open_ = keep & (parent > 0) & ~test[np.maximum(grand, 0)]
    if open_.any():
        raise refuse(TRIM_CHECKS[3], int(np.nonzero(open_)[0][0]))
    old = np.nonzero(keep)[0]
    new_of_old = np.full(N, -1, dtype=np.int32)
    new_of_old[old] = np.arange(old.size, dtype=np.int32)
    cc = nodes[:, 6]
    stub = keep & (cc > 0) & ~test
    out = nodes[old].copy()
    out[:, 1] = np.where(old == 0, -1, new_of_old[np.maximum(parent[old], 0)])
    out[:, 2] = np.arange(old.size, dtype=np.int32)
    inner = (cc[old] > 0) & test[old]
    out[inner, 5] = new_of_old[nodes[old[inner], 5]]
    out[stub[old], 3:7] = np.array([1, 0, 0, 0], dtype=np.int32)
    idx = torch.from_numpy(old)
    rows = lambda t: t.detach().cpu()[:N].index_select(0, idx).clone()
    th = Hierarchy(xyz=rows(h.xyz), shs=rows(h.shs), alpha=rows(h.alpha), log_scales=rows(h.log_scales),
                   rots=rows(h.rots), nodes=torch.from_numpy(out), boxes=rows(h.boxes.reshape(-1, 2, 4)))
    return (th, torch.from_numpy(old.astype(np.int32)), torch.from_numpy(new_of_old), int(stub.sum()),
            torch.from_numpy(np.nonzero(stub[old])[0].astype(np.int32)))


def _trim_budget_extent_torch(nodes, boxes, K, roi):
    """``trim_budget_extent`` in torch on the tensors' device (a sort and a cumulative sum) -> numpy float32."""
    cc = nodes[:, 6].long()
    ext = boxes[:, 0, 3]
    cand = (cc > 0) & (ext >= float("-inf"))
    if roi is not None:
        lo, hi = (torch.from_numpy(r).to(boxes.device) for r in roi)
        cand &= (boxes[:, 0, :3] <= hi).all(1) & (boxes[:, 1, :3] >= lo).all(1)
    e, c = ext[cand], cc[cand]
    if e.numel() == 0:
        return np.float32(np.inf)
    e, order = torch.sort(e, descending=True)
    total = 1 + torch.cumsum(c[order], 0)
    last = torch.ones_like(e, dtype=torch.bool)
    last[:-1] = e[:-1] != e[1:]
    ok = (last & (total <= K)).nonzero().flatten()
    return np.float32(e[ok[-1]].item()) if ok.numel() else np.float32(np.inf)


def trim_hierarchy_gpu(h: Hierarchy, min_extent=0.0, roi=None, max_nodes=None, stats=None) -> TrimResult:
    """``trim_hierarchy`` on the GPU (csrc/hier_trim.hip: hgs_hier_trim_plan, then N' rows are allocated, then
    hgs_hier_trim_apply).  ``h``: contiguous device tensors (float32 rows of G >= N, int32 nodes [N,7], boxes [N,2,4]);
    it is not modified, and rows behind the N nodes are not read.  Every output tensor, both maps, N' and the stub
    count equal the spec's bit for bit.  A node budget is resolved with torch on the device first.  A hierarchy that
    fails a check raises ``HierarchyTrimError`` naming the check and the first offending node; nothing has been
    allocated or written then.  ``stats`` (a dict, optional) receives ``trim_ms`` (device events around plan, the
    allocation and apply) and its two parts ``plan_ms`` (plan, its host wait and the allocation) and ``apply_ms``.
    No CPU fallback: raises without libhgs.so or a GPU."""
    lib, _ = _need_gpu("trim_hierarchy_gpu", "trim_hierarchy")
    e, roi, K = _trim_params(min_extent, roi, max_nodes)
    G, N, M = _tensor_sizes(h)
    if N < 1 or G < N or N > TRIM_MAX_NODES:
        raise ValueError(f"G = {G} rows, N = {N} nodes; 1 <= N <= G, N <= 2^31 - 1 expected")
    dev = _device_rows(h, _ROWS, "trim_hierarchy_gpu")
    boxes = h.boxes.reshape(-1, 2, 4)
    if K is not None:
        e = max(e, _trim_budget_extent_torch(h.nodes, boxes, K, roi))
    with torch.cuda.device(dev), _device_events(stats, "trim_ms") as ev:
        out, old_of_new, new_of_old, rep, mid = _plan_and_apply(lib, h, (G, N, M), dev, e, roi)
    if stats is not None:
        stats["plan_ms"], stats["apply_ms"] = ev[0].elapsed_time(mid), mid.elapsed_time(ev[1])
    return TrimResult(out, old_of_new, new_of_old, float(e), int(rep.stubs), _stub_ids(h, out, old_of_new))


def _plan_and_apply(lib, h, sizes, dev, e, roi, key=None, key_floor=0.0):
    """On the current stream of ``dev``: hgs_hier_trim_plan (with ``key``, a device float32 [N]: hgs_hier_trim_plan_keyed
    at ``key_floor``), the allocation of the N' rows, hgs_hier_trim_apply -> (hierarchy, old_of_new, new_of_old, the
    plan's report, the device event recorded between the allocation and apply).  A failed check raises
    ``HierarchyTrimError`` before anything is allocated."""
    G, N, M = sizes
    args = _lib.HierTrimArgs(float(e), 0 if roi is None else 1)
    if roi is not None:
        args.roi_lo[:], args.roi_hi[:] = [float(x) for x in roi[0]], [float(x) for x in roi[1]]
    p = lambda t: t.data_ptr()
    tmp = torch.empty(lib.hgs_hier_trim_tmp_bytes(N), dtype=torch.uint8, device=dev)
    rep = _lib.HierTrimReport()
    rep.first_bad[:] = [-1] * 4              # (a call that fails its size checks does not fill the report)
    vin = _hier_view(h, G, N, M)
    stream = _stream(dev)
    if key is None:
        name = "hgs_hier_trim_plan"
        rc = lib.hgs_hier_trim_plan(C.byref(vin), C.byref(args), p(tmp), C.byref(rep), stream, dev.index or 0)
    else:
        name = "hgs_hier_trim_plan_keyed"
        rc = lib.hgs_hier_trim_plan_keyed(C.byref(vin), C.byref(args), p(key), float(key_floor), p(tmp), C.byref(rep),
                                          stream, dev.index or 0)
    if rc != 0:
        msg = (lib.hgs_last_error() or b"?").decode()
        _raise_first_bad(TRIM_CHECKS, rep.first_bad,
                         lambda check, node: HierarchyTrimError(check, node, f"{name}: {msg}"))
        raise _lib.HgsError(f"{name} failed (code {rc}): {msg}", rc)
    n = int(rep.kept)
    out = _empty_hierarchy(dev, n, h.shs.shape[1:], h.alpha.shape[1:])
    old_of_new, new_of_old = (torch.empty(m, dtype=torch.int32, device=dev) for m in (n, N))
    mid = torch.cuda.Event(enable_timing=True)
    mid.record()
    _lib.check(lib.hgs_hier_trim_apply(C.byref(vin), C.byref(_hier_view(out, n, n, M)), p(tmp), p(old_of_new),
                                       p(new_of_old), stream, dev.index or 0), "hgs_hier_trim_apply")
    return out, old_of_new, new_of_old, rep, mid


def _stub_ids(h, out, old_of_new):
    """New indices of the stubs, ascending (int32, on the device): nodes with children that came out as leaves."""
    return ((h.nodes[:, 6][old_of_new.long()] > 0) & (out.nodes[:, 6] == 0)).nonzero().flatten().to(torch.int32)


# ---- trimming to the detail a set of views can reach ------------------------------------------------------------------------
REACH_MAX_REGIONS = 1 << 24
REACH_SLAB = 256            # kReachSlab of csrc/hier_reach.hip: the unit a split of the region range is made of
_REACH_SPEC_PAIRS = 1 << 22   # (node, region) pairs per chunk of the numpy spec


def _check_regions(lo, hi, names=None):
    """(lo, hi) float32 [C,3], finite, lo <= hi, C >= 1, or a ValueError naming the entry."""
    lo, hi = np.ascontiguousarray(lo, dtype=np.float32), np.ascontiguousarray(hi, dtype=np.float32)
    if lo.ndim != 2 or lo.shape[1] != 3 or lo.shape != hi.shape:
        raise ValueError(f"view regions are a pair (lo [C,3], hi [C,3]); got {lo.shape} and {hi.shape}")
    C_ = lo.shape[0]
    if C_ < 1 or C_ > REACH_MAX_REGIONS:
        raise ValueError(f"{C_} view regions; 1 .. 2^24 expected (an empty view set reaches nothing)")
    bad = ~(np.isfinite(lo).all(1) & np.isfinite(hi).all(1)) | (lo > hi).any(1)
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        what = f"view region {k}" if names is None else names[k]
        why = "lo > hi on an axis" if np.isfinite(lo[k]).all() and np.isfinite(hi[k]).all() else "not finite"
        raise ValueError(f"{what}: {why} (lo = {lo[k].tolist()}, hi = {hi[k].tolist()})")
    return lo, hi


def view_regions(points=None, boxes=None, pad=0.0):
    """A view set: C >= 1 closed boxes of camera positions -> (lo, hi), float32 [C,3] each.  ``points`` [P,3] become the
    boxes [fl32(p - pad), fl32(p + pad)] (``pad`` = 0: the position itself); ``boxes`` [B,2,3] or [B,6] (lo.xyz, hi.xyz)
    are taken as they are, behind the points.  Refused with a ValueError naming the entry: NaN, infinity, lo > hi,
    pad < 0 (or NaN), an empty set."""
    pad = float(pad)
    if not pad >= 0.0 or pad == float("inf"):
        raise ValueError(f"pad = {pad}; a finite number >= 0 expected")
    as64 = lambda a: np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64)
    lo, hi, names = [], [], []
    with np.errstate(over="ignore"):             # (a number too large for float32 becomes infinity and is refused)
        if points is not None:
            pts = as64(points).reshape(-1, 3)
            lo.append((pts - pad).astype(np.float32))
            hi.append((pts + pad).astype(np.float32))
            names += [f"view point {k}" for k in range(pts.shape[0])]
        if boxes is not None:
            bx = as64(boxes).reshape(-1, 6).astype(np.float32)
            lo.append(bx[:, :3])
            hi.append(bx[:, 3:])
            names += [f"view box {k}" for k in range(bx.shape[0])]
    if not names:
        raise ValueError("an empty view set: no view point and no view box")
    return _check_regions(np.concatenate(lo), np.concatenate(hi), names)


def _reach_d2(boxes, lo, hi):
    """d2(p, c), float32 [N, c]: squared distance from box p to region c, every operation float32 in the device's order."""
    mn, mx = boxes[:, None, 0, :3], boxes[:, None, 1, :3]
    d = np.fmax(np.fmax(mn - hi[None], lo[None] - mx), np.float32(0))
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _reach_of(ext, d2):
    return np.where(d2 > 0, ext / np.sqrt(d2), np.float32(_FLT_MAX)).astype(np.float32)


def view_reach(h: Hierarchy, regions) -> np.ndarray:
    """The view reach of every node, leaves included (the numpy spec of csrc/hier_reach.hip) -> float32 [N]:
    D2(p) = min over the regions c of d2(p, c), reach(p) = D2 > 0 ? extent(p) / sqrt(D2) : FLT_MAX -- ``node_size`` of
    the cut with the viewpoint widened to a box, so no viewpoint inside any region sees p at a larger size.  fmax / fmin
    as on the device: d2 is never NaN.  Walks the regions in chunks: memory stays O(N)."""
    lo, hi = _check_regions(*regions)
    boxes = np.ascontiguousarray(h.boxes.detach().cpu().numpy(), dtype=np.float32).reshape(-1, 2, 4)
    N = boxes.shape[0]
    step = max(1, _REACH_SPEC_PAIRS // max(N, 1))
    best = np.full(N, np.inf, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for c0 in range(0, lo.shape[0], step):
            best = np.fmin(best, _reach_d2(boxes, lo[c0:c0 + step], hi[c0:c0 + step]).min(1))
        return _reach_of(boxes[:, 0, 3], best)


def view_reach_gpu(h: Hierarchy, regions, stats=None) -> torch.Tensor:
    """``view_reach`` on the GPU (csrc/hier_reach.hip, hgs_hier_reach) -> a device float32 [N], the spec's bits.
    ``h.boxes``: a contiguous float32 device tensor [N,2,4]; nothing else of ``h`` is read.  Asynchronous on the current
    stream unless ``stats`` (a dict) is given: it receives ``reach_ms`` (device events around the call).  No CPU
    fallback: raises without libhgs.so or a GPU."""
    lib, _ = _need_gpu("view_reach_gpu", "view_reach")
    lo, hi = _check_regions(*regions)
    dev = _device_rows(h, ("boxes",), "view_reach_gpu")
    N = h.boxes.numel() // 8
    if N < 1 or N > TRIM_MAX_NODES:
        raise ValueError(f"N = {N} nodes; 1 .. 2^31 - 1 expected")
    with torch.cuda.device(dev), _device_events(stats, "reach_ms"):
        return _reach_on_device(lib, h.boxes, N, lo, hi, dev)


def _reach_on_device(lib, boxes, N, lo, hi, dev):
    C_ = lo.shape[0]
    regions = torch.from_numpy(np.concatenate([lo, hi], axis=1)).to(dev)          # [C,6]
    reach = torch.empty(N, dtype=torch.float32, device=dev)
    tmp = torch.empty(lib.hgs_hier_reach_tmp_bytes(N, C_), dtype=torch.uint8, device=dev)
    _lib.check(lib.hgs_hier_reach(boxes.data_ptr(), N, regions.data_ptr(), C_, reach.data_ptr(), tmp.data_ptr(),
                                  _stream(dev), dev.index or 0), "hgs_hier_reach")
    return reach


@dataclass
class ViewTrimResult(TrimResult):
    tau: float                  # the granularity that was used (float32; the larger of the given one and the budget's)
    regions: tuple              # (lo, hi), numpy float32 [C,3] each

    def covers(self, viewpoint, tau) -> bool:
        """Does the contract hold for this view: ``viewpoint`` (rounded to float32) lies in one of the closed regions
        and ``tau`` >= the granularity used?  Then ``exact_for(viewpoint, tau)`` is true and the cut of ``hierarchy`` is
        the original's mapped through ``new_of_old``."""
        v = np.asarray(viewpoint.detach().cpu().numpy() if torch.is_tensor(viewpoint) else viewpoint,
                       dtype=np.float32).reshape(3)
        lo, hi = self.regions
        return bool(((lo <= v) & (v <= hi)).all(1).any() and np.float32(tau) >= np.float32(self.tau))


def _view_tau(tau):
    t = np.float32(tau)
    if np.isnan(t):
        raise ValueError("tau is NaN")
    return t


def view_budget_tau(nodes, boxes, reach, max_nodes, min_extent=0.0, roi=None):
    """The granularity a node budget resolves to under a view set (numpy float32): the smallest reach value t among the
    nodes with children that pass the extent and region tests such that 1 + sum of count_children over {p: reach(p)
    >= t} <= max_nodes; nodes of equal reach go in together or not at all; +inf (the root alone: FLT_MAX < inf) if even
    the first run does not fit."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 2, 4)
    reach = np.asarray(reach, dtype=np.float32)
    cc = np.asarray(nodes)[:, 6].astype(np.int64)
    cand = (cc > 0) & _trim_test(boxes, np.float32(min_extent), roi) & (reach == reach)   # (a NaN never passes a test)
    r, c = reach[cand], cc[cand]
    if r.size == 0:
        return np.float32(np.inf)
    order = np.argsort(-r, kind="stable")
    r, total = r[order], 1 + np.cumsum(c[order])
    last = np.ones(r.size, dtype=bool)
    last[:-1] = r[:-1] != r[1:]
    ok = np.nonzero(last & (total <= int(max_nodes)))[0]
    return np.float32(r[ok[-1]]) if ok.size else np.float32(np.inf)


def _view_budget_tau_torch(nodes, boxes, reach, K, e, roi):
    """``view_budget_tau`` in torch on the tensors' device -> numpy float32."""
    cc = nodes[:, 6].long()
    cand = (cc > 0) & (boxes[:, 0, 3] >= float(e)) & (reach == reach)
    if roi is not None:
        lo, hi = (torch.from_numpy(r).to(boxes.device) for r in roi)
        cand &= (boxes[:, 0, :3] <= hi).all(1) & (boxes[:, 1, :3] >= lo).all(1)
    r, c = reach[cand], cc[cand]
    if r.numel() == 0:
        return np.float32(np.inf)
    r, order = torch.sort(r, descending=True, stable=True)
    total = 1 + torch.cumsum(c[order], 0)
    last = torch.ones_like(r, dtype=torch.bool)
    last[:-1] = r[:-1] != r[1:]
    ok = (last & (total <= K)).nonzero().flatten()
    return np.float32(r[ok[-1]].item()) if ok.numel() else np.float32(np.inf)


_VIEW_HINT = "hgs.refit_hierarchy makes the boxes nest"


def trim_to_views(h: Hierarchy, regions, tau, min_extent=0.0, roi=None, max_nodes=None) -> ViewTrimResult:
    """Trim a hierarchy to the detail a view set can reach at granularity ``tau`` (the numpy spec;
    ``trim_to_views_gpu`` is the same rule on the device).  ``regions``: ``view_regions(...)``.  test(p) = reach(p) >=
    tau (``view_reach``) and extent(p) >= min_extent and, with ``roi``, box(p) meets it; the rest is ``trim_hierarchy``'s
    rule word for word: node 0 is kept, node n > 0 iff test(parent(n)), stubs, renumbering, the four checks (closure
    fails where the boxes do not nest: ``hgs.refit_hierarchy`` mends that).  ``max_nodes`` = K resolves to a
    granularity first (``view_budget_tau``); the larger of it and ``tau`` is used, and at most K nodes stay.
    The contract: for every float32 viewpoint v inside a region (borders included) and every tau' >= result.tau,
    ``result.exact_for(v, tau')`` holds: the cut, its weights and an LOD render of the result are the original's mapped
    through ``new_of_old``.  Elsewhere stubs stand in at weight 1, as under ``trim_hierarchy``.  -> ViewTrimResult (host
    tensors)."""
    lo, hi = _check_regions(*regions)
    t = _view_tau(tau)
    e, roi, K = _trim_params(min_extent, roi, max_nodes)
    nodes = h.nodes.detach().cpu().numpy().astype(np.int32)
    N = nodes.shape[0]
    G = int(h.xyz.shape[0])
    if N < 1 or G < N or N > TRIM_MAX_NODES:
        raise ValueError(f"G = {G} rows, N = {N} nodes; 1 <= N <= G, N <= 2^31 - 1 expected")
    boxes = h.boxes.detach().cpu().numpy().astype(np.float32).reshape(-1, 2, 4)
    assert boxes.shape[0] == N
    refuse = lambda check, node: HierarchyTrimError(check, node, f"not a hierarchy that can be trimmed to views: {check} "
                                                                 f"(first offending node {node}; {_VIEW_HINT}); nothing "
                                                                 f"was written")
    _raise_first_bad(TRIM_CHECKS, trim_layout_checks(nodes), refuse)
    reach = view_reach(h, (lo, hi))
    if K is not None:
        t = max(t, view_budget_tau(nodes, boxes, reach, K, e, roi))
    test = _trim_test(boxes, e, roi) & (reach >= t)
    th, old_of_new, new_of_old, stubs, stub_ids = _trim_by_test(h, nodes, test, refuse)
    return ViewTrimResult(th, old_of_new, new_of_old, float(e), stubs, stub_ids, float(t), (lo, hi))


def trim_to_views_gpu(h: Hierarchy, regions, tau, min_extent=0.0, roi=None, max_nodes=None,
                      stats=None) -> ViewTrimResult:
    """``trim_to_views`` on the GPU (csrc/hier_reach.hip: hgs_hier_reach; csrc/hier_trim.hip: hgs_hier_trim_plan_keyed on
    the reach, then N' rows are allocated, then hgs_hier_trim_apply).  ``h`` as for ``trim_hierarchy_gpu``; it is not
    modified.  Every output tensor, both maps, N', the stub count and tau equal the spec's bit for bit.  A node budget
    is resolved with torch on the device, behind the reach pass.  A hierarchy that fails a check raises
    ``HierarchyTrimError``; nothing has been allocated or written then.  ``stats`` (a dict, optional) receives
    ``trim_ms`` (device events around everything) and its parts ``reach_ms``, ``plan_ms`` (the budget, plan, its host
    wait and the allocation) and ``apply_ms``.  No CPU fallback: raises without libhgs.so or a GPU."""
    lib, _ = _need_gpu("trim_to_views_gpu", "trim_to_views")
    lo, hi = _check_regions(*regions)
    t = _view_tau(tau)
    e, roi, K = _trim_params(min_extent, roi, max_nodes)
    G, N, M = _tensor_sizes(h)
    if N < 1 or G < N or N > TRIM_MAX_NODES:
        raise ValueError(f"G = {G} rows, N = {N} nodes; 1 <= N <= G, N <= 2^31 - 1 expected")
    dev = _device_rows(h, _ROWS, "trim_to_views_gpu")
    boxes = h.boxes.reshape(-1, 2, 4)
    with torch.cuda.device(dev), _device_events(stats, "trim_ms") as ev:
        reach = _reach_on_device(lib, h.boxes, N, lo, hi, dev)
        reached = torch.cuda.Event(enable_timing=True)
        reached.record()
        if K is not None:
            t = max(t, _view_budget_tau_torch(h.nodes, boxes, reach, K, e, roi))
        out, old_of_new, new_of_old, rep, mid = _plan_and_apply(lib, h, (G, N, M), dev, e, roi, reach, t)
    if stats is not None:
        stats["reach_ms"], stats["plan_ms"] = ev[0].elapsed_time(reached), reached.elapsed_time(mid)
        stats["apply_ms"] = mid.elapsed_time(ev[1])
    return ViewTrimResult(out, old_of_new, new_of_old, float(e), int(rep.stubs), _stub_ids(h, out, old_of_new),
                          float(t), (lo, hi))

# ---- similarity transform: x' = s R x + t, rotations, scales, boxes and SH bands following -------------------------------
TRANSFORM_MAX_NODES = (1 << 31) - 1
TRANSFORM_SH_WIDTHS = (1, 4, 9, 16)
_SH_C1 = 0.4886025119029199
_SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
          1.445305721320277, -0.5900435899266435)


def sh_band_basis(d):
    """The basis polynomials of bands 1, 2, 3 (the renderer's, with their signs and constants: a colour is
    sum_m c_m b_m(d)) at unit directions d float64 [n,3] -> (b1 [n,3], b2 [n,5], b3 [n,7]).  csrc/abi.cpp repeats it
    for the consistency check of hgs_hier_transform."""
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    b1 = np.stack([-_SH_C1 * y, _SH_C1 * z, -_SH_C1 * x], 1)
    b2 = np.stack([_SH_C2[0] * xy, _SH_C2[1] * yz, _SH_C2[2] * (2.0 * zz - xx - yy), _SH_C2[3] * xz,
                   _SH_C2[4] * (xx - yy)], 1)
    b3 = np.stack([_SH_C3[0] * y * (3 * xx - yy), _SH_C3[1] * xy * z, _SH_C3[2] * y * (4 * zz - xx - yy),
                   _SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), _SH_C3[4] * x * (4 * zz - xx - yy),
                   _SH_C3[5] * z * (xx - yy), _SH_C3[6] * x * (xx - 3 * yy)], 1)
    return b1, b2, b3


def fibonacci_sphere(n=64):
    """n fixed unit directions (float64 [n,3]): z_i = 1 - (2 i + 1) / n, longitude i times the golden angle."""
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def sh_rotation_blocks(R):
    """(D1 [3,3], D2 [5,5], D3 [7,7]) float64 with c' = D_l c the band-l coefficients of the rotated function:
    c' . b_l(d') = c . b_l(R^T d') for every direction d'.  D_l = lstsq(B_l(d), B_l(R^T d)) over the 64 directions of
    ``fibonacci_sphere`` (the bands are rotation invariant, so the fit is exact up to rounding); entries within 1e-13
    of -1, 0 or 1 are set to that value, so the identity and the signed permutations that give such blocks are exact."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    d = fibonacci_sphere(64)
    out = []
    for B, Br in zip(sh_band_basis(d), sh_band_basis(d @ R)):        # rows of d @ R are R^T d
        D = np.linalg.lstsq(B, Br, rcond=None)[0]
        for v in (-1.0, 0.0, 1.0):
            D[np.abs(D - v) < 1e-13] = v
        out.append(D)
    return tuple(out)


@dataclass
class Similarity:
    """x' = s R x + t with everything a transform of a hierarchy needs, float64 (``similarity`` builds it):
    R [3,3] proper rotation, q_R [4] its quaternion (w,x,y,z), s > 0, log_s = log(s), t [3], and the SH blocks
    D1 [3,3], D2 [5,5], D3 [7,7] of ``sh_rotation_blocks``.  The device consumes this block as it is."""
    R: np.ndarray
    q_R: np.ndarray
    s: float
    log_s: float
    t: np.ndarray
    D1: np.ndarray
    D2: np.ndarray
    D3: np.ndarray

    def inverse(self) -> "Similarity":
        """x = R^T (x' - t) / s."""
        Ri = self.R.T.copy()
        si = 1.0 / self.s
        return similarity(R=Ri, scale=si, translate=-(si * (Ri @ self.t)))

    def compose(self, other: "Similarity") -> "Similarity":
        """The map x -> self(other(x)): ``other`` is applied first."""
        return similarity(R=self.R @ other.R, scale=self.s * other.s, translate=self.s * (self.R @ other.t) + self.t)

    def apply(self, x):
        """s R x + t on points float64 [...,3] (numpy)."""
        return self.s * (np.asarray(x, dtype=np.float64) @ self.R.T) + self.t

    def matrix(self):
        """The 4x4 row-vector matrix S: [x', 1] = [x, 1] S (float64)."""
        S = np.eye(4)
        S[:3, :3] = self.s * self.R.T
        S[3, :3] = self.t
        return S


def similarity(R=None, quat=None, scale=1.0, translate=(0.0, 0.0, 0.0)) -> Similarity:
    """The parameter block of x' = s R x + t, built on the host in float64.  ``R`` [3,3] (kept as given; refused unless
    |R R^T - I| <= 1e-9 and det R > 0: no mirrors) or ``quat`` (w,x,y,z), normalised here; neither: the identity
    rotation.  ``scale`` finite and > 0, ``translate`` finite."""
    if R is not None and quat is not None:
        raise ValueError("give R or quat, not both")
    if quat is not None:
        q = np.asarray(quat, dtype=np.float64).reshape(-1)
        n = float(np.linalg.norm(q)) if q.shape == (4,) else 0.0
        if not (np.isfinite(n) and n > 0.0):
            raise ValueError("quat is four finite numbers (w,x,y,z), not all zero")
        R = _rot_from_quat((q / n)[None])[0]
    R = np.eye(3) if R is None else np.array(R, dtype=np.float64)
    if R.shape != (3, 3) or not np.isfinite(R).all() or np.abs(R @ R.T - np.eye(3)).max() > 1e-9:
        raise ValueError("R is not orthonormal (|R R^T - I| > 1e-9): shear and non-uniform scale are not similarities")
    if np.linalg.det(R) <= 0:
        raise ValueError("det R < 0: a mirror, not a rotation")
    s = float(scale)
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError(f"scale = {s}; a finite number > 0 expected")
    t = np.asarray(translate, dtype=np.float64).reshape(-1)
    if t.shape != (3,) or not np.isfinite(t).all():
        raise ValueError("translate is three finite numbers")
    D1, D2, D3 = sh_rotation_blocks(R)
    return Similarity(R=R, q_R=_quat_from_rot(R[None])[0], s=s, log_s=float(np.log(s)), t=t.copy(), D1=D1, D2=D2, D3=D3)


def check_similarity(sim: Similarity):
    """The checks hgs_hier_transform makes on its parameter block, on the host (ValueError names the first that fails):
    s, t finite and s > 0; log_s = log(s) to 1e-12; |R R^T - I| <= 1e-9, det R > 0; q_R reproduces R to 1e-9; every D_l
    orthogonal to 1e-9 and D_l^T b_l(d) = b_l(R^T d) to 1e-9 at the 16 directions of ``fibonacci_sphere(16)``."""
    R, t = np.asarray(sim.R, dtype=np.float64).reshape(3, 3), np.asarray(sim.t, dtype=np.float64).reshape(-1)
    if not (np.isfinite(sim.s) and np.isfinite(sim.log_s) and t.shape == (3,) and np.isfinite(t).all() and sim.s > 0):
        raise ValueError("bad transform: s and t must be finite and s > 0")
    if not abs(sim.log_s - np.log(sim.s)) <= 1e-12:
        raise ValueError("bad transform: log_s is not log(s)")
    if not np.abs(R @ R.T - np.eye(3)).max() <= 1e-9:
        raise ValueError("bad transform: R is not orthonormal (|R R^T - I| > 1e-9)")
    if not np.linalg.det(R) > 0:
        raise ValueError("bad transform: det R < 0 (a mirror)")
    if not np.abs(_rot_from_quat(np.asarray(sim.q_R, dtype=np.float64).reshape(1, 4))[0] - R).max() <= 1e-9:
        raise ValueError("bad transform: q does not reproduce R")
    d = fibonacci_sphere(16)
    for l, D, b, br in zip((1, 2, 3), (sim.D1, sim.D2, sim.D3), sh_band_basis(d), sh_band_basis(d @ R)):
        D = np.asarray(D, dtype=np.float64)
        if D.shape != (2 * l + 1, 2 * l + 1) or not np.abs(D @ D.T - np.eye(2 * l + 1)).max() <= 1e-9:
            raise ValueError(f"bad transform: D{l} is not orthogonal")
        if not np.abs(b @ D - br).max() <= 1e-9:
            raise ValueError(f"bad transform: D{l} is not the SH block of R")


def _transform_sh_width(shs):
    M = int(shs.shape[1]) if shs.dim() == 3 else int(shs.shape[1]) // 3
    if M not in TRANSFORM_SH_WIDTHS:
        raise ValueError(f"M = {M} SH coefficients per row; whole bands only: one of {TRANSFORM_SH_WIDTHS}")
    return M


def transform_rows(sim: Similarity, xyz, shs, log_scales, rots, round32=True):
    """The row rule on numpy arrays (xyz [G,3], shs [G,M,3], log_scales [G,3], rots [G,4]): every product and sum in
    float64, every sum left to right, rounded once to float32 (``round32=False``: left in float64).
    xyz'_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) s + t_a; rots' = q_R (x) q (Hamilton, norms kept); log_scales' =
    log_scales + log s; SH band 0 keeps its bits, band l: c'_{m,ch} = sum_m' D_l[m][m'] c_{m',ch}."""
    R, t = sim.R, sim.t
    x = np.asarray(xyz, dtype=np.float64)
    out_x = np.stack([((R[a, 0] * x[:, 0] + R[a, 1] * x[:, 1]) + R[a, 2] * x[:, 2]) * sim.s + t[a] for a in range(3)], 1)
    out_q = _quat_mul(sim.q_R[None, :], np.asarray(rots, dtype=np.float64))
    out_ls = np.asarray(log_scales, dtype=np.float64) + sim.log_s
    c = np.asarray(shs)
    out_c = c.astype(np.float32 if round32 else np.float64)           # band 0: the input's bits
    cd = c.astype(np.float64)
    for l, D in ((1, sim.D1), (2, sim.D2), (3, sim.D3)):
        o, n = l * l, 2 * l + 1
        if c.shape[1] < o + n:
            break
        for m in range(n):
            acc = D[m, 0] * cd[:, o, :]
            for k in range(1, n):
                acc = acc + D[m, k] * cd[:, o + k, :]
            out_c[:, o + m, :] = acc
    if round32:
        out_x, out_q, out_ls = (v.astype(np.float32) for v in (out_x, out_q, out_ls))
    return out_x, out_c, out_ls, out_q


def transform_boxes(sim: Similarity, boxes):
    """The box rule on float32 numpy boxes [N,2,4]: lo'_a = (sum_b (R_ab >= 0 ? R_ab lo_b : R_ab hi_b)) s + t_a, hi'_a
    the same with lo and hi swapped (float64, left to right, rounded once): the AABB of the rotated box.  Every term
    is monotone in its input, so nested boxes stay nested after rounding.  boxes'[:,0,3] = the largest edge of the
    ROUNDED box in float32, as the builder computes it; boxes[:,1,3] is copied."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 2, 4)
    lo, hi = b[:, 0, :3].astype(np.float64), b[:, 1, :3].astype(np.float64)
    out = b.copy()
    for a in range(3):
        tl = [sim.R[a, k] * (lo[:, k] if sim.R[a, k] >= 0 else hi[:, k]) for k in range(3)]
        th = [sim.R[a, k] * (hi[:, k] if sim.R[a, k] >= 0 else lo[:, k]) for k in range(3)]
        out[:, 0, a] = (((tl[0] + tl[1]) + tl[2]) * sim.s + sim.t[a]).astype(np.float32)
        out[:, 1, a] = (((th[0] + th[1]) + th[2]) * sim.s + sim.t[a]).astype(np.float32)
    e = out[:, 1, :3] - out[:, 0, :3]
    out[:, 0, 3] = np.maximum(np.maximum(e[:, 0], e[:, 1]), e[:, 2])
    return out


def transform_hierarchy(h: Hierarchy, sim: Similarity) -> Hierarchy:
    """Move a hierarchy by x' = s R x + t (the float64 numpy spec; ``transform_hierarchy_gpu`` is the same rule on the
    device): all G rows by ``transform_rows`` (the skybox tail behind the N nodes included), the N boxes by
    ``transform_boxes``; ``nodes`` and ``alpha`` are copied bit for bit.  M must be 1, 4, 9 or 16.  The identity
    reproduces every bit of finite input except the sign of a zero (-0.0 + 0.0 = +0.0).  For signed-permutation
    rotations the boxes are the permuted boxes; for others they grow (the AABB of the rotated AABB, up to sqrt 3),
    and with them the LOD sizes: what is invariant is the content rendered at a given cut, not the cut at a given
    granularity.  -> a new Hierarchy (host)."""
    M = _transform_sh_width(h.shs)
    check_similarity(sim)
    G, N = int(h.xyz.shape[0]), int(h.nodes.shape[0])
    if N < 1 or G < N or G > TRANSFORM_MAX_NODES:
        raise ValueError(f"G = {G} rows, N = {N} nodes; 1 <= N <= G <= 2^31 - 1 expected")
    np32 = lambda v: v.detach().cpu().numpy().astype(np.float32)
    x, c, ls, q = transform_rows(sim, np32(h.xyz), np32(h.shs).reshape(G, M, 3), np32(h.log_scales), np32(h.rots))
    boxes = transform_boxes(sim, np32(h.boxes).reshape(N, 2, 4))
    cp = lambda v: v.detach().cpu().clone()
    return Hierarchy(xyz=torch.from_numpy(x), shs=torch.from_numpy(c).reshape(h.shs.shape), alpha=cp(h.alpha),
                     log_scales=torch.from_numpy(ls), rots=torch.from_numpy(q), nodes=cp(h.nodes),
                     boxes=torch.from_numpy(boxes).reshape(h.boxes.shape))


def transform_args(sim: Similarity):
    """``sim`` as the C ABI's hgs_hier_transform_args (the same doubles)."""
    from . import _lib
    a = _lib.HierTransformArgs()
    a.R[:] = [float(v) for v in np.asarray(sim.R, dtype=np.float64).reshape(-1)]
    a.q[:] = [float(v) for v in np.asarray(sim.q_R, dtype=np.float64).reshape(-1)]
    a.s, a.log_s = float(sim.s), float(sim.log_s)
    a.t[:] = [float(v) for v in np.asarray(sim.t, dtype=np.float64).reshape(-1)]
    for name in ("D1", "D2", "D3"):
        getattr(a, name)[:] = [float(v) for v in np.asarray(getattr(sim, name), dtype=np.float64).reshape(-1)]
    return a


def transform_hierarchy_gpu(h: Hierarchy, sim: Similarity, inplace=False, stats=None) -> Hierarchy:
    """``transform_hierarchy`` on the GPU (csrc/hier_transform.hip, hgs_hier_transform).  ``h``: contiguous device
    tensors (float32 rows of G >= N, int32 nodes [N,7], boxes [N,2,4]).  ``inplace``: ``h``'s own tensors are rewritten
    and ``h`` is returned; otherwise ``h`` is left as it is and a new Hierarchy on the same device is returned.  Every
    output bit equals the spec's.  The call is asynchronous on the current stream.  ``stats`` (a dict, optional)
    receives ``transform_ms`` (device events around the call).  No CPU fallback: raises without libhgs.so or a GPU."""
    lib, _ = _need_gpu("transform_hierarchy_gpu", "transform_hierarchy")
    M = _transform_sh_width(h.shs)
    check_similarity(sim)
    G, N = int(h.xyz.shape[0]), int(h.nodes.shape[0])
    if N < 1 or G < N or G > TRANSFORM_MAX_NODES:
        raise ValueError(f"G = {G} rows, N = {N} nodes; 1 <= N <= G <= 2^31 - 1 expected")
    dev = _device_rows(h, _ROWS, "transform_hierarchy_gpu")
    out = h if inplace else Hierarchy(*(torch.empty_like(getattr(h, name)) for name in _ROWS))
    args = transform_args(sim)
    with torch.cuda.device(dev), _device_events(stats, "transform_ms"):
        _lib.check(lib.hgs_hier_transform(C.byref(_hier_view(h, G, N, M)), C.byref(_hier_view(out, G, N, M)),
                                          C.byref(args), _stream(dev), dev.index or 0), "hgs_hier_transform")
    return out


def transform_camera(cam, sim: Similarity):
    """The camera that sees a hierarchy moved by ``sim`` as ``cam`` saw the original: the stored (row-vector)
    ``world_view_transform`` and ``full_proj_transform`` left-multiplied by the inverse of ``sim.matrix()``, so that
    [x', 1] W' = [x, 1] W, and camera_center' = s R c + t.  The view matrix then carries the factor 1 / s: distances
    in camera space are the original's.  Computed in float64, stored in the camera's dtype.  -> a copy of ``cam``."""
    import copy
    Si = np.linalg.inv(sim.matrix())
    out = copy.copy(cam)
    for name in ("world_view_transform", "full_proj_transform"):
        m = getattr(cam, name)
        moved = Si @ m.detach().cpu().double().numpy()
        setattr(out, name, torch.from_numpy(moved).to(dtype=m.dtype, device=m.device))
    c = cam.camera_center
    setattr(out, "camera_center", torch.from_numpy(sim.apply(c.detach().cpu().double().numpy()))
            .to(dtype=c.dtype, device=c.device))
    return out


# ---- box refit: every box again from the rows it encloses, leaves first, parents as unions ---------------------------------
# hgs_hier_refit_report.first_bad, in the order they are reported: the merger's three layout checks, the depth checks of
# the aligner, the leaf boxes
REFIT_CHECKS = MERGE_CHECKS + ("depth outside [0, 255]",
                               "depth is not the parent's depth + 1 (without a parent in [0, N): depth != 0)",
                               "more than one node of depth 0",
                               "a leaf whose box is not finite or has lo > hi")
REFIT_CHILDREN_SUM = "count_children does not sum to N - 1 (two nodes claim the same children)"
REFIT_LEAF_MODES = {"keep": 0, "cube": 1, "ellipsoid": 2}      # hgs_hier_refit's leaf_mode
REFIT_MAX_NODES = (1 << 31) - 1


class HierarchyRefitError(HierarchyCheckError):
    """A hierarchy ``refit_boxes`` / ``refit_boxes_gpu`` rejected (nothing was written): ``check`` (what failed, one of
    REFIT_CHECKS or REFIT_CHILDREN_SUM) and ``node`` (the first offending node, None for the children sum)."""


def _refit_mode(leaf):
    if leaf not in REFIT_LEAF_MODES:
        raise ValueError(f"leaf = {leaf!r}; one of {', '.join(REFIT_LEAF_MODES)} expected")
    return REFIT_LEAF_MODES[leaf]


def leaf_boxes(xyz, log_scales, rots, mode, round32=True):
    """The leaf rule of ``refit_boxes`` on float32 numpy rows -> (lo [n,3], hi [n,3]), float32 (``round32=False``: the
    float64 values before their one rounding).  With s_k = exp(double(log_scales_k)): ``"cube"``: e = 3 max_k s_k,
    lo = x - e, hi = x + e (the builder's leaf rule on the stored rows); ``"ellipsoid"``: q^ = q / |q| with |q| =
    sqrt(((w w + x x) + y y) + z z), R = _rot_from_quat(q^), h_a = 3 sqrt(((R_a0 R_a0) s_0^2 + (R_a1 R_a1) s_1^2) +
    (R_a2 R_a2) s_2^2), lo = x - h, hi = x + h: the AABB of the 3 sigma ellipsoid.  Float64, every sum left to right.
    A NaN or inf row gives a box that is not finite; so does a zero quaternion under ``"ellipsoid"``."""
    if mode not in ("cube", "ellipsoid"):
        raise ValueError(f"mode = {mode!r}; cube or ellipsoid expected")
    x = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        s = np.exp(np.asarray(log_scales, dtype=np.float32).reshape(-1, 3).astype(np.float64))
        if mode == "cube":
            h = (3.0 * s.max(axis=1))[:, None]                 # (np.max propagates a NaN)
        else:
            q = np.asarray(rots, dtype=np.float32).reshape(-1, 4).astype(np.float64)
            n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
            R = _rot_from_quat(q / n[:, None])
            v = s * s
            h = 3.0 * np.sqrt(((R[:, :, 0] * R[:, :, 0]) * v[:, None, 0] + (R[:, :, 1] * R[:, :, 1]) * v[:, None, 1])
                              + (R[:, :, 2] * R[:, :, 2]) * v[:, None, 2])
        lo, hi = x - h, x + h
        return (lo.astype(np.float32), hi.astype(np.float32)) if round32 else (lo, hi)


def _box_extent(lo, hi):
    """boxes[:,0,3] of float32 (lo, hi): the largest edge, a float32 subtraction, as the builder computes it."""
    with np.errstate(all="ignore"):
        e = hi - lo
    return np.maximum(np.maximum(e[:, 0], e[:, 1]), e[:, 2])


def refit_first_bad(nodes, leaf_lo, leaf_hi):
    """The seven checks of ``refit_boxes`` on int32 nodes [N,7] and the float32 boxes (lo [N,3], hi [N,3]) its leaves
    are about to get (rows of other nodes are ignored) -> ([first offending node or -1] x 7 in the order of
    REFIT_CHECKS, the sum of count_children over the valid children ranges)."""
    nd = np.asarray(nodes).astype(np.int64)
    N = nd.shape[0]
    i = np.arange(N)
    depth, parent, cc = nd[:, 0], nd[:, 1], nd[:, 6]
    masks = list(layout_check_masks(nodes))
    masks.append((depth < 0) | (depth > 255))
    in_range = (parent >= 0) & (parent < N)
    masks.append((depth != 0) & (~in_range | (depth[np.where(in_range, parent, 0)] != depth - 1)))
    roots = i[depth == 0]
    second = np.zeros(N, dtype=bool)
    second[roots[1:2]] = True
    masks.append(second)
    with np.errstate(all="ignore"):
        ok = np.isfinite(leaf_lo).all(1) & np.isfinite(leaf_hi).all(1) & (leaf_lo <= leaf_hi).all(1)
    masks.append((cc == 0) & ~ok)
    first = [int(np.nonzero(m)[0][0]) if m.any() else -1 for m in masks]
    return first, int(cc[~masks[1]].sum())


def refit_boxes(h: Hierarchy, leaf="cube") -> Hierarchy:
    """Every box again from the rows it is meant to enclose (the float64 numpy spec; ``refit_boxes_gpu`` is the same
    rule on the device).  Only ``boxes`` changes: the five row tensors, ``nodes`` and rows at index >= N come back bit
    for bit.  A leaf (count_children == 0) by ``leaf``: ``"keep"`` its input box, all eight floats; ``"cube"`` or
    ``"ellipsoid"`` the box ``leaf_boxes`` gives its row.  A node with children: lo = min, hi = max over the FINAL boxes
    of its children [start_children, start_children + count_children), children before parents; its own Gaussian is
    not included (the builder's and the merger's rule).  Every written box: boxes[n,0,3] = max_a (hi_a - lo_a) in
    float32 on the rounded values; boxes[n,1,3] is copied.  The result nests exactly (min, max and rounding are
    monotone); ``"keep"`` returns the bits of a hierarchy this package built or merged.
    Refused with ``HierarchyRefitError`` (check, first offending node), all before anything is computed: the three
    layout checks, a depth outside [0, 255], a depth that is not the parent's + 1, a second node of depth 0, a leaf
    whose box is not finite or has lo > hi (NaN or inf rows, a zero quaternion under ``"ellipsoid"``, a bad kept box
    under ``"keep"``), and a count_children sum other than N - 1.  -> a new Hierarchy (host)."""
    _refit_mode(leaf)
    nodes = h.nodes.detach().cpu().numpy().astype(np.int32)
    N, G = nodes.shape[0], int(h.xyz.shape[0])
    if N < 1 or G < N or N > REFIT_MAX_NODES:
        raise ValueError(f"G = {G} rows, N = {N} nodes; 1 <= N <= G, N <= 2^31 - 1 expected")
    np32 = lambda v: v.detach().cpu().numpy().astype(np.float32)
    boxes = np32(h.boxes).reshape(-1, 2, 4)
    assert boxes.shape[0] == N
    if leaf == "keep":
        lo, hi = boxes[:, 0, :3].copy(), boxes[:, 1, :3].copy()
    else:
        lo, hi = leaf_boxes(np32(h.xyz)[:N], np32(h.log_scales)[:N], np32(h.rots)[:N], leaf)
    first_bad, children_sum = refit_first_bad(nodes, lo, hi)
    refuse = lambda check, node: HierarchyRefitError(check, node, f"not a hierarchy that can be refit: {check} (first "
                                                                  f"offending node {node}); nothing was written")
    _raise_first_bad(REFIT_CHECKS, first_bad, refuse)
    if children_sum != N - 1:
        raise HierarchyRefitError(REFIT_CHILDREN_SUM, None, f"not a hierarchy that can be refit: count_children sums to "
                                                            f"{children_sum} over {N} nodes; nothing was written")
    depth, sc, cc = nodes[:, 0].astype(np.int64), nodes[:, 5].astype(np.int64), nodes[:, 6].astype(np.int64)
    out = boxes.copy()
    leaf_ids = np.nonzero(cc == 0)[0]
    if leaf != "keep":
        out[leaf_ids, 0, :3], out[leaf_ids, 1, :3] = lo[leaf_ids], hi[leaf_ids]
        out[leaf_ids, 0, 3] = _box_extent(lo[leaf_ids], hi[leaf_ids])
    for d in range(int(depth.max()) - 1, -1, -1):              # children before parents
        ids = np.nonzero((depth == d) & (cc > 0))[0]
        if ids.size == 0:
            continue
        starts = np.concatenate([[0], np.cumsum(cc[ids])[:-1]])
        kids = np.repeat(sc[ids] - starts, cc[ids]) + np.arange(int(cc[ids].sum()))
        l = np.minimum.reduceat(out[kids, 0, :3], starts, axis=0)
        u = np.maximum.reduceat(out[kids, 1, :3], starts, axis=0)
        out[ids, 0, :3], out[ids, 1, :3] = l, u
        out[ids, 0, 3] = _box_extent(l, u)
    cp = lambda v: v.detach().cpu().clone()
    return Hierarchy(xyz=cp(h.xyz), shs=cp(h.shs), alpha=cp(h.alpha), log_scales=cp(h.log_scales), rots=cp(h.rots),
                     nodes=cp(h.nodes), boxes=torch.from_numpy(out).reshape(h.boxes.shape))


def refit_boxes_gpu(h: Hierarchy, leaf="cube", inplace=False, stats=None, report=None) -> Hierarchy:
    """``refit_boxes`` on the GPU (csrc/hier_refit.hip, hgs_hier_refit).  ``h``: contiguous device tensors (float32 rows
    of G >= N, int32 nodes [N,7], boxes [N,2,4]); rows behind the N nodes are neither read nor written.  ``inplace``:
    ``h.boxes`` is rewritten and ``h`` is returned; otherwise ``h`` is left as it is and the result is a Hierarchy with
    a new ``boxes`` tensor that SHARES the six other tensors with ``h`` (no row changes, so none is copied).  Interior
    boxes, extents and kept leaves equal the spec's bit for bit; ``"cube"`` and ``"ellipsoid"`` leaf coordinates are
    within one float32 ulp of it (the device's double exp may round differently from numpy's).  A hierarchy that fails
    a check raises ``HierarchyRefitError`` naming the check and the first offending node and is left untouched, in place
    or out of place.  One host wait (the level sizes and the checks), the rest is asynchronous on the current stream.
    ``stats`` (a dict, optional) receives ``refit_ms`` (device events around the call), ``levels`` and ``leaves``;
    ``report`` (optional) a ``_lib.HierRefitReport`` to fill.  No CPU fallback: raises without libhgs.so or a GPU."""
    lib, _ = _need_gpu("refit_boxes_gpu", "refit_boxes")
    mode = _refit_mode(leaf)
    G, N, M = _tensor_sizes(h)
    if N < 1 or G < N or N > REFIT_MAX_NODES:
        raise ValueError(f"G = {G} rows, N = {N} nodes; 1 <= N <= G, N <= 2^31 - 1 expected")
    dev = _device_rows(h, _ROWS, "refit_boxes_gpu")
    boxes_out = h.boxes if inplace else torch.empty_like(h.boxes)
    tmp = torch.empty(lib.hgs_hier_refit_tmp_bytes(N), dtype=torch.uint8, device=dev)
    rep = _lib.HierRefitReport() if report is None else report
    rep.first_bad[:] = [-1] * 7              # (a call that fails its size checks does not fill the report)
    p = _lib.ptr
    with torch.cuda.device(dev), _device_events(stats, "refit_ms"):
        rc = lib.hgs_hier_refit(C.byref(_hier_view(h, G, N, M)), p(boxes_out), mode, p(tmp), C.byref(rep), _stream(dev),
                                dev.index or 0)
        if rc != 0:
            msg = (lib.hgs_last_error() or b"?").decode()
            _raise_first_bad(REFIT_CHECKS, rep.first_bad,
                             lambda check, node: HierarchyRefitError(check, node, f"hgs_hier_refit: {msg}"))
            if rc == 1 and "count_children sums to" in msg:
                raise HierarchyRefitError(REFIT_CHILDREN_SUM, None, f"hgs_hier_refit: {msg}")
            raise _lib.HgsError(f"hgs_hier_refit failed (code {rc}): {msg}", rc)
    if stats is not None:
        stats["levels"], stats["leaves"] = int(rep.levels), int(rep.leaves)
    if inplace:
        # the library wrote h.boxes behind torch's back: an in-place no-op on an empty view bumps the version counter,
        # which is what the cached "do these boxes nest?" answer of gaussian_hierarchy._C is keyed on
        h.boxes.reshape(-1)[:0].zero_()
    return h if inplace else Hierarchy(h.xyz, h.shs, h.alpha, h.log_scales, h.rots, h.nodes, boxes_out)


# ---- leaf removal: take leaves out, drop what dies with them, re-merge the ancestors that changed -------------------------
# This project's own rule (DESIGN.md section 4 "Removing leaves (f-21)").  hgs_hier_prune_report.first_bad, in the order
# they are reported: the three layout checks and the three depth checks of the refit
PRUNE_CHECKS = REFIT_CHECKS[:6]
PRUNE_CHILDREN_SUM = REFIT_CHILDREN_SUM
PRUNE_ROOT_DEAD = "every leaf would be removed"
PRUNE_REMERGE = {"none": 0, "dirty": 1, "all": 2}      # hgs_hier_prune_apply's remerge
PRUNE_MAX_BOXES = 16
PRUNE_MAX_NODES = (1 << 31) - 1


class HierarchyPruneError(HierarchyCheckError):
    """A hierarchy ``prune_hierarchy`` / ``prune_hierarchy_gpu`` rejected (nothing was written): ``check`` (what failed,
    one of PRUNE_CHECKS, PRUNE_CHILDREN_SUM or PRUNE_ROOT_DEAD) and ``node`` (the first offending node; None for the
    children sum, 0 for the root)."""


@dataclass
class PruneResult:
    hierarchy: Hierarchy        # the N' alive nodes, in ascending old order
    old_of_new: torch.Tensor    # int32 [N']
    new_of_old: torch.Tensor    # int32 [N], -1 at dead nodes
    removed_leaves: int         # leaves a criterion removed
    dead: int                   # N - N': the removed leaves and the nodes all of whose leaves were removed
    dirty: int                  # alive nodes with a dead or dirty child: their boxes, and by ``remerge`` their rows, changed
    single_child: int           # alive nodes left with exactly one child (such chains are not spliced)


def _as_f32(v, shape, what):
    a = np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32)
    if a.shape != shape or np.isnan(a).any():
        raise ValueError(f"{what}: {shape} numbers expected (no NaN)")
    return a


def prune_criteria(N, remove_boxes=None, keep_box=None, min_opacity=None, max_scale=None, remove=None):
    """The criteria of ``prune_hierarchy`` as the numbers both the spec and the device compare: ``boxes`` float32 [k,2,3]
    (k <= 16 closed boxes (lo, hi)), ``keep`` float32 [2,3] or None, ``min_opacity`` float32 or None, ``log_max_scale``
    = float32(log(S)) or None -- the logarithm is taken once, here --, ``remove`` uint8 numpy [N] or a uint8 device
    tensor [N] or None.  NaN bounds, more than 16 boxes and S <= 0 are refused."""
    boxes = np.zeros((0, 2, 3), dtype=np.float32)
    if remove_boxes is not None:
        k = len(remove_boxes)
        if k > PRUNE_MAX_BOXES:
            raise ValueError(f"{k} remove boxes; at most {PRUNE_MAX_BOXES} expected")
        if k:
            boxes = np.stack([_as_f32(np.stack([np.asarray(b[0], dtype=np.float64), np.asarray(b[1], dtype=np.float64)]),
                                      (2, 3), "a remove box (lo[3], hi[3])") for b in remove_boxes])
    keep = None if keep_box is None else _as_f32(np.stack([np.asarray(keep_box[0], dtype=np.float64),
                                                            np.asarray(keep_box[1], dtype=np.float64)]), (2, 3),
                                                  "keep_box (lo[3], hi[3])")
    A = None if min_opacity is None else np.float32(min_opacity)
    if A is not None and np.isnan(A):
        raise ValueError("min_opacity is NaN")
    L = None
    if max_scale is not None:
        S = float(max_scale)
        if not S > 0.0:
            raise ValueError(f"max_scale = {max_scale}; a positive number expected")
        L = np.float32(np.log(np.float64(S)))
    if remove is not None:
        if torch.is_tensor(remove) and remove.is_cuda:
            remove = remove.reshape(-1).to(torch.uint8).contiguous()
        else:
            remove = (np.asarray(remove.detach().cpu().numpy() if torch.is_tensor(remove) else remove).reshape(-1) != 0) \
                .astype(np.uint8)
        if int(remove.shape[0]) != N:
            raise ValueError(f"remove has {int(remove.shape[0])} entries; N = {N} expected")
    return dict(boxes=boxes, keep=keep, min_opacity=A, log_max_scale=L, remove=remove)


def _inside(x, box):
    with np.errstate(invalid="ignore"):
        return ((x >= box[0][None, :]) & (x <= box[1][None, :])).all(1)


def prune_removed(xyz, alpha, log_scales, crit):
    """Step 1 of the rule at every row of float32 numpy (xyz [n,3], alpha [n], log_scales [n,3]) -> bool [n]; the caller
    masks it with count_children == 0.  float32 comparisons only; a NaN mean is in no box."""
    n = xyz.shape[0]
    r = np.zeros(n, dtype=bool)
    for b in crit["boxes"]:
        r |= _inside(xyz, b)
    if crit["keep"] is not None:
        r |= ~_inside(xyz, crit["keep"])
    with np.errstate(invalid="ignore"):
        if crit["min_opacity"] is not None:
            r |= ~(alpha >= crit["min_opacity"])
        if crit["log_max_scale"] is not None:
            r |= ~(log_scales.max(axis=1) <= crit["log_max_scale"])          # (np.max propagates a NaN)
    if crit["remove"] is not None:
        rm = crit["remove"]
        r |= (rm.cpu().numpy() if torch.is_tensor(rm) else rm) != 0
    return r


def _children_of(ids, sc, cc):
    """-> (kids, starts): the children of ``ids`` one after another, and where each node's run starts (for reduceat)."""
    starts = np.concatenate([[0], np.cumsum(cc[ids])[:-1]])
    kids = np.repeat(sc[ids] - starts, cc[ids]) + np.arange(int(cc[ids].sum()))
    return kids, starts


def merge_rows(xyz, shs, alpha, log_scales, rots, counts, weights=None):
    """The merge rule of an interior node generalised to k children ("Interior nodes"; the float64
    numpy statement of csrc/hier_merge_rule.h).  The children's rows are float32 numpy arrays, node after node: node j
    owns the next ``counts[j]`` rows.  w_c = ``weights`` (float64, one per child row: what ``prune_hierarchy`` carries
    up from the leaves) or, without them, alpha_c exp(ls_c0) exp(ls_c1) exp(ls_c2) of the row; f_c = w_c / max(sum w_c, 1e-30);
    mean = sum f_c x_c; covariance = sum f_c (R_c diag(s_c^2) R_c^T + d_c d_c^T) with R_c = _rot_from_quat of the
    stored quaternion; SH and opacity = f-weighted averages, opacity clipped to [0, 1]; eigenvalues ascending and
    clamped at 1e-12, every eigenvector's largest component (the first of equal ones) positive, column 0 negated if
    the frame is improper.  Every sum runs over a node's children left to right.
    -> dict of float64 arrays: xyz [n,3], shs [n,W], alpha [n], log_scales [n,3], rots [n,4], cov [n,3,3]."""
    counts = np.asarray(counts, dtype=np.int64)
    n = counts.shape[0]
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]) if n else np.zeros(0, dtype=np.int64)
    x = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    sh = np.asarray(shs, dtype=np.float32).reshape(x.shape[0], -1).astype(np.float64)
    al = np.asarray(alpha, dtype=np.float32).reshape(-1).astype(np.float64)
    ls = np.asarray(log_scales, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    q = np.asarray(rots, dtype=np.float32).reshape(-1, 4).astype(np.float64)
    with np.errstate(all="ignore"):
        s = np.exp(ls)
        w = al * ((s[:, 0] * s[:, 1]) * s[:, 2]) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        R = _rot_from_quat(q)
        C = (R * (s * s)[:, None, :]) @ R.transpose(0, 2, 1)
        kmax = int(counts.max()) if n else 0
        slot = lambda j: (counts > j, np.where(counts > j, first + j, first))     # (a node without slot j: f = 0 there)
        total = np.zeros(n)
        for j in range(kmax):
            m, c = slot(j)
            total = total + np.where(m, w[c], 0.0)
        ws = np.maximum(total, 1e-30)
        mu, op, shm = np.zeros((n, 3)), np.zeros(n), np.zeros((n, sh.shape[1]))
        for j in range(kmax):
            m, c = slot(j)
            f = np.where(m, w[c] / ws, 0.0)
            mu = mu + f[:, None] * x[c]
            op = op + f * al[c]
            shm = shm + f[:, None] * sh[c]
        cov = np.zeros((n, 3, 3))
        for j in range(kmax):
            m, c = slot(j)
            f = np.where(m, w[c] / ws, 0.0)
            d = x[c] - mu
            cov = cov + f[:, None, None] * (C[c] + d[:, :, None] * d[:, None, :])
        evals, evecs = np.linalg.eigh(cov) if n else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
        evals = np.maximum(evals, 1e-12)
        lead = np.argmax(np.abs(evecs), axis=1)                      # per column, the first of equal ones
        sign = np.where(np.take_along_axis(evecs, lead[:, None, :], axis=1)[:, 0, :] < 0, -1.0, 1.0)
        evecs = evecs * sign[:, None, :]
        flip = np.linalg.det(evecs) < 0
        evecs[flip, :, 0] *= -1
        quat = _quat_from_rot(evecs) if n else np.zeros((0, 4))
    return dict(xyz=mu, shs=shm, alpha=np.clip(op, 0.0, 1.0), log_scales=np.log(np.sqrt(evals)), rots=quat, cov=cov, weight=ws)


def prune_hierarchy(h: Hierarchy, *, remove_boxes=None, keep_box=None, min_opacity=None, max_scale=None, remove=None,
                    remerge="dirty") -> PruneResult:
    """Remove leaves from a hierarchy, drop every node all of whose leaves went, and re-merge the ancestors that changed
    (the numpy spec, float64 where it computes rows; ``prune_hierarchy_gpu`` is the same rule on the device).  This
    project's own rule.
    A node without children is REMOVED iff a given criterion holds, all in float32: its mean lies in one of the closed
    ``remove_boxes`` [(lo[3], hi[3]), ...] (at most 16; a NaN coordinate is in no box); its mean does not lie in
    ``keep_box`` (lo[3], hi[3]); not (alpha >= ``min_opacity``); not (max(log_scales) <= float32(log(``max_scale``)));
    ``remove`` (uint8 [N]) is nonzero at it.  Bottom-up, a leaf is ALIVE iff it is not removed and a node with children
    iff one of its children is; an alive node with children is DIRTY iff one of its children is dead or dirty.  The
    alive nodes keep their ascending order: depth, count_leafs and count_merged kept, parent / start / start_children
    renumbered, count_children = the surviving children (a node left with one child stays).  Leaves and clean nodes
    are bit copies.  A dirty node's box is the union of its surviving children's final boxes (extent = its largest edge,
    boxes[n,1,3] copied), in every ``remerge`` mode; its row is ``merge_rows`` of its surviving children's final
    float32 rows, deepest level first, with the weights the builder carries: a leaf weighs alpha s0 s1 s2 of its row
    (s = exp(log_scales), double), a node with children the sum of its surviving children's weights, clamped at 1e-30
    -- the sum over its surviving leaves, not alpha s0 s1 s2 of its own merged row.  ``remerge="none"`` keeps the dirty rows (a topology-only prune);
    ``remerge="all"`` recomputes the row of every alive node with children (clean ones keep their boxes).  Rows at
    index >= N are not the function's business: the result has G = N' rows.  Removing nothing returns the input's bits.
    Refused with ``HierarchyPruneError`` (check, first offending node), before anything is computed: the six checks of
    PRUNE_CHECKS, a count_children sum other than N - 1, and a dead root.  -> PruneResult (host tensors)."""
    if remerge not in PRUNE_REMERGE:
        raise ValueError(f"remerge = {remerge!r}; one of {', '.join(PRUNE_REMERGE)} expected")
    nodes = h.nodes.detach().cpu().numpy().astype(np.int32)
    N, G = nodes.shape[0], int(h.xyz.shape[0])
    if N < 1 or G < N or N > PRUNE_MAX_NODES:
        raise ValueError(f"G = {G} rows, N = {N} nodes; 1 <= N <= G, N <= 2^31 - 1 expected")
    crit = prune_criteria(N, remove_boxes, keep_box, min_opacity, max_scale, remove)
    np32 = lambda v: v.detach().cpu().numpy().astype(np.float32)
    rows = {k: np32(getattr(h, k))[:N].copy() for k in ("xyz", "shs", "alpha", "log_scales", "rots")}
    boxes = np32(h.boxes).reshape(-1, 2, 4).copy()
    assert boxes.shape[0] == N
    first_bad, children_sum = refit_first_bad(nodes, np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32))
    refuse = lambda check, node: HierarchyPruneError(check, node, f"not a hierarchy that can be pruned: {check} (first "
                                                                  f"offending node {node}); nothing was written")
    _raise_first_bad(PRUNE_CHECKS, first_bad[:6], refuse)
    if children_sum != N - 1:
        raise HierarchyPruneError(PRUNE_CHILDREN_SUM, None, f"not a hierarchy that can be pruned: count_children sums to "
                                                            f"{children_sum} over {N} nodes; nothing was written")
    depth, sc, cc = nodes[:, 0].astype(np.int64), nodes[:, 5].astype(np.int64), nodes[:, 6].astype(np.int64)
    # ---- 1-3: removed, alive, dirty
    removed = (cc == 0) & prune_removed(rows["xyz"], rows["alpha"].reshape(-1), rows["log_scales"], crit)
    alive = (cc == 0) & ~removed
    dirty = np.zeros(N, dtype=bool)
    surviving, first_alive = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for d in range(int(depth.max()) - 1, -1, -1):              # children before parents
        ids = np.nonzero((depth == d) & (cc > 0))[0]
        if ids.size == 0:
            continue
        kids, starts = _children_of(ids, sc, cc)
        a = alive[kids]
        n = np.add.reduceat(a.astype(np.int64), starts)
        alive[ids] = n > 0
        dirty[ids] = (n > 0) & np.logical_or.reduceat(~a | dirty[kids], starts)
        surviving[ids] = n
        first_alive[ids] = np.minimum.reduceat(np.where(a, kids, N), starts)
    if not alive[0]:
        raise HierarchyPruneError(PRUNE_ROOT_DEAD, 0, f"{PRUNE_ROOT_DEAD} ({int(removed.sum())} of {N} nodes are leaves a "
                                                      f"criterion removes); nothing was written")
    # ---- 4: topology
    old = np.nonzero(alive)[0]
    K = old.size
    new_of_old = np.full(N, -1, dtype=np.int32)
    new_of_old[old] = np.arange(K, dtype=np.int32)
    out = nodes[old].copy()
    out[:, 1] = np.where(old == 0, -1, new_of_old[np.maximum(nodes[old, 1], 0)])
    out[:, 2] = np.arange(K, dtype=np.int32)
    inner = cc[old] > 0
    out[inner, 5] = new_of_old[first_alive[old[inner]]]
    out[inner, 6] = surviving[old[inner]]
    # ---- 5, 6: rows and boxes, deepest level first, from the children's FINAL float32 rows
    r = {k: v[old] for k, v in rows.items()}
    b = boxes[old]
    odepth, osc, occ, odirty = out[:, 0].astype(np.int64), out[:, 5].astype(np.int64), out[:, 6].astype(np.int64), dirty[old]
    with np.errstate(all="ignore"):
        sl = np.exp(r["log_scales"].astype(np.float64))
        weight = np.where(occ == 0, r["alpha"].reshape(K).astype(np.float64) * ((sl[:, 0] * sl[:, 1]) * sl[:, 2]), 0.0)
    for d in range(int(odepth.max()) - 1, -1, -1):
        level = (odepth == d) & (occ > 0)
        ids = np.nonzero(level)[0]
        if ids.size and remerge != "none":                     # the carried weights, at clean nodes too
            kids, _ = _children_of(ids, osc, occ)
            total, first = np.zeros(ids.size), osc[ids]
            for j in range(int(occ[ids].max())):
                total = total + np.where(occ[ids] > j, weight[np.where(occ[ids] > j, first + j, first)], 0.0)
            weight[ids] = np.maximum(total, 1e-30)
        ids = np.nonzero(level & odirty)[0]
        if ids.size:
            kids, starts = _children_of(ids, osc, occ)
            lo = np.minimum.reduceat(b[kids, 0, :3], starts, axis=0)
            hi = np.maximum.reduceat(b[kids, 1, :3], starts, axis=0)
            b[ids, 0, :3], b[ids, 1, :3] = lo, hi
            b[ids, 0, 3] = _box_extent(lo, hi)
        ids = np.nonzero(level & {"none": np.zeros(K, dtype=bool), "dirty": odirty, "all": np.ones(K, dtype=bool)}[remerge])[0]
        if ids.size:
            kids, _ = _children_of(ids, osc, occ)
            m = merge_rows(r["xyz"][kids], r["shs"][kids], r["alpha"][kids], r["log_scales"][kids], r["rots"][kids], occ[ids],
                           weight[kids])
            for k in ("xyz", "log_scales", "rots"):
                r[k][ids] = m[k].astype(np.float32)
            r["shs"][ids] = m["shs"].astype(np.float32).reshape((ids.size,) + r["shs"].shape[1:])
            r["alpha"][ids] = m["alpha"].astype(np.float32).reshape((ids.size,) + r["alpha"].shape[1:])
    t = torch.from_numpy
    ph = Hierarchy(xyz=t(r["xyz"]), shs=t(r["shs"]), alpha=t(r["alpha"]), log_scales=t(r["log_scales"]), rots=t(r["rots"]),
                   nodes=t(out), boxes=t(b).reshape((K,) + tuple(h.boxes.shape[1:])))
    return PruneResult(ph, t(old.astype(np.int32)), t(new_of_old), int(removed.sum()), int(N - K), int(dirty.sum()),
                       int((occ == 1).sum()))


def prune_hierarchy_gpu(h: Hierarchy, *, remove_boxes=None, keep_box=None, min_opacity=None, max_scale=None, remove=None,
                        remerge="dirty", align=False, stats=None) -> PruneResult:
    """``prune_hierarchy`` on the GPU (csrc/hier_prune.hip: hgs_hier_prune_plan, then N' rows are allocated, then
    hgs_hier_prune_apply).  ``h``: contiguous device tensors (float32 rows of G >= N, int32 nodes [N,7], boxes
    [N,2,4]); it is not modified, and rows behind the N nodes are not read.  ``remove``: uint8 or bool [N], host or
    device.  The records, the boxes, both maps, the counts and every row that is copied equal the spec's bit for bit; a
    re-merged row agrees with it within the builder's bounds (mean, SH, opacity 1e-5; covariance 1e-5 Frobenius): the
    frame of a near-isotropic covariance is free.  Re-merged rows come in the builder's canonical frame, not their
    parents': ``align=True`` runs ``align_hierarchy_gpu`` on the result.  A hierarchy that fails a check, or all of whose
    leaves would go, raises ``HierarchyPruneError`` naming the check and the node; nothing has been allocated or written
    then.  Two host waits (the level sizes and the checks; the counts), the rest is asynchronous on the current stream.
    ``stats`` (a dict, optional) receives ``prune_ms`` (device events around plan, the allocation and apply), its parts
    ``plan_ms`` and ``apply_ms``, and ``levels``.  No CPU fallback: raises without libhgs.so or a GPU."""
    lib, _ = _need_gpu("prune_hierarchy_gpu", "prune_hierarchy")
    if remerge not in PRUNE_REMERGE:
        raise ValueError(f"remerge = {remerge!r}; one of {', '.join(PRUNE_REMERGE)} expected")
    G, N, M = _tensor_sizes(h)
    if N < 1 or G < N or N > PRUNE_MAX_NODES:
        raise ValueError(f"G = {G} rows, N = {N} nodes; 1 <= N <= G, N <= 2^31 - 1 expected")
    dev = _device_rows(h, _ROWS, "prune_hierarchy_gpu")
    crit = prune_criteria(N, remove_boxes, keep_box, min_opacity, max_scale, remove)
    args = _lib.HierPruneArgs(len(crit["boxes"]), 0 if crit["keep"] is None else 1, 0 if crit["min_opacity"] is None else 1,
                              0 if crit["log_max_scale"] is None else 1)
    for k, bx in enumerate(crit["boxes"]):
        args.remove_lo[k][:], args.remove_hi[k][:] = [float(x) for x in bx[0]], [float(x) for x in bx[1]]
    if crit["keep"] is not None:
        args.keep_lo[:], args.keep_hi[:] = [float(x) for x in crit["keep"][0]], [float(x) for x in crit["keep"][1]]
    args.min_opacity = 0.0 if crit["min_opacity"] is None else float(crit["min_opacity"])
    args.log_max_scale = 0.0 if crit["log_max_scale"] is None else float(crit["log_max_scale"])
    mask = crit["remove"]
    if mask is not None:
        mask = (mask if torch.is_tensor(mask) else torch.from_numpy(mask)).to(dev).contiguous()
    p = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev), _device_events(stats, "prune_ms") as ev:
        tmp = torch.empty(lib.hgs_hier_prune_tmp_bytes(N), dtype=torch.uint8, device=dev)
        rep = _lib.HierPruneReport()
        rep.first_bad[:] = [-1] * 6              # (a call that fails its size checks does not fill the report)
        vin, stream = _hier_view(h, G, N, M), _stream(dev)
        rc = lib.hgs_hier_prune_plan(C.byref(vin), C.byref(args), p(mask), p(tmp), C.byref(rep), stream, dev.index or 0)
        if rc != 0:
            msg = (lib.hgs_last_error() or b"?").decode()
            _raise_first_bad(PRUNE_CHECKS, rep.first_bad,
                             lambda check, node: HierarchyPruneError(check, node, f"hgs_hier_prune_plan: {msg}"))
            if rc == 1 and "count_children sums to" in msg:
                raise HierarchyPruneError(PRUNE_CHILDREN_SUM, None, f"hgs_hier_prune_plan: {msg}")
            if rc == 1 and rep.root_dead:
                raise HierarchyPruneError(PRUNE_ROOT_DEAD, 0, f"hgs_hier_prune_plan: {msg}")
            raise _lib.HgsError(f"hgs_hier_prune_plan failed (code {rc}): {msg}", rc)
        n = int(rep.kept)
        out = _empty_hierarchy(dev, n, h.shs.shape[1:], h.alpha.shape[1:])
        old_of_new, new_of_old = (torch.empty(m, dtype=torch.int32, device=dev) for m in (n, N))
        mid = torch.cuda.Event(enable_timing=True)
        mid.record()
        _lib.check(lib.hgs_hier_prune_apply(C.byref(vin), C.byref(_hier_view(out, n, n, M)), p(tmp), PRUNE_REMERGE[remerge],
                                            p(old_of_new), p(new_of_old), stream, dev.index or 0), "hgs_hier_prune_apply")
    if stats is not None:
        stats["plan_ms"], stats["apply_ms"], stats["levels"] = ev[0].elapsed_time(mid), mid.elapsed_time(ev[1]), int(rep.levels)
    if align:
        align_hierarchy_gpu(out)
    out.boxes = out.boxes.reshape((n,) + tuple(h.boxes.shape[1:]))
    return PruneResult(out, old_of_new, new_of_old, int(rep.removed_leaves), int(rep.dead), int(rep.dirty),
                       int(rep.single_child))
