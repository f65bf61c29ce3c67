"""numpy restatement of the frustum-culled hierarchy cut ("Frustum-culled cut"; include/hgs.h):
the view-independent bounding spheres, the five planes and the filter applied to the oracle's unculled cut.  Everything
the device decides on is float32 in the fixed operation order of csrc/lod_frustum.hip (contraction off), so cuts compare
exactly; the planes are built in double and rounded once.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import math

import numpy as np

from oracle import lod_oracle as lo

F = np.float32
NEAR_Z = 0.2          # K1's near cull (view z)
K1_CLAMP = 1.3        # K1's clamp on t.x / t.z in units of tanfov
PAD_PX = 36.0         # fov_scale - 1 >= 36 / min(W, H): 18 px of slack on the narrower half-frame


def bounds_spec(nodes, means, scales):
    """float32 [N,4] = (centre, radius) of every node's own rows [start, start + count_leafs + count_merged): centre =
    mean of the rows' means (summed in row order, one division), radius = max_i(|m_i - c| + 3 max_k s_i,k).  A node
    without rows gets (0, 0, 0, +inf): it is never outside a plane."""
    nodes = np.asarray(nodes)
    m = np.ascontiguousarray(means, dtype=np.float32).reshape(-1, 3)
    s = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1, 3)
    N = nodes.shape[0]
    start = nodes[:, 2].astype(np.int64)
    cnt = (nodes[:, 3] + nodes[:, 4]).astype(np.int64)
    out = np.zeros((N, 4), dtype=np.float32)
    if N == 0:
        return out
    kmax = int(cnt.max())
    acc = np.zeros((N, 3), dtype=np.float32)
    for k in range(kmax):
        on = cnt > k
        acc[on] = acc[on] + m[start[on] + k]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (acc / cnt.astype(np.float32)[:, None]).astype(np.float32)
    R = np.zeros(N, dtype=np.float32)
    for k in range(kmax):
        on = cnt > k
        row = start[on] + k
        d = m[row] - c[on]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        smax = np.maximum(np.maximum(s[row, 0], s[row, 1]), s[row, 2])
        R[on] = np.maximum(R[on], np.sqrt(d2) + F(3.0) * smax)
    empty = cnt <= 0
    c[empty] = 0.0
    R[empty] = np.inf
    out[:, :3] = c
    out[:, 3] = R
    return out


def fov_scale(width, height):
    return max(K1_CLAMP, 1.0 + PAD_PX / min(int(width), int(height)))


def radius_scale_spec(tanfovx, tanfovy, scale_modifier=1.0):
    k2 = K1_CLAMP * K1_CLAMP
    tx, ty = float(tanfovx), float(tanfovy)
    kappa = math.sqrt((1.0 + k2 * (tx * tx + ty * ty)) / (1.0 + k2 * min(tx, ty) ** 2))
    return max(1.0, float(scale_modifier)) * kappa


def planes_spec(world_view_transform, tanfovx, tanfovy, width, height, scale_modifier=1.0, near=NEAR_Z):
    """(planes float32 [5,4], radius_scale).  Row k = (a, d) with a unit normal: a . x + d >= 0 inside.  Rows: left,
    right, bottom (-y), top (+y) side planes through the camera centre at tangents fov_scale * tanfov, then the near
    plane view z = near.  world_view_transform is the stored (row-vector) matrix: view = [x 1] @ M."""
    M = np.asarray(world_view_transform, dtype=np.float64).reshape(4, 4)
    fs = fov_scale(width, height)
    tx, ty = fs * float(tanfovx), fs * float(tanfovy)
    view_planes = [((1.0, 0.0, tx), 0.0), ((-1.0, 0.0, tx), 0.0), ((0.0, 1.0, ty), 0.0), ((0.0, -1.0, ty), 0.0),
                   ((0.0, 0.0, 1.0), -float(near))]
    out = np.zeros((5, 4), dtype=np.float64)
    for k, (nv, d0) in enumerate(view_planes):
        nv = np.asarray(nv)
        a = M[:3, :3] @ nv                    # view_j = sum_i x_i M[i][j] + M[3][j]
        d = float(M[3, :3] @ nv) + d0
        ln = math.sqrt(float(a @ a))
        out[k, :3] = a / ln
        out[k, 3] = d / ln
    return out.astype(np.float32), radius_scale_spec(tanfovx, tanfovy, scale_modifier)


def ball_outside(bounds, idx, plane, radius_scale):
    """float32: ((a.x c.x + a.y c.y) + a.z c.z) + d + radius_scale * R < 0 for the balls ``idx`` against one plane."""
    b = bounds[idx]
    a = np.asarray(plane, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((a[0] * b[:, 0] + a[1] * b[:, 1]) + a[2] * b[:, 2]) + a[3]
        return (t + F(radius_scale) * b[:, 3]) < F(0.0)


def culled_spec(nodes, bounds, node_indices, planes, radius_scale, own_ball_only=False):
    """bool [n]: the entries of the nodes ``node_indices`` that the rule drops: some plane has the node's ball AND its
    parent's ball (the root: itself) outside.  ``own_ball_only`` is the cheaper, UNSAFE rule the tests must catch."""
    nodes = np.asarray(nodes)
    bounds = np.asarray(bounds, dtype=np.float32)
    ni = np.asarray(node_indices, dtype=np.int64)
    par = nodes[ni, 1].astype(np.int64)
    par = np.where(par < 0, ni, par)
    out = np.zeros(ni.shape[0], dtype=bool)
    for k in range(5):
        o = ball_outside(bounds, ni, planes[k], radius_scale)
        if not own_ball_only:
            o &= ball_outside(bounds, par, planes[k], radius_scale)
        out |= o
    return out


def cut_view_spec(nodes, boxes, bounds, tau, viewpoint, planes, radius_scale):
    """The culled cut: the oracle's unculled cut and weights with the culled entries removed, nothing else changed.
    -> dict(n, n_unculled, render_indices, parent_indices, node_indices, weights, kids, culled)."""
    nodes = np.asarray(nodes)
    r, p, ni = lo.expand_to_size(nodes, boxes, tau, viewpoint)
    if len(ni):
        w, kids = lo.get_interpolation_weights(ni, tau, nodes, boxes, viewpoint)
        drop = culled_spec(nodes, bounds, ni, planes, radius_scale)
    else:
        w, kids, drop = np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, bool)
    keep = ~drop
    return dict(n=int(keep.sum()), n_unculled=int(len(r)), render_indices=r[keep], parent_indices=p[keep],
                node_indices=ni[keep], weights=w[keep], kids=kids[keep], culled=drop)
