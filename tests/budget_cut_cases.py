"""Shared inputs of the budget-cut tests: small builder hierarchies with their culling balls, a hand-built nested
hierarchy with several rows per node, and the budgets / requests the issue of the feature lists."""
from __future__ import annotations

import functools

import numpy as np
import torch

import frustum_cases as fc
import frustum_spec as fs
from hgs import hierarchy, synth

CPU_LEAVES = (1, 2, 3, 33, 129, 1000)
TAU_MINS_PX = (None, 3.0, 40.0)          # None: tau_min = 0


@functools.lru_cache(maxsize=None)
def built(P):
    """(nodes int32 [N,7], boxes f32 [N,2,4], bounds f32 [N,4], means [G,3], scales [G,3]) of a P-leaf builder hierarchy."""
    if P == 20000:
        h, full, bounds = fc.hier20k()
        return h.nodes.numpy(), h.boxes.numpy(), bounds, full["xyz"].numpy(), full["scaling"].numpy()
    h = hierarchy.build_hierarchy(synth.make_scene_trained_like(P, synth.make_camera(fc.W, fc.H), seed=5 + P))
    means, scales = h.xyz.numpy(), torch.exp(h.log_scales).numpy()
    nodes = h.nodes.numpy()
    return nodes, h.boxes.numpy().reshape(-1, 2, 4), fs.bounds_spec(nodes, means, scales), means, scales


@functools.lru_cache(maxsize=None)
def multi_row():
    """fc.multi_row_case() with nested boxes around it, placed in front of cameras A and B: nodes of several rows, a
    node without rows (L + M = 0) and a node that has children AND leaf rows (node 1), for which ``rows`` is only an
    upper bound of the distinct rows."""
    nodes, means, scales = fc.multi_row_case()
    means = (means * np.float32(0.6) + np.array([0.0, 0.0, 6.0], np.float32)).astype(np.float32)
    N = nodes.shape[0]
    boxes = np.zeros((N, 2, 4), dtype=np.float32)
    mn = np.full((N, 3), np.inf, np.float32)
    mx = np.full((N, 3), -np.inf, np.float32)
    for n in range(N):
        s, c = int(nodes[n, 2]), int(nodes[n, 3] + nodes[n, 4])
        if c:
            mn[n] = (means[s:s + c] - 3 * scales[s:s + c]).min(0)
            mx[n] = (means[s:s + c] + 3 * scales[s:s + c]).max(0)
    mn[4], mx[4] = mn[3] + np.float32(0.01), mn[3] + np.float32(0.02)       # the empty node: a small box inside its sibling's
    for n in range(N - 1, 0, -1):                                          # children before parents (ids descend)
        p = int(nodes[n, 1])
        mn[p], mx[p] = np.minimum(mn[p], mn[n]), np.maximum(mx[p], mx[n])
    boxes[:, 0, :3], boxes[:, 1, :3] = mn, mx
    boxes[:, 0, 3] = np.linalg.norm((mx - mn).astype(np.float64), axis=1).astype(np.float32)
    return nodes, boxes, fs.bounds_spec(nodes, means, scales), means, scales


def planes_of(name):
    cam = fc.camera(name)
    planes, rs = fs.planes_spec(cam.world_view_transform.numpy(), cam.tanfovx, cam.tanfovy, fc.W, fc.H)
    return cam, planes, rs


def tau_min_of(cam, px):
    return 0.0 if px is None else fc.tau_of(cam, px)


def budgets(N, cost_inf):
    """The issue's budgets: cost(+inf), cost(+inf) + 1, 2, 3, N/8, N/4, N/2, N, 2N (duplicates dropped, order kept)."""
    return list(dict.fromkeys([cost_inf, cost_inf + 1, 2, 3, N // 8, N // 4, N // 2, N, 2 * N]))
