#!/usr/bin/env python
"""What a box refit does to the LOD cut (profiles/f19_refit.md), on the GPU:

  transforms   the 2 000-leaf scene of the tests under five transforms (identity, a half turn with s = 2, a quarter turn
               with a translation, a rotation by 1e-4 rad, a general rotation with s = 1.7) and under the five random
               rotations of the transform tests (seed 21, with their scales and translations): the root extent and the size
               of the cut at 3 and at 30 pixels from the (moved) camera for the original, the transformed hierarchy, and the
               transformed hierarchy refit with "cube" and with "ellipsoid"
  perturbed    the same scene with its rows moved under its boxes (means + 0.3 N(0,1), log-scales + 0.4 U(0,1), seed 19):
               leaves whose cube sticks out of the box they were loaded with, the cut sizes before and after a refit
  leaves       cube and ellipsoid leaf coordinates of the device against the float64 numpy spec, in float32 ulp

    python scripts/refit_effect.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))

from gaussian_hierarchy._C import expand_to_size   # noqa: E402
from hgs import hierarchy, synth   # noqa: E402

ARRAYS = ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes")
CAM = synth.make_camera(256, 160)
TAU_PX = 3.0
COARSE_PX = 30.0          # a second, coarser granularity: the cut at 3 px is nearly the leaves


def cut_size(h, viewpoint, tau):
    N = h.num_nodes
    dev = h.nodes.device
    ri = torch.zeros(N, dtype=torch.int32, device=dev)
    pi, ni = torch.zeros_like(ri), torch.zeros_like(ri)
    return expand_to_size(h.nodes, h.boxes, float(tau), torch.as_tensor(viewpoint, dtype=torch.float32), torch.zeros(3), ri, pi, ni)


def ulps(a, b):
    o = lambda x: (lambda i: np.where(i < 0, -(i & 0x7FFFFFFF), i))(np.ascontiguousarray(x).view(np.int32).astype(np.int64))
    return np.abs(o(a) - o(b))


def main():
    dev = torch.device("cuda", 0)
    host = hierarchy.build_hierarchy(synth.make_scene_trained_like(2000, CAM, seed=5))
    to_dev = lambda h: hierarchy.Hierarchy(*(getattr(h, k).to(dev).clone().contiguous() for k in ARRAYS))
    d = to_dev(host)
    c = CAM.camera_center.double().numpy()
    tiny = 1e-4
    rng = np.random.default_rng(11)
    q = rng.normal(size=4)
    sims = {"identity": hierarchy.similarity(),
            "half_turn_s2": hierarchy.similarity(R=np.diag([-1.0, 1.0, -1.0]), scale=2.0),
            "quarter_turn_t": hierarchy.similarity(R=np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), translate=(0.5, -4.0, 2.0)),
            "tiny_rotation": hierarchy.similarity(quat=(np.cos(tiny / 2), 0.0, np.sin(tiny / 2) * 0.6, np.sin(tiny / 2) * 0.8)),
            "general": hierarchy.similarity(quat=q / np.linalg.norm(q), scale=1.7, translate=(3.0, -2.0, 9.0))}
    # the five rotations of tests/test_hier_transform_cpu.py::test_nesting_survives_rounding_exactly, with its scales
    # and translations
    q5 = np.random.default_rng(21).normal(size=(5, 4))
    for k in range(5):
        sims[f"test rotation {k}"] = hierarchy.similarity(quat=q5[k] / np.linalg.norm(q5[k]), scale=(0.37, 1.0, 1.7, 12.5, 3.0)[k],
                                                         translate=(0.1 * k, -7.3, 100.0 * k))
    # ---- rows moved under their boxes
    p = hierarchy.Hierarchy(*(getattr(host, k).clone() for k in ARRAYS))
    g = torch.Generator().manual_seed(19)
    p.xyz += 0.3 * torch.randn(p.xyz.shape, generator=g)
    p.log_scales += 0.4 * torch.rand(p.log_scales.shape, generator=g)
    lo, hi = hierarchy.leaf_boxes(p.xyz.numpy(), p.log_scales.numpy(), p.rots.numpy(), "cube")
    b, leaf = p.boxes.numpy(), p.nodes[:, 6].numpy() == 0
    outside = leaf & ((lo < b[:, 0, :3]).any(1) | (hi > b[:, 1, :3]).any(1))
    dp = to_dev(p)
    for px in (TAU_PX, COARSE_PX):
        tau = 2 * px * CAM.tanfovx / (0.5 * CAM.image_width)
        print(f"original: root extent {float(d.boxes[0, 0, 3]):.6g}, cut at {px} px = {cut_size(d, c, tau)} of {d.num_nodes} nodes")
        print("| transform | root extent: transformed | + cube | + ellipsoid | cut: transformed | + cube | + ellipsoid |")
        print("|---|---|---|---|---|---|---|")
        for name, sim in sims.items():
            moved = hierarchy.transform_hierarchy_gpu(d, sim)
            v = sim.apply(c)
            t = tau                  # extents and distances both scale by s: the same granularity gives the same pixels
            row = [moved] + [hierarchy.refit_boxes_gpu(moved, leaf_mode) for leaf_mode in ("cube", "ellipsoid")]
            ext = " | ".join(f"{float(h.boxes[0, 0, 3]):.6g}" for h in row)
            cuts = " | ".join(str(cut_size(h, v, t)) for h in row)
            print(f"| {name} | {ext} | {cuts} |")
        line = (f"perturbed: {int(outside.sum())} of {int(leaf.sum())} leaves stick out of their stale box; cut at {px} px: "
                f"stale {cut_size(dp, c, tau)}")
        for mode in ("cube", "ellipsoid"):
            r = hierarchy.refit_boxes_gpu(dp, mode)
            line += f", {mode} {cut_size(r, c, tau)} (root extent {float(dp.boxes[0, 0, 3]):.6g} -> {float(r.boxes[0, 0, 3]):.6g})"
        print(line)
    # ---- the device's leaves against the spec
    for name, h in (("2 000 leaves", host), ("perturbed", p)):
        for mode in ("cube", "ellipsoid"):
            got = hierarchy.refit_boxes_gpu(to_dev(h), mode).boxes.cpu().numpy()
            wlo, whi = hierarchy.leaf_boxes(h.xyz.numpy(), h.log_scales.numpy(), h.rots.numpy(), mode)
            lf = h.nodes[:, 6].numpy() == 0
            u = np.maximum(ulps(got[lf, 0, :3], wlo[lf]), ulps(got[lf, 1, :3], whi[lf]))
            print(f"leaves, {name}, {mode}: {int(u.max())} ulp at most, {int((u > 0).sum())} of {u.size} coordinates differ")
    big = hierarchy.build_hierarchy_on_device(500_000, synth.make_camera(1920, 1080), dev, seed=1)
    for mode in ("cube", "ellipsoid"):
        got = hierarchy.refit_boxes_gpu(big, mode).boxes.cpu().numpy()
        wlo, whi = hierarchy.leaf_boxes(big.xyz.cpu().numpy(), big.log_scales.cpu().numpy(), big.rots.cpu().numpy(), mode)
        lf = big.nodes[:, 6].cpu().numpy() == 0
        u = np.maximum(ulps(got[lf, 0, :3], wlo[lf]), ulps(got[lf, 1, :3], whi[lf]))
        print(f"leaves, 500 000 leaves, {mode}: {int(u.max())} ulp at most, {int((u > 0).sum())} of {u.size} coordinates differ "
              f"({float((u > 0).mean()):.2e})")


if __name__ == "__main__":
    main()
