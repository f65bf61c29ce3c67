"""Shared inputs of the contribution-score GPU tests: the 2 000-leaf hierarchy built on the GPU (once per session, kept
on the host and never modified), its camera, the three orbit cameras and the same cameras as ``cameras.json`` entries."""
import dataclasses
import functools

import torch

from hgs import hierarchy, synth

W, H = 64, 48
FIELDS = ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes")


def camera():
    return synth.make_camera(W, H)


@functools.lru_cache(maxsize=None)
def hier2000():
    """The host copy of ``build_hierarchy_gpu`` on ``make_scene(2000, camera(), seed=4)``: N = 3 999 nodes."""
    h = hierarchy.build_hierarchy_gpu(synth.make_scene(2000, camera(), seed=4), device=torch.device("cuda:0"))
    return dataclasses.replace(h, **{k: getattr(h, k).cpu() for k in FIELDS})


def on_device(h, dev, **changed):
    """A copy of ``h`` on ``dev`` (fresh tensors), ``changed`` fields replaced first."""
    h = dataclasses.replace(h, **changed)
    return dataclasses.replace(h, **{k: getattr(h, k).to(dev).clone().contiguous() for k in FIELDS})


def orbit(n=3):
    return [synth.orbit_camera(W, H, k, n) for k in range(n)]


def camera_entry(cam):
    """The ``cameras.json`` entry of a synthetic camera: camera-to-world pose, focal lengths from the tangents."""
    c2w = cam.world_view_transform.t().double().inverse()
    return dict(width=cam.image_width, height=cam.image_height, position=c2w[:3, 3].tolist(), rotation=c2w[:3, :3].tolist(),
                fx=0.5 * cam.image_width / cam.tanfovx, fy=0.5 * cam.image_height / cam.tanfovy)
