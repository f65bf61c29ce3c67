"""Shared inputs of the frustum-cull tests: the 20 000-leaf trained-like hierarchy, the three cameras that look at it
from inside / past it, and the lerped cut entries pushed through the float32 geometry spec of K1."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import frustum_spec as fs
from boundary_fixtures import lod_lerp
from hgs import hierarchy, synth
from oracle import lod_oracle as lo
from oracle import raster_oracle as ro

W, H = 256, 160
TAUS_PX = (3.0, 40.0)


def yaw_camera(center, yaw_deg, width=W, height=H):
    """A camera at ``center`` turned by ``yaw_deg`` about the y axis (0: looking down +z)."""
    a = math.radians(yaw_deg)
    R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    return synth.make_camera(width, height, R=R, T=-R.T @ np.asarray(center, dtype=np.float64))


CAMERAS = {"A": ((0.0, 0.0, 0.0), 40.0), "B": ((0.0, 0.0, 10.0), 0.0), "C": ((0.0, 0.0, 10.0), 120.0)}


def camera(name):
    return yaw_camera(*CAMERAS[name])


def tau_of(cam, tau_px):
    """render_hierarchy.py:55-56: the granularity in pixels as a tangent-space size."""
    return (2 * (tau_px + 0.5)) * cam.tanfovx / (0.5 * cam.image_width)


@functools.lru_cache(maxsize=None)
def hier20k():
    """(Hierarchy, activated attribute dict for lod_lerp, bounds float32 [N,4]) -- built once per session."""
    h = hierarchy.build_hierarchy(synth.make_scene_trained_like(20000, synth.make_camera(W, H), seed=5))
    full = dict(xyz=h.xyz, scaling=torch.exp(h.log_scales), rotation=torch.nn.functional.normalize(h.rots),
                opacity=h.alpha.abs(), features=h.shs)
    bounds = fs.bounds_spec(h.nodes.numpy(), full["xyz"].numpy(), full["scaling"].numpy())
    return h, full, bounds


@functools.lru_cache(maxsize=None)
def unculled(cam_name, tau_px):
    """The unculled cut of one (camera, granularity) and K1's verdict on its lerped entries:
    dict(cam, tau, r, p, ni, w, kids, radii)."""
    h, full, _ = hier20k()
    cam = camera(cam_name)
    tau = tau_of(cam, tau_px)
    vp = cam.camera_center.numpy()
    nodes, boxes = h.nodes.numpy(), h.boxes.numpy()
    r, p, ni = lo.expand_to_size(nodes, boxes, tau, vp)
    w, kids = lo.get_interpolation_weights(ni, tau, nodes, boxes, vp)
    geo = {k: full[k] for k in ("xyz", "scaling", "rotation")}
    L = lod_lerp(geo, torch.from_numpy(r).long(), torch.from_numpy(p).long(), torch.from_numpy(w))
    q = torch.nn.functional.normalize(L["rotation"])
    g = ro.geometry_spec(L["xyz"].numpy(), L["scaling"].numpy(), q.numpy(), None, cam.world_view_transform.numpy(),
                         cam.full_proj_transform.numpy(), W, H, cam.tanfovx, cam.tanfovy)
    return dict(cam=cam, tau=tau, r=r, p=p, ni=ni, w=w, kids=kids, radii=g.radii)


def multi_row_case():
    """(nodes int32 [5,7], means [12,3], scales [12,3]): a hand-built node list with several rows per node, one node
    without rows and rows shared by nobody -- this project's builder always gives one row per node."""
    g = np.random.default_rng(3)
    means = g.normal(size=(12, 3)).astype(np.float32)
    scales = (np.exp(g.normal(size=(12, 3))) * 0.1).astype(np.float32)
    nodes = np.array([[0, -1, 0, 1, 2, 1, 2], [1, 0, 3, 4, 0, 3, 2], [1, 0, 7, 0, 1, 0, 0], [2, 1, 8, 3, 1, 0, 0],
                      [2, 1, 0, 0, 0, 0, 0]], dtype=np.int32)
    return nodes, means, scales


def flight_camera(k, n=6, center=(0.0, 0.0, 10.0), radius=3.0):
    """k-th of n views of a camera that flies a circle INSIDE the scene (in the x-z plane around ``center``) and looks
    where it is going: the budgeted viewer's case -- most of the scene is beside or behind every view, and every step
    moves the viewpoint, so the plain cut changes all around the camera."""
    a = 2.0 * math.pi * k / n
    pos = (center[0] + radius * math.sin(a), center[1], center[2] - radius * math.cos(a))
    return yaw_camera(pos, 90.0 - math.degrees(a))


def inside_orbit_camera(k, n=6, center=(0.0, 0.0, 15.0), radius=0.4, tilt=0.05):
    """k-th of n views on a small circle deep inside the scene, all looking roughly down +z (synth.orbit_camera moved
    to ``center``): the far quarter of the scene's depth range lies ahead, seen through a cone that is a small part of the
    scene's width there -- a few per cent of the leaves -- and everything else beside or behind."""
    a = 2.0 * math.pi * k / n
    pos = np.array([center[0] + radius * math.cos(a), center[1] + radius * math.sin(a), center[2]])
    yaw, pitch = tilt * math.cos(a), tilt * math.sin(a)
    Ry = np.array([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(pitch), -math.sin(pitch)], [0, math.sin(pitch), math.cos(pitch)]])
    R = Ry @ Rx
    return synth.make_camera(W, H, R=R, T=-R.T @ pos)
