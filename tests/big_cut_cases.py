"""Shared inputs of tests/test_big_cuts_gpu.py: ONE hierarchy whose workgroup sums need a second chunk of the chained
scan (csrc/common.h: kScanChunk = 8192 sums of 256 nodes each, so from 2 097 153 nodes upward), the views the cuts are
taken from, and their expected cuts from tests/big_cut_spec.py -- each built once per process.

1 050 000 leaves give N = 2 099 999 nodes = 8 204 workgroup sums, 12 of them in the second chunk.  The builder numbers
level by level, so the 2 847 nodes at or behind index 2 097 152 are leaves of the deepest level, scattered through the
scene: whether one of them emits, and whether the cull keeps it, depends on the view as for any other leaf."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

import big_cut_spec as bg
import budget_cut_spec as bs
import frustum_cases as fc
from hgs import hierarchy, synth

LEAVES = 1_050_000
NODES = 2 * LEAVES - 1
SCAN_CHUNK = 8192                          # workgroup sums per scan workgroup (kScanChunk)
SEAM = SCAN_CHUNK * 256                    # the first node whose workgroup sum lies in the second chunk
HIST_SEAM = 2048 * 256                     # the first node of budget_hist_kernel's second grid-stride step (kHistGrid)
CAMERAS = ("B", "C", "O")                  # O: frustum_cases.inside_orbit_camera(0), deep inside the scene
TAUS_PX = (-0.5, 3.0, 15.0)                # -0.5 px is tau = 0: every leaf


def camera(name):
    """B, C: frustum_cases' cameras; O: the inside orbit's first; away: behind the scene, looking away from it."""
    if name == "away":
        return fc.yaw_camera((0.0, 0.0, -50.0), 180.0)
    return fc.inside_orbit_camera(0) if name == "O" else fc.camera(name)


def build(device):
    """The hierarchy on ``device`` -> (nodes int32 [N,7], boxes [N,2,4], means [N,3], activated scales [N,3])."""
    h = hierarchy.build_hierarchy_on_device(LEAVES, synth.make_camera(fc.W, fc.H), device, seed=2, sh_degree=0)
    return h.nodes, h.boxes, h.xyz.contiguous(), torch.exp(h.log_scales).contiguous()


@functools.lru_cache(maxsize=None)
def big():
    """nodes, boxes, means, scales, bounds on the GPU (the bounds made there), host copies nodes_h, boxes_h, bounds_h."""
    from hgs.frustum import cull_bounds
    nodes, boxes, means, scales = build(torch.device("cuda:0"))
    bounds = cull_bounds(nodes, means, scales)
    torch.cuda.empty_cache()               # (the builder's SH block and temporaries)
    f = SimpleNamespace(nodes=nodes, boxes=boxes, means=means, scales=scales, bounds=bounds, N=int(nodes.shape[0]),
                        nodes_h=nodes.cpu().numpy(), boxes_h=boxes.cpu().numpy(), bounds_h=bounds.cpu().numpy())
    assert f.N == NODES and (f.N + 255) // 256 == 8204 and (f.N + 255) // 256 - SCAN_CHUNK == 12
    return f


@functools.lru_cache(maxsize=None)
def view(name, tau_px):
    """One view's arguments: dict(cam, tau, vp [3], planes [5,4], rs), all on the host."""
    from hgs.frustum import frustum_planes
    cam = camera(name)
    planes, rs = frustum_planes(cam.world_view_transform, cam.tanfovx, cam.tanfovy, fc.W, fc.H)
    return dict(cam=cam, tau=fc.tau_of(cam, tau_px), vp=cam.camera_center.clone(), planes=planes, rs=rs)


@functools.lru_cache(maxsize=None)
def host_view(name, culled):
    """The ``budget_cut_spec.View`` of a camera on the fixture's host copies; its sizes nest."""
    f, v = big(), view(name, 3.0)
    hv = (bs.View(f.nodes_h, f.boxes_h, v["vp"].numpy(), f.bounds_h, v["planes"].numpy(), v["rs"]) if culled
          else bs.View(f.nodes_h, f.boxes_h, v["vp"].numpy()))
    assert hv.nested()
    return hv


@functools.lru_cache(maxsize=None)
def events(name, culled, cost):
    return bs.Events(host_view(name, culled), cost)


@functools.lru_cache(maxsize=None)
def raw_spec(name, tau_px, culled):
    """The expected cut of one view, whatever it holds (``spec`` is this behind the seam conditions)."""
    return bg.nested_cut_spec(host_view(name, culled), view(name, tau_px)["tau"])


@functools.lru_cache(maxsize=None)
def seam_counts(name, tau_px):
    """What the spec says the second scan chunk holds for this view: dict(entries, emit_lo, emit_hi, kept_lo, kept_hi,
    culled_hi) -- the unculled entries, the emitting nodes in front of / at or behind SEAM, and those the cull keeps."""
    ni = raw_spec(name, tau_px, False)["node_indices"]         # one row per node here: entries are nodes
    keep = host_view(name, True).kept[ni]
    hi = ni >= SEAM
    return dict(entries=int(ni.shape[0]), emit_lo=int((~hi).sum()), emit_hi=int(hi.sum()), kept_lo=int((keep & ~hi).sum()),
                kept_hi=int((keep & hi).sum()), culled_hi=int((~keep & hi).sum()))


def spec(name, tau_px, culled):
    """The expected cut (big_cut_spec.nested_cut_spec).  Whoever takes one has the seam exercised: camera B at 3 px has
    at least 500 emitting nodes behind it, 100 of them kept and 100 culled; every other view has emitting nodes on both
    sides, and kept ones on both sides where there is a cull."""
    c = seam_counts(name, tau_px)
    if (name, tau_px) == ("B", 3.0):
        assert c["emit_hi"] >= 500 and c["kept_hi"] >= 100 and c["culled_hi"] >= 100, c
    assert c["emit_lo"] >= 1 and c["emit_hi"] >= 1, (name, tau_px, c)
    assert not culled or (c["kept_lo"] >= 1 and c["kept_hi"] >= 1), (name, tau_px, c)
    return raw_spec(name, tau_px, culled)
