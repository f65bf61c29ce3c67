"""Pointing at the picture: what every pixel of a render shows (csrc/pixels.hip).

``hgs.importance`` reads a forward from the Gaussians' side and ends in per-row arrays; this module reads it from the
pixels' side.  Per pixel: which row is in front, which is last, which carries the pixel (the largest blending weight
``alpha * T``), at which row the pixel becomes half opaque and how deep that row lies -- a *surface* depth, where the
blended inverse depth of the op is a mixture over everything along the ray::

    r = read_hierarchy_view(h, cam)                       # PixelReadout, ids are hierarchy nodes
    ids = pick(r, (x0, y0, x1, y1), which=("front",))     # "what do I see in this rectangle"
    pruned = prune_hierarchy_gpu(h, remove=leaves_below(h.nodes, ids))

``read_view`` is the one-view step on any rasterizer call (plain rows or an in-op LOD cut); ``python -m
hgs.pick_hierarchy`` is the command.  The planes come from the forward's workspaces: there is no CPU path for them;
``pick``, ``leaves_below``, ``world_points`` and ``node_depth_image`` are torch statements that work wherever their
arguments live."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

PLANES = ("alpha", "count", "front", "back", "heaviest", "wmax", "median", "median_depth")
ID_PLANES = ("front", "back", "heaviest", "median")


@dataclass
class PixelReadout:
    """The planes of one view, each [H, W] or None when it was not asked for.  Ids are slots (hierarchy nodes on the
    in-op LOD route), -1 where no row answers and -2 where the row that does has no slot."""
    alpha: Optional[torch.Tensor] = None          # float32  1 - final_T
    count: Optional[torch.Tensor] = None          # int32    rows blended at the pixel
    front: Optional[torch.Tensor] = None          # int32    the first blended row
    back: Optional[torch.Tensor] = None           # int32    the last one
    heaviest: Optional[torch.Tensor] = None       # int32    the row of the largest weight alpha * T (front-most on a tie)
    wmax: Optional[torch.Tensor] = None           # float32  that weight
    median: Optional[torch.Tensor] = None         # int32    the first row after which T < 0.5
    median_depth: Optional[torch.Tensor] = None   # float32  its view-space depth, 0 where there is none
    H: int = 0
    W: int = 0

    def numpy(self) -> dict:
        out = {name: getattr(self, name).cpu().numpy() for name in PLANES if getattr(self, name) is not None}
        out.update(H=np.int64(self.H), W=np.int64(self.W))
        return out


def read_view(raster_settings, means3D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
              cov3D_precomp=None, slot_of_row=None, n_slots=None, skybox_points=0, want=PLANES):
    """-> (PixelReadout, call) of one view: the no-grad forward ``hgs.importance.score_view`` makes (the in-op LOD route
    when ``raster_settings.render_indices`` is non-empty, the last ``skybox_points`` rows appended), then the readout
    on its workspaces.  ``slot_of_row``: int32 [P] over the op's rows; default: the row itself, and with a cut
    ``render_indices`` for the cut's entries and -1 for the skybox rows (read as -2), so that ids are hierarchy
    nodes.  ``want``: the planes to compute."""
    from diff_gaussian_rasterization import _C
    from .importance import _view_forward
    with torch.no_grad():
        res, slot_of_row = _view_forward(raster_settings, means3D, opacities, shs, colors_precomp, scales, rotations,
                                         cov3D_precomp, slot_of_row, skybox_points)
        call = res[-1]
        planes = _C.raster_pixels(call, slot_of_row=slot_of_row, n_slots=n_slots if slot_of_row is not None else None,
                                  want=want)
    return PixelReadout(H=call.H, W=call.W, **planes), call


def read_hierarchy_view(h, cam, tau_px=0.0, frustum=True, bounds=None, want=PLANES) -> PixelReadout:
    """The readout of ``h``'s node rows under ``cam`` at the cut of ``tau_px`` pixels (0: the leaves), as
    ``hgs.importance.score_hierarchy`` cuts and renders it; ids are nodes of ``h``.  An empty cut reads as nothing.
    ``bounds``: ``hgs.frustum.cull_bounds`` of the hierarchy when the caller has them already."""
    from .importance import _nodes_only, _settings, activated, tau_of, view_cut
    if not h.nodes.is_cuda:
        raise RuntimeError("read_hierarchy_view works on the GPU: upload the hierarchy first (there is no CPU path)")
    dev = h.nodes.device
    hn = _nodes_only(h)
    rows = activated(hn)
    if frustum and bounds is None:
        from .frustum import cull_bounds
        bounds = cull_bounds(h.nodes, rows["means3D"], rows["scales"])
    ri, pi, w, kids = view_cut(hn, cam, tau_of(tau_px, cam.tanfovx, cam.image_width), frustum, bounds)
    if ri.numel() == 0:
        return nothing(int(cam.image_height), int(cam.image_width), dev, want)
    rs = _settings(cam, dev, ri.contiguous(), pi.contiguous(), w.contiguous(), kids.contiguous())
    return read_view(rs, n_slots=h.num_nodes, want=want, **rows)[0]


def nothing(H, W, device="cpu", want=PLANES) -> PixelReadout:
    """The readout of a view that shows no row."""
    planes = {}
    for name in ((want,) if isinstance(want, str) else want):
        if name not in PLANES:
            raise ValueError(f"unknown plane {name!r}: one of {PLANES}")
        if name in ID_PLANES:
            planes[name] = torch.full((H, W), -1, dtype=torch.int32, device=device)
        else:
            planes[name] = torch.zeros((H, W), dtype=torch.int32 if name == "count" else torch.float32, device=device)
    return PixelReadout(H=H, W=W, **planes)


def region_mask(readout: PixelReadout, region) -> torch.Tensor:
    """bool [H, W] of ``region``: ``(x0, y0, x1, y1)`` half-open in pixels (clipped to the image), or a bool / uint8
    [H, W] mask (tensor or array; non-zero = inside)."""
    H, W = readout.H, readout.W
    if isinstance(region, (tuple, list)) and len(region) == 4 and not torch.is_tensor(region[0]):
        x0, y0, x1, y1 = (int(v) for v in region)
        m = torch.zeros((H, W), dtype=torch.bool)
        m[max(y0, 0):max(min(y1, H), 0), max(x0, 0):max(min(x1, W), 0)] = True
        return m
    m = torch.as_tensor(region)
    if m.dtype not in (torch.bool, torch.uint8) or tuple(m.shape) != (H, W):
        raise ValueError(f"region must be (x0, y0, x1, y1) or a bool / uint8 [{H}, {W}] mask, "
                         f"not {m.dtype} {tuple(m.shape)}")
    return m != 0


def pick(readout: PixelReadout, region, which=("front",)) -> torch.Tensor:
    """int64 [K]: the sorted unique non-negative ids the planes ``which`` hold inside ``region`` (see ``region_mask``);
    -1 (no row) and -2 (a row without a slot) are never picked.  Lives where the planes live."""
    which = (which,) if isinstance(which, str) else tuple(which)
    if not which or any(name not in ID_PLANES for name in which):
        raise ValueError(f"which must name planes of {ID_PLANES}, not {which}")
    found = []
    for name in which:
        plane = getattr(readout, name)
        if plane is None:
            raise ValueError(f"the readout holds no {name!r} plane")
        ids = plane[region_mask(readout, region).to(plane.device)].long()
        found.append(ids[ids >= 0])
    return torch.unique(torch.cat(found))


def leaves_below(nodes, ids) -> torch.Tensor:
    """uint8 [N]: the leaves in the subtrees of the nodes ``ids``; a leaf id marks itself.  The format
    ``hgs.hierarchy.prune_hierarchy_gpu(remove=...)`` and ``python -m hgs.prune_hierarchy --mask`` read.  Top-down over
    the depth column (a node inherits its parent's mark), so any numbering works; lives where ``nodes`` lives."""
    nodes = torch.as_tensor(nodes)
    if nodes.dim() != 2 or nodes.shape[1] != 7:
        raise ValueError(f"nodes must be [N,7], not {tuple(nodes.shape)}")
    N = nodes.shape[0]
    ids = torch.as_tensor(ids, dtype=torch.int64, device=nodes.device).reshape(-1)
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= N):
        raise ValueError(f"ids must lie in [0, {N}), got {int(ids.min())} .. {int(ids.max())}")
    marked = torch.zeros(N, dtype=torch.bool, device=nodes.device)
    marked[ids] = True
    if ids.numel():
        depth, parent = nodes[:, 0].long(), nodes[:, 1].long()
        for d in range(int(depth[ids].min()) + 1, int(depth.max()) + 1):
            level = (depth == d).nonzero().flatten()
            marked[level] |= marked[parent[level]]
    return (marked & (nodes[:, 6] == 0)).to(torch.uint8)


def world_points(readout: PixelReadout, cam) -> torch.Tensor:
    """float32 [H, W, 3]: every pixel's centre unprojected at ``median_depth`` through ``cam``'s view matrix
    (``world_view_transform``, row vectors, as the renderer takes it) -- the point where the pixel becomes half
    opaque; NaN where ``median == -1``."""
    if readout.median is None or readout.median_depth is None:
        raise ValueError("world_points needs the median and median_depth planes")
    d = readout.median_depth
    dev, H, W = d.device, readout.H, readout.W
    x = ((2.0 * torch.arange(W, dtype=torch.float64, device=dev) + 1.0) / W - 1.0) * float(cam.tanfovx)
    y = ((2.0 * torch.arange(H, dtype=torch.float64, device=dev) + 1.0) / H - 1.0) * float(cam.tanfovy)
    z = d.double()
    view = torch.stack((x[None, :] * z, y[:, None] * z, z, torch.ones_like(z)), dim=-1)
    world = view @ torch.linalg.inv(cam.world_view_transform.to(dev).double())
    out = (world[..., :3] / world[..., 3:]).float()
    out[readout.median == -1] = float("nan")
    return out


def node_depth_image(ids, nodes) -> torch.Tensor:
    """int32, the shape of ``ids``: the tree depth (``nodes[:, 0]``) of each pixel's node, -1 where the id names none
    (-1, -2): the debug view of an LOD cut."""
    nodes = torch.as_tensor(nodes)
    ids = torch.as_tensor(ids, device=nodes.device).long()
    if ids.numel() and int(ids.max()) >= nodes.shape[0]:
        raise ValueError(f"id {int(ids.max())} names no node of {nodes.shape[0]}")
    depth = nodes[:, 0].to(torch.int32)[ids.clamp(min=0)]
    return torch.where(ids >= 0, depth, torch.full_like(depth, -1))
