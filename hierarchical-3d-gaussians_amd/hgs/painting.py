"""Painting values into the picture: a number per row or per hierarchy node, blended with the weights of a render
(csrc/values.hip).

``hgs.importance`` scatters a per-pixel image onto rows and ``hgs.picking`` names the rows a pixel shows; this module
goes the other way: a table of values, one row per Gaussian or per hierarchy node, becomes an image in which every
pixel holds ``sum_k w_k v_k`` over the rows the renderer blended there, ``w = alpha * T`` -- the picture a render with
those values as colours would give, for any number of channels, without a second preprocess, binning and sort, and
with the table indexed by node through a cut's ``render_indices``::

    err = Attribution(...)                                      # python -m hgs.lod_error, or lod_error_hierarchy
    img = paint_hierarchy_view(h, cam, error_per_weight(err), tau_px=3.0, normalize=True)     # [1, H, W]: look at it
    lvl = paint_hierarchy_view(h, cam, node_levels(h.nodes), tau_px=3.0, normalize=True)      # the cut's tree levels

``paint_view`` is the one-view step on any rasterizer call (plain rows or an in-op LOD cut); ``python -m
hgs.paint_hierarchy`` is the command.  The image comes from the forward's workspaces: there is no CPU path for it; the
makers of per-node values (``node_levels``, ``node_extents``, ``node_opacities``, ``error_per_weight``) are torch
statements that work wherever their arguments live.

Not built: values of interior nodes derived from their leaves' values (pass a value for every node that can be in the
cut), several views per launch, and a flag of ``bench.py``."""
from __future__ import annotations

import math

import torch


def paint_view(raster_settings, values, means3D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
               cov3D_precomp=None, slot_of_row=None, background=None, want_wsum=False, skybox_points=0):
    """-> (out [C, H, W], wsum [H, W] or None, call) of one view: the no-grad forward ``hgs.importance.score_view``
    makes (the in-op LOD route when ``raster_settings.render_indices`` is non-empty, the last ``skybox_points`` rows
    appended), then ``values`` (float32 [S, C] or [S] on the device) blended on its workspaces.  ``slot_of_row``: int32
    [P] over the op's rows; default: the row itself, and with a cut ``render_indices`` for the cut's entries and -1 for
    the skybox rows (they occlude and add nothing), so that ``values`` is read per hierarchy node.  ``background``: None
    (zeros) or C floats; ``wsum``: the weights of the rows that have a slot."""
    from diff_gaussian_rasterization import _C
    from .importance import _view_forward
    with torch.no_grad():
        res, slot_of_row = _view_forward(raster_settings, means3D, opacities, shs, colors_precomp, scales, rotations,
                                         cov3D_precomp, slot_of_row, skybox_points)
        call = res[-1]
        got = _C.raster_values(call, values, slot_of_row=slot_of_row, background=background, want_wsum=want_wsum)
    out, wsum = got if want_wsum else (got, None)
    return out, wsum, call


def _node_values(values, N, dev):
    values = torch.as_tensor(values)
    if values.dim() not in (1, 2) or values.shape[0] != N:
        raise ValueError(f"values must be [N] or [N, C] with N = {N} nodes, not {tuple(values.shape)}")
    values = values.to(dev, torch.float32)
    return (values.reshape(N, 1) if values.dim() == 1 else values).contiguous()


def _background(background, C, dev):
    if background is None:
        return None
    bg = torch.as_tensor(background, dtype=torch.float32).reshape(-1).to(dev)
    if bg.numel() == 1 and C > 1:
        bg = bg.expand(C).contiguous()
    if bg.numel() != C:
        raise ValueError(f"background must hold one value, or one per channel ({C}), not {bg.numel()}")
    return bg


def paint_hierarchy_view(h, cam, values, tau_px=0.0, frustum=True, bounds=None, background=None, normalize=False,
                         fill=math.nan) -> torch.Tensor:
    """float32 [C, H, W]: ``values`` -- one row per NODE of ``h``, [N] or [N, C] -- blended into ``cam``'s view of the
    cut at ``tau_px`` pixels (0: the leaves), as ``hgs.importance.score_hierarchy`` cuts and renders it; the cut's
    ``render_indices`` are the map, so a pixel mixes the values of the nodes it shows.  ``background``: None (zeros),
    one value, or one per channel.  ``normalize``: divide by the sum of the weights where that is positive -- the
    weighted MEAN of the values under the pixel, which lies between the smallest and the largest of them -- and write
    ``fill`` where no node is blended.  An empty cut paints the background (``fill`` with ``normalize``).  ``bounds``:
    ``hgs.frustum.cull_bounds`` of the hierarchy when the caller has them already."""
    from .importance import _nodes_only, _settings, activated, tau_of, view_cut
    if not h.nodes.is_cuda:
        raise RuntimeError("paint_hierarchy_view works on the GPU: upload the hierarchy first (there is no CPU path)")
    dev, N = h.nodes.device, h.num_nodes
    values = _node_values(values, N, dev)
    C = int(values.shape[1])
    bg = _background(background, C, dev)
    H, W = int(cam.image_height), int(cam.image_width)
    hn = _nodes_only(h)
    rows = activated(hn)
    if frustum and bounds is None:
        from .frustum import cull_bounds
        bounds = cull_bounds(h.nodes, rows["means3D"], rows["scales"])
    ri, pi, w, kids = view_cut(hn, cam, tau_of(tau_px, cam.tanfovx, cam.image_width), frustum, bounds)
    if ri.numel() == 0:
        if normalize:
            return torch.full((C, H, W), float(fill), dtype=torch.float32, device=dev)
        out = torch.zeros((C, H, W), dtype=torch.float32, device=dev)
        return out if bg is None else out + bg[:, None, None]
    rs = _settings(cam, dev, ri.contiguous(), pi.contiguous(), w.contiguous(), kids.contiguous())
    out, wsum, _ = paint_view(rs, values, background=bg, want_wsum=normalize, **rows)
    if not normalize:
        return out
    seen = wsum > 0
    mean = out / torch.where(seen, wsum, torch.ones_like(wsum))
    return torch.where(seen, mean, torch.full_like(mean, float(fill)))


# ---- makers of per-node values ---------------------------------------------------------------------------------------
def node_levels(nodes) -> torch.Tensor:
    """float32 [N]: the tree depth of every node (``nodes[:, 0]``; the root is 0)."""
    nodes = torch.as_tensor(nodes)
    if nodes.dim() != 2 or nodes.shape[1] != 7:
        raise ValueError(f"nodes must be [N,7], not {tuple(nodes.shape)}")
    return nodes[:, 0].to(torch.float32)


def node_extents(boxes) -> torch.Tensor:
    """float32 [N]: the longest edge of every node's box (``boxes[:, 0, 3]``, the size the cut compares with the
    granularity)."""
    boxes = torch.as_tensor(boxes)
    if boxes.dim() != 3 or tuple(boxes.shape[1:]) != (2, 4):
        raise ValueError(f"boxes must be [N,2,4], not {tuple(boxes.shape)}")
    return boxes[:, 0, 3].to(torch.float32)


def node_opacities(h) -> torch.Tensor:
    """float32 [N]: the opacity the renderer takes from every node's row (``|alpha|``, as ``hgs.importance.activated``)."""
    return h.alpha[:h.num_nodes].abs().reshape(-1).to(torch.float32)


def error_per_weight(att) -> torch.Tensor:
    """float32 [N]: the mean error under every node, ``err / wsum``, and NaN where the node was never blended
    (``wsum == 0``).  ``att``: an ``hgs.importance.Attribution`` (its first channel), or a mapping with ``err`` and
    ``wsum`` -- the ``.npz`` ``python -m hgs.lod_error`` writes."""
    if hasattr(att, "acc"):
        err, wsum = att.acc[:, 0], att.wsum
    else:
        err, wsum = torch.as_tensor(att["err"]), torch.as_tensor(att["wsum"])
    if err.dim() != 1 or err.shape != wsum.shape:
        raise ValueError(f"err and wsum must be [N] both, not {tuple(err.shape)} and {tuple(wsum.shape)}")
    err, wsum = err.double(), wsum.double()
    seen = wsum != 0
    mean = err / torch.where(seen, wsum, torch.ones_like(wsum))
    return torch.where(seen, mean, torch.full_like(mean, math.nan)).to(torch.float32)
