"""Scores of Gaussians by what they blend into a set of views (csrc/contrib.hip).

Every removal criterion of ``hgs.hierarchy.prune_hierarchy_gpu`` is geometric or reads one attribute; this module makes
the mask the renderer itself would vote for.  Per Gaussian and over a set of views it collects the largest blending
weight ``w = alpha * T`` reached at any pixel, the sum of the weights and the number of pixels blended into::

    scores = score_hierarchy(h, cameras, tau_px=0.0)                    # Scores over the N nodes
    mask = low_contribution_mask(h.nodes, scores, max_weight_below=1 / 255)
    pruned = prune_hierarchy_gpu(h, remove=mask)

``score_view`` is the one-view step on any rasterizer call (plain rows or an in-op LOD cut); ``python -m
hgs.score_hierarchy`` is the command.  There is no CPU path for the scores: they come from the forward's workspaces."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch


@dataclass
class Scores:
    """Statistics of S slots over ``views`` views.  ``entries``: in how many views the slot was an op row."""
    wmax: torch.Tensor       # float32 [S] largest weight alpha * T at any counted pixel of any view
    wsum: torch.Tensor       # float64 [S] sum of the weights
    count: torch.Tensor      # int64 [S] (view, pixel) pairs blended into
    entries: torch.Tensor    # int64 [S]
    views: int = 0

    @staticmethod
    def zeros(S, device) -> "Scores":
        z = lambda dtype: torch.zeros(int(S), dtype=dtype, device=device)
        return Scores(z(torch.float32), z(torch.float64), z(torch.int64), z(torch.int64), 0)

    def merge(self, other: "Scores") -> "Scores":
        """The scores of both view sets (max / add); a new object."""
        if other.wmax.shape != self.wmax.shape:
            raise ValueError(f"Scores of {other.wmax.shape[0]} slots cannot be merged into {self.wmax.shape[0]}")
        return Scores(torch.maximum(self.wmax, other.wmax), self.wsum + other.wsum, self.count + other.count,
                      self.entries + other.entries, self.views + other.views)

    def numpy(self) -> dict:
        return dict(wmax=self.wmax.cpu().numpy(), wsum=self.wsum.cpu().numpy(), count=self.count.cpu().numpy(),
                    entries=self.entries.cpu().numpy(), views=np.int64(self.views))


def _view_forward(rs, means3D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp, slot_of_row,
                  skybox_points):
    """The forward ``score_view``, ``attribute_view`` and ``hgs.picking.read_view`` make (call it under no_grad):
    ``prepare_backward`` off; the in-op LOD route when ``rs.render_indices`` is non-empty, with the last
    ``skybox_points`` rows appended as the product path appends them.  -> (the op's result tuple, slot_of_row); a
    ``slot_of_row`` of None becomes, on the LOD route, the cut's ``render_indices`` with -1 for the skybox rows."""
    from diff_gaussian_rasterization import _C
    lod = rs.render_indices is not None and rs.render_indices.numel() > 0
    if lod:
        if colors_precomp is not None or cov3D_precomp is not None:
            raise RuntimeError("in-op LOD interpolation needs shs and scales/rotations (no precomputed colours/covariances)")
        n, K = int(rs.render_indices.numel()), int(skybox_points)
        w, kids = rs.interpolation_weights, rs.num_node_kids
        if K > 0:
            w = torch.cat((w[:n], torch.ones(K, dtype=w.dtype, device=w.device)))
            kids = torch.cat((kids[:n], torch.ones(K, dtype=kids.dtype, device=kids.device)))
        empty = rs.render_indices.new_empty(0)
        res = _C.rasterize_gaussians(
            rs.bg, means3D, None, opacities, scales, rotations, rs.scale_modifier, None, rs.viewmatrix, rs.projmatrix,
            rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, shs, rs.sh_degree, rs.campos, rs.prefiltered,
            rs.debug, empty, empty, w, kids, rs.do_depth, prepare_backward=False,
            lod=(rs.render_indices, rs.parent_indices, K))
        if slot_of_row is None:
            slot_of_row = torch.cat((rs.render_indices.to(torch.int32),
                                     torch.full((K,), -1, dtype=torch.int32, device=rs.render_indices.device)))
    else:
        res = _C.rasterize_gaussians(
            rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3D_precomp,
            rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, shs, rs.sh_degree,
            rs.campos, rs.prefiltered, rs.debug, rs.render_indices, rs.parent_indices, rs.interpolation_weights,
            rs.num_node_kids, rs.do_depth, prepare_backward=False)
    return res, slot_of_row


def score_view(scores: Scores, raster_settings, means3D, opacities, shs=None, colors_precomp=None, scales=None,
               rotations=None, cov3D_precomp=None, slot_of_row=None, pixel_mask=None, skybox_points=0):
    """One view into ``scores`` (in place): a no-grad forward of the rasterizer as ``GaussianRasterizer`` makes it
    (``prepare_backward`` off; the in-op LOD route when ``raster_settings.render_indices`` is non-empty, with the last
    ``skybox_points`` rows appended as the product path appends them), then the contribution call on its workspaces.
    ``slot_of_row``: int32 [P] over the op's rows; default: the row itself, and with a cut ``render_indices`` for the
    cut's entries and -1 (ignored) for the skybox rows.  ``pixel_mask``: uint8 [H*W], non-zero = counted.  Returns the
    forward's ``call``."""
    from diff_gaussian_rasterization import _C
    with torch.no_grad():
        res, slot_of_row = _view_forward(raster_settings, means3D, opacities, shs, colors_precomp, scales, rotations,
                                         cov3D_precomp, slot_of_row, skybox_points)
        call = res[-1]
        _C.raster_contributions(call, scores.wmax, scores.wsum, scores.count, slot_of_row=slot_of_row,
                                pixel_mask=pixel_mask)
        S = scores.entries.shape[0]
        if slot_of_row is None:
            scores.entries[:call.P] += 1
        else:
            s = slot_of_row.long()
            s = s[(s >= 0) & (s < S)]
            scores.entries[s] += 1          # (distinct by the precondition)
        scores.views += 1
    return call


def tau_of(tau_px, tanfovx, width):
    """The renderer's granularity for a target of ``tau_px`` pixels: 2 (tau_px + 0.5) tanfovx / (0.5 width)."""
    return (2.0 * (tau_px + 0.5)) * tanfovx / (0.5 * width)


def _settings(cam, dev, ri, pi, w, kids):
    import diff_gaussian_rasterization as dgr
    return dgr.GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
        bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev),
        projmatrix=cam.full_proj_transform.to(dev), sh_degree=3, campos=cam.camera_center.to(dev), prefiltered=False,
        debug=False, render_indices=ri, parent_indices=pi, interpolation_weights=w, num_node_kids=kids, do_depth=False)


def activated(h):
    """The attribute tensors the renderer takes from a hierarchy's rows (scene/gaussian_model.py in hierarchy mode: exp,
    normalize, abs)."""
    return dict(means3D=h.xyz.contiguous(), shs=h.shs.contiguous(), opacities=h.alpha.abs().reshape(-1, 1).contiguous(),
                scales=torch.exp(h.log_scales).contiguous(), rotations=torch.nn.functional.normalize(h.rots).contiguous())


def view_cut(h, cam, tau, frustum=True, bounds=None):
    """(render_indices, parent_indices, weights, kids) of one camera's cut at granularity ``tau``: ``hgs.frustum.cut_view``
    or, with ``frustum`` off, expand_to_size + get_interpolation_weights."""
    dev = h.nodes.device
    if frustum:
        from .frustum import cut_view, frustum_planes
        planes, rs = frustum_planes(cam.world_view_transform, cam.tanfovx, cam.tanfovy, cam.image_width, cam.image_height)
        cv = cut_view(h.nodes, h.boxes, bounds, tau, cam.camera_center.cpu(), planes, rs)
        return cv.render_indices, cv.parent_indices, cv.weights, cv.kids
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    N = h.num_nodes
    ri = torch.zeros(N, dtype=torch.int32, device=dev); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(N, device=dev); ns = torch.zeros(N, dtype=torch.int32, device=dev)
    n = expand_to_size(h.nodes, h.boxes, tau, cam.camera_center.to(dev), torch.zeros(3), ri, pi, ni)
    get_interpolation_weights(ni[:n], tau, h.nodes, h.boxes, cam.camera_center, torch.zeros(3), w, ns)
    return ri[:n], pi[:n], w[:n], ns[:n]


def score_hierarchy(h, cameras, tau_px=0.0, frustum=True, pixel_masks=None) -> Scores:
    """Scores of the N nodes of ``h`` (device tensors; rows behind the nodes are ignored) over ``cameras`` (objects with
    the fields of ``hgs.synth.Camera``).  Per camera: the cut at ``2 (tau_px + 0.5) tanfovx / (0.5 width)`` -- at
    ``tau_px = 0`` the leaves --, culled to the frustum unless ``frustum`` is off, rendered on the in-op LOD route, scored
    into the cut's ``render_indices``.  ``pixel_masks``: one uint8 [H*W] device tensor (or None) per camera."""
    if not h.nodes.is_cuda:
        raise RuntimeError("score_hierarchy works on the GPU: upload the hierarchy first (there is no CPU path)")
    dev, N = h.nodes.device, h.num_nodes
    cameras = list(cameras)
    if pixel_masks is not None and len(pixel_masks) != len(cameras):
        raise ValueError(f"{len(pixel_masks)} pixel masks for {len(cameras)} cameras")
    hn = h if h.xyz.shape[0] == N else type(h)(h.xyz[:N], h.shs[:N], h.alpha[:N], h.log_scales[:N], h.rots[:N], h.nodes, h.boxes)
    att = activated(hn)
    bounds = None
    if frustum:
        from .frustum import cull_bounds
        bounds = cull_bounds(h.nodes, att["means3D"], att["scales"])
    scores = Scores.zeros(N, dev)
    for k, cam in enumerate(cameras):
        ri, pi, w, kids = view_cut(hn, cam, tau_of(tau_px, cam.tanfovx, cam.image_width), frustum, bounds)
        if ri.numel() == 0:              # nothing of the hierarchy in this view
            scores.views += 1
            continue
        score_view(scores, _settings(cam, dev, ri.contiguous(), pi.contiguous(), w.contiguous(), kids.contiguous()),
                   pixel_mask=None if pixel_masks is None else pixel_masks[k], **att)
    return scores


def low_contribution_mask(nodes, scores: Scores, max_weight_below=None, sum_below=None, pixels_below=None, unseen="keep"):
    """uint8 [N] for ``prune_hierarchy_gpu(remove=...)`` / ``python -m hgs.prune_hierarchy --mask``: a LEAF (no children)
    is marked iff it was seen (``entries > 0``) and EVERY given criterion holds -- ``wmax < max_weight_below``,
    ``wsum < sum_below``, ``count < pixels_below``, all strict --; ``unseen="remove"`` also marks the leaves with
    ``entries == 0``.  Interior nodes are never marked.  Works where ``scores`` lives (device or host tensors); ``nodes``
    is moved there."""
    if max_weight_below is None and sum_below is None and pixels_below is None:
        raise ValueError("low_contribution_mask needs at least one of max_weight_below, sum_below, pixels_below")
    if unseen not in ("keep", "remove"):
        raise ValueError(f"unseen must be 'keep' or 'remove', not {unseen!r}")
    nodes = torch.as_tensor(nodes).to(scores.wmax.device)
    if nodes.dim() != 2 or nodes.shape[1] != 7 or nodes.shape[0] != scores.wmax.shape[0]:
        raise ValueError(f"nodes must be [N,7] with N = {scores.wmax.shape[0]} scored slots, not {tuple(nodes.shape)}")
    leaf = nodes[:, 6] == 0
    seen = scores.entries > 0
    low = seen.clone()
    if max_weight_below is not None:
        low &= scores.wmax < float(max_weight_below)
    if sum_below is not None:
        low &= scores.wsum < float(sum_below)
    if pixels_below is not None:
        low &= scores.count < pixels_below
    if unseen == "remove":
        low |= ~seen
    return (leaf & low).to(torch.uint8)


# ---- attribution of per-pixel images (csrc/attribute.hip) -----------------------------------------
@dataclass
class Attribution:
    """``acc[s, c] = sum over views and pixels of w * f_c`` for S slots and C channels, the weights' own sum and, as in
    ``Scores``, in how many views the slot was an op row::

        err = lod_error_hierarchy(h, cameras, tau_px=3.0)        # Attribution over the N nodes, C = 1
        worst = err.mean()[:, 0].argsort(descending=True)        # the nodes that stand in worst for what is below them
    """
    acc: torch.Tensor        # float64 [S, C]
    wsum: torch.Tensor       # float64 [S]
    entries: torch.Tensor    # int64 [S]
    views: int = 0

    @staticmethod
    def zeros(S, device, channels=1) -> "Attribution":
        if not 1 <= int(channels) <= 3:
            raise ValueError(f"1 to 3 channels can be attributed, not {channels}")
        return Attribution(torch.zeros(int(S), int(channels), dtype=torch.float64, device=device),
                           torch.zeros(int(S), dtype=torch.float64, device=device),
                           torch.zeros(int(S), dtype=torch.int64, device=device), 0)

    def merge(self, other: "Attribution") -> "Attribution":
        """The attribution over both view sets (sums); a new object."""
        if other.acc.shape != self.acc.shape:
            raise ValueError(f"an Attribution of shape {tuple(other.acc.shape)} cannot be merged into {tuple(self.acc.shape)}")
        return Attribution(self.acc + other.acc, self.wsum + other.wsum, self.entries + other.entries,
                           self.views + other.views)

    def mean(self) -> torch.Tensor:
        """``acc / wsum``, the weighted mean of the image under every slot; 0 where ``wsum == 0``.  float64 [S, C]."""
        seen = self.wsum != 0
        return torch.where(seen[:, None], self.acc / torch.where(seen, self.wsum, torch.ones_like(self.wsum))[:, None],
                           torch.zeros_like(self.acc))

    def numpy(self) -> dict:
        return dict(acc=self.acc.cpu().numpy(), wsum=self.wsum.cpu().numpy(), entries=self.entries.cpu().numpy(),
                    views=np.int64(self.views))


def attribute_view(att: Attribution, raster_settings, image, means3D, opacities, shs=None, colors_precomp=None,
                   scales=None, rotations=None, cov3D_precomp=None, slot_of_row=None, pixel_mask=None, skybox_points=0):
    """One view into ``att`` (in place): the no-grad forward ``score_view`` makes, on either of its routes, then the
    attribution call on its workspaces.  ``image``: float32 [C, H, W] (or [H, W] for C = 1) on the device, or a callable
    that takes the forward's rendered [3, H, W] and returns such a tensor -- an error image of the same forward without
    a second render.  ``slot_of_row``, ``pixel_mask``, ``skybox_points`` as for ``score_view``.  Returns the forward's
    ``call``."""
    from diff_gaussian_rasterization import _C
    with torch.no_grad():
        res, slot_of_row = _view_forward(raster_settings, means3D, opacities, shs, colors_precomp, scales, rotations,
                                         cov3D_precomp, slot_of_row, skybox_points)
        color, call = res[1], res[-1]
        f = image(color) if callable(image) else image
        _C.raster_attribute(call, f, att.acc, wsum=att.wsum, slot_of_row=slot_of_row, pixel_mask=pixel_mask)
        S = att.entries.shape[0]
        if slot_of_row is None:
            att.entries[:call.P] += 1
        else:
            s = slot_of_row.long()
            s = s[(s >= 0) & (s < S)]
            att.entries[s] += 1             # (distinct by the precondition)
        att.views += 1
    return call


def _nodes_only(h):
    N = h.num_nodes
    return h if h.xyz.shape[0] == N else type(h)(h.xyz[:N], h.shs[:N], h.alpha[:N], h.log_scales[:N], h.rots[:N], h.nodes, h.boxes)


def abs_error_image(target):
    """-> the callable ``attribute_view`` takes: the forward's render -> mean over the three channels of
    ``|render - target|``, float32 [1, H, W]."""
    return lambda color: (color - target).abs().mean(dim=0, keepdim=True)


def error_hierarchy(h, cameras, targets, tau_px=0.0, frustum=True, pixel_masks=None) -> Attribution:
    """Per-node photometric error of ``h`` over ``cameras`` against ``targets`` (one float32 [3, H, W] per camera, moved
    to the device): per camera ``score_hierarchy``'s cut and render, ``e = mean over the three channels of |render -
    target|`` (C = 1), attributed to the cut's ``render_indices``: ``acc[n, 0] = sum over views and pixels of w_n e``.
    ``mean()`` is the error an average pixel under node n shows."""
    if not h.nodes.is_cuda:
        raise RuntimeError("error_hierarchy works on the GPU: upload the hierarchy first (there is no CPU path)")
    dev, N = h.nodes.device, h.num_nodes
    cameras, targets = list(cameras), list(targets)
    if len(targets) != len(cameras):
        raise ValueError(f"{len(targets)} targets for {len(cameras)} cameras")
    if pixel_masks is not None and len(pixel_masks) != len(cameras):
        raise ValueError(f"{len(pixel_masks)} pixel masks for {len(cameras)} cameras")
    for k, (cam, t) in enumerate(zip(cameras, targets)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (3, int(cam.image_height), int(cam.image_width)):
            raise ValueError(f"target {k} must be a float32 tensor [3, {int(cam.image_height)}, {int(cam.image_width)}]")
    hn = _nodes_only(h)
    rows = activated(hn)
    bounds = None
    if frustum:
        from .frustum import cull_bounds
        bounds = cull_bounds(h.nodes, rows["means3D"], rows["scales"])
    att = Attribution.zeros(N, dev, channels=1)
    for k, cam in enumerate(cameras):
        ri, pi, w, kids = view_cut(hn, cam, tau_of(tau_px, cam.tanfovx, cam.image_width), frustum, bounds)
        if ri.numel() == 0:              # nothing of the hierarchy in this view
            att.views += 1
            continue
        attribute_view(att, _settings(cam, dev, ri.contiguous(), pi.contiguous(), w.contiguous(), kids.contiguous()),
                       abs_error_image(targets[k].to(dev)),
                       pixel_mask=None if pixel_masks is None else pixel_masks[k], **rows)
    return att


def render_hierarchy(h, cam, tau_px=0.0, frustum=True, bounds=None):
    """The no-grad render [3, H, W] of ``h``'s node rows at the cut of ``tau_px`` pixels on the in-op LOD route, as
    ``score_hierarchy`` renders it (a clone: a later forward cannot touch it); black when the cut is empty.  ``bounds``:
    ``hgs.frustum.cull_bounds`` of the hierarchy when the caller has them already."""
    from diff_gaussian_rasterization import _C
    dev = h.nodes.device
    hn = _nodes_only(h)
    rows = activated(hn)
    if frustum and bounds is None:
        from .frustum import cull_bounds
        bounds = cull_bounds(h.nodes, rows["means3D"], rows["scales"])
    ri, pi, w, kids = view_cut(hn, cam, tau_of(tau_px, cam.tanfovx, cam.image_width), frustum, bounds)
    if ri.numel() == 0:
        return torch.zeros(3, int(cam.image_height), int(cam.image_width), device=dev)
    rs = _settings(cam, dev, ri.contiguous(), pi.contiguous(), w.contiguous(), kids.contiguous())
    empty = ri.new_empty(0)
    with torch.no_grad():
        color = _C.rasterize_gaussians(
            rs.bg, rows["means3D"], None, rows["opacities"], rows["scales"], rows["rotations"], rs.scale_modifier, None,
            rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rows["shs"],
            rs.sh_degree, rs.campos, rs.prefiltered, rs.debug, empty, empty, rs.interpolation_weights, rs.num_node_kids,
            rs.do_depth, prepare_backward=False, lod=(rs.render_indices, rs.parent_indices, 0))[1]
    return color.clone()


def lod_error_hierarchy(h, cameras, tau_px, ref_tau_px=0.0, frustum=True) -> Attribution:
    """Where do the interior rows of ``h`` misrepresent what is below them?  ``error_hierarchy`` at ``tau_px`` whose
    targets are the same hierarchy rendered at the finer ``ref_tau_px`` (default 0: the leaves), no grad, each target
    cloned before the second forward.  With ``ref_tau_px == tau_px`` the error is zero everywhere."""
    if not h.nodes.is_cuda:
        raise RuntimeError("lod_error_hierarchy works on the GPU: upload the hierarchy first (there is no CPU path)")
    cameras = list(cameras)
    bounds = None
    if frustum:
        from .frustum import cull_bounds
        rows = activated(_nodes_only(h))
        bounds = cull_bounds(h.nodes, rows["means3D"], rows["scales"])
    targets = [render_hierarchy(h, cam, ref_tau_px, frustum, bounds) for cam in cameras]
    return error_hierarchy(h, cameras, targets, tau_px=tau_px, frustum=frustum)
