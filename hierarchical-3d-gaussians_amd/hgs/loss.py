"""Fused SSIM loss on the GPU: the reference's photometric loss with a HIP forward and backward.

A drop-in for ``utils/loss_utils.py`` of the reference (train_single.py:14, train_post.py:14, train_coarse.py:14,
render_hierarchy.py:16):

    from hgs.loss import l1_loss, ssim       # instead of: from utils.loss_utils import l1_loss, ssim

``ssim`` computes the standard SSIM of the reference's loss -- an 11x11 Gaussian window (sigma 1.5) applied separably,
zero padding, C1 = 0.01^2, C2 = 0.03^2 -- in one forward launch plus a fixed-order reduction (``hgs_ssim_fwd``,
``csrc/ssim.hip``) and one backward launch (``hgs_ssim_bwd``), on the caller's stream, with no host synchronisation.
Only the first image gets a gradient (the rendered one; the second is the ground truth).  Not supported: other window
sizes, dtypes other than float32, CPU tensors, double backward.  There is no fallback to the torch formula.

``photometric_loss`` is the whole loss of train_single.py:100-121, train_post.py:134-140 and
train_coarse.py:99-105 in one call -- the exposure transform and clamp of gaussian_renderer/__init__.py:115-118, the
alpha mask, L1, D-SSIM, the lambda mix and the inverse-depth L1 term -- with the gradients of the rendered image, the
exposure and the inverse depth (``hgs_photo_fwd`` / ``hgs_photo_bwd``, ``csrc/photometric.hip``).  INTEGRATION.md
shows the call for each script.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib


def l1_loss(network_output, gt):
    return torch.abs((network_output - gt)).mean()


def _check(img1, img2, window_size, size_average):
    if window_size != 11:
        raise ValueError(f"hgs.loss.ssim: window_size={window_size}; only the reference's 11 is supported")
    if not isinstance(img1, torch.Tensor) or not isinstance(img2, torch.Tensor):
        raise ValueError("hgs.loss.ssim: img1 and img2 must be tensors")
    if img1.shape != img2.shape:
        raise ValueError(f"hgs.loss.ssim: shapes differ: {tuple(img1.shape)} vs {tuple(img2.shape)}")
    if img1.dim() not in (3, 4):
        raise ValueError(f"hgs.loss.ssim: expected (C,H,W) or (N,C,H,W), got shape {tuple(img1.shape)}")
    if not size_average and img1.dim() != 4:
        raise ValueError("hgs.loss.ssim: size_average=False needs (N,C,H,W) input (the per-image mean of a (C,H,W) "
                         "image is undefined, as in the reference's formula)")
    if img2.requires_grad:
        raise ValueError("hgs.loss.ssim: img2 requires grad; only img1 (the rendered image) gets a gradient -- pass "
                         "the ground truth as img2, detached")
    for name, t in (("img1", img1), ("img2", img2)):
        if t.dtype != torch.float32:
            raise ValueError(f"hgs.loss.ssim: {name} has dtype {t.dtype}; only float32 is supported")
    for name, t in (("img1", img1), ("img2", img2)):
        if not t.is_cuda:
            raise ValueError(f"hgs.loss.ssim: {name} is on {t.device}; a GPU tensor is needed (no CPU fallback)")
    if img1.device != img2.device:
        raise ValueError(f"hgs.loss.ssim: devices differ: {img1.device} vs {img2.device}")


def _dims(x):
    return tuple(x.shape) if x.dim() == 4 else (1,) + tuple(x.shape)


def _stream_device(x):
    return C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream), x.device.index


def _forward(x1, x2, maps):
    """-> (per-image means [N], overall mean 0-d); ``maps`` (or None) receives the backward's per-pixel partials."""
    l = _lib.lib()
    N, Ch, H, W = _dims(x1)
    tmp_bytes = l.hgs_ssim_tmp_bytes(N, Ch, H, W)
    if tmp_bytes == 0:          # sizes refused (the reason is in hgs_last_error)
        raise _lib.HgsError(f"hgs_ssim_tmp_bytes: {l.hgs_last_error().decode()}", 1)
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=x1.device)
    per_image = torch.empty(N, dtype=torch.float32, device=x1.device)
    mean = torch.empty((), dtype=torch.float32, device=x1.device)
    stream, dev = _stream_device(x1)
    _lib.check(l.hgs_ssim_fwd(_lib.ptr(x1), _lib.ptr(x2), N, Ch, H, W, _lib.ptr(per_image), _lib.ptr(mean),
                              _lib.ptr(maps), _lib.ptr(tmp), stream, dev), "hgs_ssim_fwd")
    return per_image, mean


class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, size_average):
        maps = torch.empty((3,) + tuple(x1.shape), dtype=torch.float32, device=x1.device)
        per_image, mean = _forward(x1, x2, maps)
        ctx.save_for_backward(x1, x2, maps)
        ctx.size_average = size_average
        return mean if size_average else per_image

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x1, x2, maps = ctx.saved_tensors
        g = grad_out.to(torch.float32).contiguous()
        grad = torch.empty_like(x1)
        N, Ch, H, W = _dims(x1)
        stream, dev = _stream_device(x1)
        _lib.check(_lib.lib().hgs_ssim_bwd(_lib.ptr(x1), _lib.ptr(x2), _lib.ptr(maps), _lib.ptr(g),
                                           0 if ctx.size_average else 1, N, Ch, H, W, _lib.ptr(grad), stream, dev),
                   "hgs_ssim_bwd")
        return grad, None, None


def ssim(img1, img2, window_size=11, size_average=True):
    """Mean SSIM of img1 against img2, (C,H,W) or (N,C,H,W) float32 GPU tensors: a 0-d tensor, or with
    ``size_average=False`` (4-D input) the per-image means, shape (N,).  Differentiable with respect to img1."""
    _check(img1, img2, window_size, size_average)
    x1, x2 = img1.contiguous(), img2.contiguous()
    if torch.is_grad_enabled() and img1.requires_grad:
        return _SSIM.apply(x1, x2, bool(size_average))
    per_image, mean = _forward(x1, x2, None)
    return mean if size_average else per_image


class PhotometricLoss(NamedTuple):
    """0-d float32 tensors, views of one 4-float device buffer (so one host read can serve a progress bar).  Only
    ``loss`` carries a gradient."""
    loss: torch.Tensor
    l1: torch.Tensor
    ssim: torch.Tensor
    depth: torch.Tensor


def _plane(name, t, batched, N, H, W):
    """An (H,W) / (1,H,W) plane per image, with a leading N when batched -> contiguous [N,H,W]."""
    ok = [(N, H, W), (N, 1, H, W)] if batched else [(H, W), (1, H, W)]
    if tuple(t.shape) not in ok:
        raise ValueError(f"hgs.loss.photometric_loss: {name} has shape {tuple(t.shape)}; expected one of {ok}")
    return t.reshape(N, H, W).contiguous()


def _check_photo(rendered, gt, lambda_dssim, exposure, alpha_mask, depth, depth_weight):
    who = "hgs.loss.photometric_loss"
    named = [("rendered", rendered), ("gt", gt), ("exposure", exposure), ("alpha_mask", alpha_mask),
             ("invdepth", depth[0]), ("mono_invdepth", depth[1]), ("depth_mask", depth[2])]
    if not isinstance(rendered, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise ValueError(f"{who}: rendered and gt must be tensors")
    if any(t is not None and not isinstance(t, torch.Tensor) for _, t in named):
        raise ValueError(f"{who}: every optional input is a tensor or None")
    lam = float(lambda_dssim)
    if not (math.isfinite(lam) and 0.0 <= lam <= 1.0):
        raise ValueError(f"{who}: lambda_dssim={lambda_dssim} is not in [0, 1]")
    if not math.isfinite(float(depth_weight)):
        raise ValueError(f"{who}: depth_weight={depth_weight} is not finite")
    if rendered.shape != gt.shape:
        raise ValueError(f"{who}: shapes differ: rendered {tuple(rendered.shape)} vs gt {tuple(gt.shape)}")
    if rendered.dim() not in (3, 4):
        raise ValueError(f"{who}: expected (C,H,W) or (N,C,H,W), got shape {tuple(rendered.shape)}")
    if sum(t is not None for t in depth) not in (0, 3):
        raise ValueError(f"{who}: incomplete depth triple: invdepth, mono_invdepth and depth_mask are given all three "
                         "or none")
    N, Ch, H, W = _dims(rendered)
    if exposure is not None:
        if Ch != 3:
            raise ValueError(f"{who}: exposure needs C = 3, got C = {Ch}")
        want = (N, 3, 4) if rendered.dim() == 4 else (3, 4)
        if tuple(exposure.shape) != want:
            raise ValueError(f"{who}: exposure has shape {tuple(exposure.shape)}; expected {want}")
    for name, t in named:
        if t is not None and name not in ("rendered", "exposure", "invdepth") and t.requires_grad:
            raise ValueError(f"{who}: {name} requires grad; only rendered, exposure and invdepth get a gradient")
    for name, t in named:
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"{who}: {name} has dtype {t.dtype}; only float32 is supported")
    for name, t in named[2:]:
        if t is not None and name != "exposure":
            _plane(name, t, rendered.dim() == 4, N, H, W)
    for name, t in named:
        if t is not None and not t.is_cuda:
            raise ValueError(f"{who}: {name} is on {t.device}; a GPU tensor is needed (no CPU fallback)")
    for name, t in named:
        if t is not None and t.device != rendered.device:
            raise ValueError(f"{who}: devices differ: {name} on {t.device}, rendered on {rendered.device}")


def _photo_args(r, gt, E, mask, d, mono, md, lam, clamp, dw):
    N, Ch, H, W = _dims(r)
    p = lambda t: None if t is None else t.data_ptr()
    return _lib.PhotoArgs(rendered=p(r), gt=p(gt), exposure=p(E), alpha_mask=p(mask), invdepth=p(d),
                          mono_invdepth=p(mono), depth_mask=p(md), N=N, C=Ch, H=H, W=W, clamp=1 if clamp else 0,
                          reserved=0, lambda_dssim=lam, depth_weight=dw)


def _photo_tmp(r):
    l = _lib.lib()
    tmp_bytes = l.hgs_photo_tmp_bytes(*_dims(r))
    if tmp_bytes == 0:          # sizes refused (the reason is in hgs_last_error)
        raise _lib.HgsError(f"hgs_photo_tmp_bytes: {l.hgs_last_error().decode()}", 1)
    return torch.empty(tmp_bytes, dtype=torch.uint8, device=r.device)


def _photo_forward(tensors, scalars, maps):
    """-> the 4-float buffer (loss, L1, S, D); ``maps`` (or None) receives the backward's per-pixel partials."""
    r = tensors[0]
    args = _photo_args(*tensors, *scalars)
    tmp = _photo_tmp(r)
    out = torch.empty(4, dtype=torch.float32, device=r.device)
    stream, dev = _stream_device(r)
    _lib.check(_lib.lib().hgs_photo_fwd(C.byref(args), _lib.ptr(out), _lib.ptr(maps), _lib.ptr(tmp), stream, dev),
               "hgs_photo_fwd")
    return out


class _Photometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, E, d, gt, mask, mono, md, lam, clamp, dw):
        tensors = (r, gt, E, mask, d, mono, md)
        maps = torch.empty((3,) + tuple(r.shape), dtype=torch.float32, device=r.device)
        out = _photo_forward(tensors, (lam, clamp, dw), maps)
        ctx.save_for_backward(maps, *tensors)
        ctx.scalars = (lam, clamp, dw)
        loss, l1, s, depth = out.unbind(0)
        ctx.mark_non_differentiable(l1, s, depth)
        return loss, l1, s, depth

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        maps, *tensors = ctx.saved_tensors
        r, _, E, _, d, _, _ = tensors
        g = g.to(torch.float32).contiguous()
        need_r, need_E, need_d = ctx.needs_input_grad[:3]
        grad_r = torch.empty_like(r)      # always written: the kernel forms it on the way to the other two
        grad_E = torch.empty_like(E) if need_E else None
        grad_d = torch.empty_like(d) if need_d else None
        args = _photo_args(*tensors, *ctx.scalars)
        tmp = _photo_tmp(r)
        stream, dev = _stream_device(r)
        _lib.check(_lib.lib().hgs_photo_bwd(C.byref(args), _lib.ptr(maps), _lib.ptr(g), _lib.ptr(grad_r),
                                            _lib.ptr(grad_E), _lib.ptr(grad_d), _lib.ptr(tmp), stream, dev),
                   "hgs_photo_bwd")
        return (grad_r if need_r else None), grad_E, grad_d, None, None, None, None, None, None, None


def photometric_loss(rendered, gt, *, lambda_dssim, exposure=None, clamp=True, alpha_mask=None, invdepth=None,
                     mono_invdepth=None, depth_mask=None, depth_weight=0.0):
    """The reference's training loss in one call: per pixel and output channel j

        u_j = sum_i rendered_i * exposure[i, j] + exposure[j, 3]      (u = rendered without ``exposure``)
        v = u.clamp(0, 1) if clamp else u                             (the gradient passes where 0 <= u <= 1)
        x = v * alpha_mask
        loss = (1 - lambda_dssim) * mean|x - gt| + lambda_dssim * (1 - SSIM(x, gt))
               + depth_weight * mean|(invdepth - mono_invdepth) * depth_mask|

    ``rendered`` and ``gt`` are (C,H,W) or (N,C,H,W) float32 GPU tensors; ``alpha_mask``, ``invdepth``,
    ``mono_invdepth`` and ``depth_mask`` are (H,W) or (1,H,W) and ``exposure`` is (3,4) (C = 3) -- each with a leading N
    for a batch; the depth inputs come all three or not at all.  All means run over every element of the batch.
    Returns ``PhotometricLoss(loss, l1, ssim, depth)``; gradients go to ``rendered``, ``exposure`` and ``invdepth``."""
    depth = (invdepth, mono_invdepth, depth_mask)
    _check_photo(rendered, gt, lambda_dssim, exposure, alpha_mask, depth, depth_weight)
    batched = rendered.dim() == 4
    N, _, H, W = _dims(rendered)
    plane = lambda name, t: None if t is None else _plane(name, t, batched, N, H, W)
    r, g = rendered.contiguous(), gt.contiguous()
    E = None if exposure is None else exposure.contiguous()
    mask = plane("alpha_mask", alpha_mask)
    d, mono, md = plane("invdepth", invdepth), plane("mono_invdepth", mono_invdepth), plane("depth_mask", depth_mask)
    scalars = (float(lambda_dssim), bool(clamp), float(depth_weight))
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (r, E, d)):
        return PhotometricLoss(*_Photometric.apply(r, E, d, g, mask, mono, md, *scalars))
    return PhotometricLoss(*_photo_forward((r, g, E, mask, d, mono, md), scalars, None).unbind(0))
