"""Fused SSIM loss on the GPU: the reference's photometric loss with a HIP forward and backward.

A drop-in for ``utils/loss_utils.py`` of the reference (train_single.py:14, train_post.py:14, train_coarse.py:14,
render_hierarchy.py:16):

    from hgs.loss import l1_loss, ssim       # instead of: from utils.loss_utils import l1_loss, ssim

``ssim`` computes the standard SSIM of the reference's loss -- an 11x11 Gaussian window (sigma 1.5) applied separably,
zero padding, C1 = 0.01^2, C2 = 0.03^2 -- in one forward launch plus a fixed-order reduction (``hgs_ssim_fwd``,
``csrc/ssim.hip``) and one backward launch (``hgs_ssim_bwd``), on the caller's stream, with no host synchronisation.
Only the first image gets a gradient (the rendered one; the second is the ground truth).  Not supported: other window
sizes, dtypes other than float32, CPU tensors, double backward.  There is no fallback to the torch formula.
"""
from __future__ import annotations

import ctypes as C

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
