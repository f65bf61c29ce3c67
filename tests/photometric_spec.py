"""The fused training loss restated in float64: the spec hgs.loss.photometric_loss and
csrc/photometric.hip are held to.

Per pixel p and output channel j, in the reference's order of operations (gaussian_renderer/__init__.py:115-118,
train_single.py:100-121):
    u_j = sum_i r_i E[i, j] + E[j, 3]        (u = r without an exposure)
    v   = min(max(u, 0), 1) with clamp       (the gradient passes where 0 <= u <= 1, both ends included, as torch.clamp)
    x   = v m                                (m: the alpha mask, broadcast over channels)
    L1 = mean |x - gt|  (d|t|/dt = sign t, sign 0 = 0),  S = SSIM(x, gt) (tests/ssim_spec.py),
    D  = mean |(d - d_mono) m_d|,            loss = (1 - lambda) L1 + lambda (1 - S) + depth_weight D.
All means run over every element of the batch.  The backward is the analytic one of the kernels:
    dx = -lambda g / count (F[A] + 2 x F[B] + gt F[Cc]) + (1 - lambda) g / count sign(x - gt)
    du = dx m [0 <= u <= 1],   grad_r_i = sum_j E[i, j] du_j,   grad_E[i, j] = sum_p r_i du_j,  grad_E[j, 3] = sum_p du_j,
    grad_d = depth_weight g / count_d sign(q) m_d,  q = (d - d_mono) m_d.
"""
import torch

import ssim_spec


def _batched(t, dims):
    """Optional input -> float64 with a leading N and, for planes, a channel axis of 1; None stays None."""
    if t is None:
        return None
    return t.double().reshape(dims)


def transform(r, exposure, clamp, mask):
    """r [N,C,H,W], exposure [N,3,4] or None, mask [N,1,H,W] or None -> u, x."""
    if exposure is None:
        u = r
    else:
        u = torch.einsum("nihw,nij->njhw", r, exposure[:, :, :3]) + exposure[:, :, 3][:, :, None, None]
    v = u.clamp(0, 1) if clamp else u
    return u, (v if mask is None else v * mask)


def loss_and_grads(rendered, gt, *, lambda_dssim, exposure=None, clamp=True, alpha_mask=None, invdepth=None,
                   mono_invdepth=None, depth_mask=None, depth_weight=0.0, grad_out=1.0):
    """-> dict(loss, l1, ssim, depth: 0-d float64; grad_rendered, grad_exposure, grad_invdepth in the inputs' shapes, the
    last two None without the input)."""
    four = rendered.dim() == 4
    r = (rendered if four else rendered[None]).double()
    t = (gt if four else gt[None]).double()
    N, C_, H, W = r.shape
    E = _batched(exposure, (N, 3, 4))
    m = _batched(alpha_mask, (N, 1, H, W))
    d, mono, md = (_batched(a, (N, 1, H, W)) for a in (invdepth, mono_invdepth, depth_mask))
    lam, g = float(lambda_dssim), float(grad_out)

    u, x = transform(r, E, clamp, m)
    count = x.numel()
    l1 = (x - t).abs().mean()
    S, A, B, Cc = ssim_spec.maps(x, t)
    s = S.mean()
    if d is None:
        depth = torch.zeros((), dtype=torch.float64)
    else:
        q = (d - mono) * md
        depth = q.abs().mean()
    loss = (1 - lam) * l1 + lam * (1 - s) + float(depth_weight) * depth

    f = ssim_spec.filt
    dx = -lam * g / count * (f(A) + 2 * x * f(B) + t * f(Cc)) + (1 - lam) * g / count * torch.sign(x - t)
    du = dx if m is None else dx * m
    if clamp:
        du = du * ((u >= 0) & (u <= 1))
    if E is None:
        grad_r, grad_E = du, None
    else:
        grad_r = torch.einsum("njhw,nij->nihw", du, E[:, :, :3])
        grad_E = torch.cat([torch.einsum("nihw,njhw->nij", r, du), du.sum(dim=(2, 3))[:, :, None]], dim=2)
        grad_E = grad_E.reshape(exposure.shape)
    grad_d = None if d is None else (float(depth_weight) * g / q.numel() * torch.sign(q) * md).reshape(invdepth.shape)
    return dict(loss=loss, l1=l1, ssim=s, depth=depth, grad_rendered=grad_r.reshape(rendered.shape),
                grad_exposure=grad_E, grad_invdepth=grad_d)


def bands(rendered, gt, *, exposure=None, clamp=True, alpha_mask=None, invdepth=None, mono_invdepth=None,
          depth_mask=None, clamp_band=1e-4, l1_band=1e-5, depth_band=1e-5):
    """The knife-edge pixels of the definition, as boolean masks (clamp [N,C,H,W], l1 [N,C,H,W], depth [N,1,H,W] or
    None): u within clamp_band of 0 or 1 without being exactly 0 or 1; 0 < |x - gt| < l1_band; 0 < |q| < depth_band.
    float32 and float64 may take different branches there."""
    four = rendered.dim() == 4
    r = (rendered if four else rendered[None]).double()
    t = (gt if four else gt[None]).double()
    N, C_, H, W = r.shape
    u, x = transform(r, _batched(exposure, (N, 3, 4)), clamp, _batched(alpha_mask, (N, 1, H, W)))
    near = lambda a, b: ((a - b).abs() < clamp_band) & (a != b)
    cb = (near(u, 0.0) | near(u, 1.0)) if clamp else torch.zeros_like(u, dtype=torch.bool)
    e = (x - t).abs()
    lb = (e > 0) & (e < l1_band)
    db = None
    if invdepth is not None:
        q = ((_batched(invdepth, (N, 1, H, W)) - _batched(mono_invdepth, (N, 1, H, W))) *
             _batched(depth_mask, (N, 1, H, W))).abs()
        db = (q > 0) & (q < depth_band)
    return cb, lb, db


def planes_ssim(ssim_fn):
    """tests/train_loop.ssim takes (C,H,W): a batch goes in as (N*C,H,W), the same per-channel planes and mean."""
    return lambda a, b: ssim_fn(a.reshape(-1, *a.shape[-2:]), b.reshape(-1, *b.shape[-2:]))


def torch_formula(rendered, gt, *, ssim_fn, lambda_dssim, exposure=None, clamp=True, alpha_mask=None, invdepth=None,
                  mono_invdepth=None, depth_mask=None, depth_weight=0.0):
    """The reference's own lines in plain torch, in the inputs' dtype and on their device, autograd-differentiable:
    gaussian_renderer/__init__.py:117-118 (exposure, clamp), train_single.py:104-117 (mask, L1, the lambda mix, the
    inverse-depth term).  -> (loss, l1, ssim, depth)."""
    image = rendered
    four = image.dim() == 4
    if exposure is not None:
        if four:
            image = torch.matmul(image.permute(0, 2, 3, 1), exposure[:, None, :3, :3]).permute(0, 3, 1, 2) \
                + exposure[:, :3, 3, None, None]
        else:
            image = torch.matmul(image.permute(1, 2, 0), exposure[:3, :3]).permute(2, 0, 1) + exposure[:3, 3, None, None]
    if clamp:
        image = image.clamp(0, 1)
    if alpha_mask is not None:
        image = image * alpha_mask.reshape(image.shape[:-3] + (1,) + image.shape[-2:])
    l1 = torch.abs(image - gt).mean()
    s = ssim_fn(image, gt)
    loss = (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - s)
    depth = torch.zeros((), dtype=rendered.dtype, device=rendered.device)
    if invdepth is not None:
        depth = torch.abs((invdepth - mono_invdepth) * depth_mask).mean()
        loss = loss + depth_weight * depth
    return loss, l1, s, depth
