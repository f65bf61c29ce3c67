"""The SSIM loss restated in float64: the spec hgs.loss.ssim and csrc/ssim.hip are held to.

The standard definition of the reference's loss (tests/train_loop.ssim): an 11-tap Gaussian window, sigma 1.5,
normalised to sum 1, applied separably (one horizontal pass, then one vertical pass) with zero padding; C1 = 0.01^2,
C2 = 0.03^2; per channel and pixel
    mu = F[x],  sigma1^2 = F[x1^2] - mu1^2,  sigma2^2 = F[x2^2] - mu2^2,  sigma12 = F[x1 x2] - mu1 mu2,
    S = N1 N2 / (D1 D2),  N1 = 2 mu1 mu2 + C1,  N2 = 2 sigma12 + C2,  D1 = mu1^2 + mu2^2 + C1,  D2 = sigma1^2 + sigma2^2 + C2,
and the mean of S over every channel and pixel (or per image).  The backward is the analytic one of the kernels: with
the partials of S with respect to the filtered moments F[x1], F[x1^2], F[x1 x2]
    B = -S / D2,  Cc = 2 N1 / (D1 D2),  A = dS/dmu1 - 2 mu1 B - mu2 Cc,  dS/dmu1 = 2 mu2 N2 / (D1 D2) - 2 mu1 S / D1,
grad_x1 = g / count * (F[A] + 2 x1 F[B] + x2 F[Cc]) -- F is its own adjoint (a symmetric window, zero padding)."""
import torch
import torch.nn.functional as F

TAPS, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype=torch.float64):
    x = torch.arange(TAPS, dtype=dtype) - TAPS // 2
    g = torch.exp(-(x ** 2) / (2 * SIGMA ** 2))
    return g / g.sum()


def filt(t):
    """The separable Gaussian filter of the last two dimensions, zero padding, same size."""
    w = window(t.dtype).to(t.device)
    H, W = t.shape[-2:]
    r = TAPS // 2
    p = F.pad(t, (r, r, r, r))
    h = sum(w[k] * p[..., :, k:k + W] for k in range(TAPS))
    return sum(w[k] * h[..., k:k + H, :] for k in range(TAPS))


def _as4(x):
    return x if x.dim() == 4 else x[None]


def maps(x1, x2):
    """-> S, A, B, Cc per pixel, shape (N, C, H, W), float64."""
    x1, x2 = _as4(x1).double(), _as4(x2).double()
    mu1, mu2 = filt(x1), filt(x2)
    s1 = filt(x1 * x1) - mu1 * mu1
    s2 = filt(x2 * x2) - mu2 * mu2
    s12 = filt(x1 * x2) - mu1 * mu2
    n1, n2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    d1, d2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    S = n1 * n2 / (d1 * d2)
    B = -S / d2
    Cc = 2 * n1 / (d1 * d2)
    dmu1 = 2 * mu2 * n2 / (d1 * d2) - 2 * mu1 * S / d1
    A = dmu1 - 2 * mu1 * B - mu2 * Cc
    return S, A, B, Cc


def ssim(x1, x2, size_average=True):
    S = maps(x1, x2)[0]
    return S.mean() if size_average else S.mean(dim=(1, 2, 3))


def ssim_and_grad(x1, x2, size_average=True, grad_out=None):
    """-> (value, grad with respect to x1 in x1's shape), float64; grad_out: the upstream gradient (1 by default; a
    vector of N with size_average=False)."""
    S, A, B, Cc = maps(x1, x2)
    N = S.shape[0]
    a1, a2 = _as4(x1).double(), _as4(x2).double()
    if size_average:
        value = S.mean()
        g = torch.as_tensor(1.0 if grad_out is None else grad_out, dtype=torch.float64).reshape(1, 1, 1, 1) / S.numel()
    else:
        value = S.mean(dim=(1, 2, 3))
        g = (torch.ones(N, dtype=torch.float64) if grad_out is None else torch.as_tensor(grad_out).double())
        g = g.reshape(N, 1, 1, 1) / S[0].numel()
    grad = g * (filt(A) + 2 * a1 * filt(B) + a2 * filt(Cc))
    return value, grad.reshape(x1.shape)
