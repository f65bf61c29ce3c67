"""The fused SSIM loss on the device (hgs.loss.ssim, csrc/ssim.hip) against the float64 spec (tests/ssim_spec.py).

Parity follows the project's "as good as float32" rule: the yardstick is the float32 CPU evaluation of the reference's
formula (tests/train_loop.ssim, value and autograd gradient); the kernels' errors against the spec may be at most
max(2e-6, 3x) the yardstick's for the value, 1.5x its relative L2 and 3x its largest deviation for the gradient."""
import pytest
import torch

import ssim_spec
import train_loop as tl

pytestmark = pytest.mark.gpu


def natural(C_, H, W, seed):
    """A smooth image with texture, noise and a flat block."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64),
                            indexing="ij")
    img = torch.stack([0.5 + 0.3 * torch.sin(7 * xx + 5 * yy + k) * torch.cos(11 * yy - 3 * xx) for k in range(C_)])
    img = img + 0.08 * torch.rand(C_, H, W, generator=g, dtype=torch.float64)
    img[:, H // 3: H // 3 + max(1, H // 4), W // 3: W // 3 + max(1, W // 4)] = 0.25
    return img.clamp(0, 1)


def pair(shape, seed=1):
    if len(shape) == 3:
        x1 = natural(*shape, seed)
        x2 = (0.8 * x1 + 0.2 * natural(*shape, seed + 1)).clamp(0, 1)
    else:
        x1 = torch.stack([natural(*shape[1:], seed + 10 * i) for i in range(shape[0])])
        x2 = torch.stack([(0.8 * x1[i] + 0.2 * natural(*shape[1:], seed + 10 * i + 1)).clamp(0, 1)
                          for i in range(shape[0])])
    return x1.float(), x2.float()


def yardstick(x1, x2, size_average, grad_out=None):
    """float32 CPU: the reference's formula image by image, autograd for the gradient (of v.sum(), or of
    (grad_out * v).sum())."""
    a = x1.clone().requires_grad_(True)
    if a.dim() == 3:
        v = tl.ssim(a, x2)
    else:
        per = torch.stack([tl.ssim(a[i], x2[i]) for i in range(a.shape[0])])
        v = per.mean() if size_average else per
    (v if grad_out is None else v * torch.as_tensor(grad_out, dtype=torch.float32)).sum().backward()
    return v.detach(), a.grad


def errors(v, g, vs, gs):
    d = g.double().cpu() - gs
    return ((v.double().cpu() - vs).abs().max().item(), (d.norm() / gs.norm()).item(),
            d.abs().max().item() / gs.abs().max().item())


def hip(x1, x2, dev, size_average, grad_out=None):
    from hgs import loss
    a = x1.to(dev).requires_grad_(True)
    v = loss.ssim(a, x2.to(dev), size_average=size_average)
    (v if grad_out is None else v * torch.as_tensor(grad_out, dtype=torch.float32).to(dev)).sum().backward()
    return v.detach(), a.grad


SHAPES = [((3, 1080, 1920), True), ((3, 37, 53), True), ((1, 8, 9), True), ((2, 3, 270, 480), True),
          ((2, 3, 270, 480), False), ((4, 64, 64), True)]


@pytest.mark.parametrize("shape,size_average", SHAPES)
def test_parity_with_the_spec(gpu, shape, size_average):
    x1, x2 = pair(shape)
    vs, gs = ssim_spec.ssim_and_grad(x1.double(), x2.double(), size_average=size_average)
    ye = errors(*yardstick(x1, x2, size_average), vs, gs)
    v, g = hip(x1, x2, gpu, size_average)
    assert v.shape == vs.shape and g.shape == x1.shape
    he = errors(v, g, vs, gs)
    print(f"{shape} size_average={size_average}: hip {he}, yardstick {ye}")
    assert he[0] <= max(2e-6, 3 * ye[0])
    assert he[1] <= 1.5 * ye[1]
    assert he[2] <= 3 * ye[2]


def test_two_calls_are_bit_identical_and_no_grad_matches(gpu):
    x1, x2 = pair((2, 3, 135, 241), seed=3)
    v1, g1 = hip(x1, x2, gpu, True)
    v2, g2 = hip(x1, x2, gpu, True)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    from hgs import loss
    with torch.no_grad():
        v0 = loss.ssim(x1.to(gpu), x2.to(gpu))
    assert torch.equal(v0, v1)
    p1, _ = hip(x1, x2, gpu, False)
    p0 = loss.ssim(x1.to(gpu), x2.to(gpu), size_average=False)       # no input requires grad: no maps
    assert torch.equal(p0, p1)


def test_reference_loss_expression_with_alpha_mask(gpu):
    """train_post.py:137-140: image * alpha_mask, 0.8 L1 + 0.2 (1 - SSIM), backward into the rendered image."""
    from hgs import loss
    x1, gt = pair((3, 120, 200), seed=5)
    mask = (torch.rand(1, 120, 200, generator=torch.Generator().manual_seed(9)) > 0.2).float()
    mask[:, :, :30] = 0

    def grads(ssim_fn, dev, dtype):
        img = x1.to(dev, dtype).clone().requires_grad_(True)
        image = img * mask.to(dev, dtype)
        t = gt.to(dev, dtype)
        Ll1 = loss.l1_loss(image, t)
        l = 0.8 * Ll1 + 0.2 * (1.0 - ssim_fn(image, t))
        l.backward()
        return l.detach().double().cpu(), img.grad.double().cpu()

    ls, gs = grads(lambda a, b: ssim_spec.ssim(a, b), "cpu", torch.float64)
    ly, gy = grads(tl.ssim, "cpu", torch.float32)
    lh, gh = grads(loss.ssim, gpu, torch.float32)
    assert abs(lh - ls).item() <= max(2e-6, 3 * abs(ly - ls).item())
    assert ((gh - gs).norm() / gs.norm()).item() <= 1.5 * ((gy - gs).norm() / gs.norm()).item()
    assert (gh - gs).abs().max().item() <= 3 * (gy - gs).abs().max().item()
    assert torch.all(gh[:, :, :30] == 0)


def test_training_with_the_fused_loss_matches_the_torch_formula(gpu, monkeypatch):
    """test_train_gpu's multi_tile_l1_dssim problem on the HIP renderer, once with train_loop.ssim and once with it
    replaced by hgs.loss.ssim, from the same jittered start."""
    from hgs import loss
    cams, scene = tl.make_problem(P=8000, size=320, height=192, n_views=6, seed=1)
    steps, dssim = 30, 0.2
    bg = torch.zeros(3)
    oracle = tl.oracle_render_fn(bg, 3, torch.float64)
    hipr = tl.hip_render_fn(bg, 3, gpu)
    with torch.no_grad():
        gt = {k: v.detach() for k, v in tl.activate(tl.raw_params_from_scene(scene, "cpu")).items()}
        targets = [oracle(c, gt) for c in cams]
    raw_t = tl.raw_params_from_scene(scene, gpu, jitter_seed=5)
    loss_t = tl.optimise(hipr, raw_t, cams, targets, steps, lambda_dssim=dssim)
    p_t = tl.evaluate(hipr, raw_t, cams, targets)
    monkeypatch.setattr(tl, "ssim", loss.ssim)
    raw_f = tl.raw_params_from_scene(scene, gpu, jitter_seed=5)
    loss_f = tl.optimise(hipr, raw_f, cams, targets, steps, lambda_dssim=dssim)
    p_f = tl.evaluate(hipr, raw_f, cams, targets)
    print(f"loss {loss_t[0]:.6f}->{loss_t[-1]:.6f} (torch SSIM) / {loss_f[0]:.6f}->{loss_f[-1]:.6f} (fused); "
          f"PSNR {p_t:.4f} / {p_f:.4f} dB")
    assert abs(loss_f[0] - loss_t[0]) <= 1e-5 * abs(loss_t[0])
    assert abs(p_f - p_t) <= 0.01


def test_rejections_on_the_device(gpu):
    from hgs import loss
    a, b = torch.rand(3, 16, 16, device=gpu), torch.rand(3, 16, 16, device=gpu)
    with pytest.raises(ValueError, match="float32"):
        loss.ssim(a.half(), b.half())
    with pytest.raises(ValueError, match="float32"):
        loss.ssim(a.double(), b.double())
    with pytest.raises(ValueError, match="shapes differ"):
        loss.ssim(a, b[:, :, :15])
    with pytest.raises(ValueError, match="only img1"):
        loss.ssim(a.clone().requires_grad_(True), b.clone().requires_grad_(True))


def test_non_contiguous_input(gpu):
    """A channels-last view is made contiguous; the gradient lands in the caller's layout."""
    from hgs import loss
    x1, x2 = pair((3, 40, 70), seed=7)
    base = x1.permute(1, 2, 0).contiguous().to(gpu)           # (H, W, C) storage
    a = base.permute(2, 0, 1).detach().requires_grad_(True)
    assert not a.is_contiguous()
    v = loss.ssim(a, x2.to(gpu))
    v.backward()
    vs, gs = ssim_spec.ssim_and_grad(x1.double(), x2.double())
    assert abs(v.item() - vs.item()) <= 2e-6
    assert ((a.grad.double().cpu() - gs).norm() / gs.norm()).item() <= 1e-4


# -- edges of the tiling, tiny and batched images, upstream gradients, degenerate content -----------------------------
# The kernels stage a 32x16 output tile plus a 5-pixel halo; the reduction walks C * tiles_per_plane partials per image.

EPS32 = torch.finfo(torch.float32).eps


def assert_within_yardstick(x1, x2, dev, size_average, grad_out=None, what=""):
    """The module's parity rule for one call, with an optional upstream gradient; -> (hip value, hip grad, spec grad)."""
    vs, gs = ssim_spec.ssim_and_grad(x1.double(), x2.double(), size_average=size_average, grad_out=grad_out)
    ye = errors(*yardstick(x1, x2, size_average, grad_out), vs, gs)
    v, g = hip(x1, x2, dev, size_average, grad_out)
    assert v.shape == vs.shape and g.shape == x1.shape
    he = errors(v, g, vs, gs)
    print(f"{what} {tuple(x1.shape)} size_average={size_average}: hip {he}, yardstick {ye}")
    assert he[0] <= max(2e-6, 3 * ye[0]), (what, he, ye)
    assert he[1] <= 1.5 * ye[1], (what, he, ye)
    assert he[2] <= 3 * ye[2], (what, he, ye)
    return v.cpu(), g.cpu(), gs


def content(kind, shape, seed):
    """x1, x2 of (C,H,W) or (N,C,H,W): "random" (uniform, x2 correlated with x1) or "smooth" (pair())."""
    if kind == "smooth":
        return pair(shape, seed)
    g = torch.Generator().manual_seed(seed)
    x1 = torch.rand(*shape, generator=g)
    x2 = (0.6 * x1 + 0.4 * torch.rand(*shape, generator=g)).clamp(0, 1)
    return x1, x2


# (H, W, C, N or None for 3-D, content): every W of {1, 2, 5, 6, 11, 31, 32, 33, 64, 65} and every H of
# {1, 2, 5, 6, 15, 16, 17, 33}, 1x1, 1xW and Hx1 among them -- single rows, single columns, images narrower or shorter
# than the window (the zero padding covers both sides of every window) and one pixel either side of the tile grid.
OFF_GRID = [(1, 1, 1, None, "random"), (1, 65, 3, None, "random"), (33, 1, 4, 2, "smooth"), (2, 2, 3, 2, "random"),
            (5, 5, 1, None, "smooth"), (6, 6, 4, None, "random"), (15, 11, 3, 2, "smooth"), (16, 31, 1, 2, "random"),
            (17, 32, 3, None, "random"), (33, 33, 4, 2, "random"), (16, 64, 3, None, "smooth"),
            (17, 65, 1, 2, "smooth"), (1, 32, 1, 2, "random"), (2, 33, 4, None, "smooth"), (5, 64, 3, 2, "random"),
            (6, 1, 3, None, "random"), (15, 2, 1, 2, "random"), (16, 5, 4, 2, "smooth"), (17, 6, 3, None, "random"),
            (33, 11, 1, None, "random"), (2, 31, 3, 2, "smooth"), (15, 65, 4, None, "random"),
            (33, 64, 3, 2, "smooth"), (6, 32, 1, 2, "random"), (1, 5, 3, 2, "smooth"), (16, 33, 3, None, "random")]


def test_off_grid_sweep_covers_every_size():
    assert {w for _, w, *_ in OFF_GRID} == {1, 2, 5, 6, 11, 31, 32, 33, 64, 65}
    assert {h for h, *_ in OFF_GRID} == {1, 2, 5, 6, 15, 16, 17, 33}
    hw = {(h, w) for h, w, *_ in OFF_GRID}
    assert (1, 1) in hw and any(h == 1 and w > 1 for h, w in hw) and any(w == 1 and h > 1 for h, w in hw)


@pytest.mark.parametrize("H,W,C_,N,kind", OFF_GRID)
def test_off_grid_and_tiny_images(gpu, H, W, C_, N, kind):
    shape = (C_, H, W) if N is None else (N, C_, H, W)
    x1, x2 = content(kind, shape, seed=H * 100 + W)
    for size_average in ((True,) if N is None else (True, False)):
        assert_within_yardstick(x1, x2, gpu, size_average, what=kind)


# Impulses: x mod 32 in {0, 4, 5, 26, 27, 31} and y mod 16 in {0, 4, 5, 10, 11, 15} put the 11x11 footprint across a
# seam of the 32x16 tiles (or a halo column / row just inside one); the rest sit on the four borders and corners.
IMP_C, IMP_H, IMP_W = 3, 60, 130          # 5 x 4 tiles, the last column and row partial
IMPULSES_1 = [(16, 32), (20, 36), (21, 37), (26, 58), (27, 59), (31, 63), (32, 96), (36, 100), (37, 101), (42, 122),
              (43, 123), (47, 127), (0, 0), (0, 69), (59, 90), (30, 0), (11, 129), (59, 129)]
IMPULSES_2 = [(y + 4, x + 5) if y + 4 < IMP_H and x + 5 < IMP_W else (y - 5, x - 4) for y, x in IMPULSES_1[::2]]


def _impulse_images():
    x1 = torch.zeros(IMP_C, IMP_H, IMP_W)
    x2 = torch.zeros(IMP_C, IMP_H, IMP_W)
    for i, (y, x) in enumerate(IMPULSES_1):
        x1[:, y, x] = torch.tensor([0.2 + 0.15 * i, 1.0 - 0.04 * i, 0.05 + 0.1 * (i % 5)])
    for i, (y, x) in enumerate(IMPULSES_2):
        x2[:, y, x] = torch.tensor([0.9 - 0.07 * i, 0.3 + 0.05 * i, 0.6])
    return x1, x2


def _far_from(points, H, W, d):
    """Pixels more than d (Chebyshev) from every point."""
    far = torch.ones(H, W, dtype=torch.bool)
    for y, x in points:
        far[max(0, y - d): y + d + 1, max(0, x - d): x + d + 1] = False
    return far


def test_impulses_on_seams_and_borders(gpu):
    """Single pixels on a zero background, x1's set and an offset set in x2.  Besides the parity rule, two exact facts:
    more than 10 pixels from every impulse of both images the gradient is exactly 0.0 -- the window of every pixel
    whose A, B, Cc reach it (5 pixels) sees only zeros (5 more), so mu = sigma = 0 there, A = 0 exactly, F[A] = 0 and
    x1 = x2 = 0 multiply F[B] and F[Cc] -- and it is non-zero wherever the spec's gradient exceeds 1e-6 of its largest
    value (tinier spec values may cancel to exactly zero in float32)."""
    x1, x2 = _impulse_images()
    assert {x % 32 for _, x in IMPULSES_1[:12]} == {0, 4, 5, 26, 27, 31}
    assert {y % 16 for y, _ in IMPULSES_1[:12]} == {0, 4, 5, 10, 11, 15}
    far = _far_from(IMPULSES_1 + IMPULSES_2, IMP_H, IMP_W, 10)
    assert int(far.sum()) >= 500, "the exact-zero check needs pixels far from every impulse"
    _, gs = ssim_spec.ssim_and_grad(x1.double(), x2.double())
    assert bool((gs[:, far] == 0).all()), "the spec's gradient must be exactly zero far from the impulses"
    assert bool((gs[:, ~far] != 0).any())
    _, g, gs = assert_within_yardstick(x1, x2, gpu, True, what="impulses")
    assert bool((g[:, far] == 0).all()), f"{int((g[:, far] != 0).sum())} non-zero gradients far from every impulse"
    big = gs.abs() > 1e-6 * gs.abs().max()
    assert bool((g[big] != 0).all()), f"{int((g[big] == 0).sum())} zero gradients where the spec's is not small"


def test_upstream_gradient_vector_per_image(gpu):
    """size_average=False, N = 5: grad_out = w = (0.7, 0, -1.3, 2.5, 1e-3), so image n's gradient is w[n] over C*H*W.
    Image 1's is exactly zero (0 times finite partials)."""
    x1, x2 = pair((5, 3, 37, 53), seed=11)
    w = torch.tensor([0.7, 0.0, -1.3, 2.5, 1e-3])
    _, g, _ = assert_within_yardstick(x1, x2, gpu, False, grad_out=w, what="w * ssim")
    assert bool((g[1] == 0).all())


def test_upstream_gradient_one_image_of_the_batch(gpu):
    """ssim(..., size_average=False)[3] alone: the other images' gradients are exactly zero."""
    from hgs import loss
    x1, x2 = pair((5, 3, 37, 53), seed=12)
    e3 = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0])
    _, g, _ = assert_within_yardstick(x1, x2, gpu, False, grad_out=e3, what="e3")
    a = x1.to(gpu).requires_grad_(True)
    loss.ssim(a, x2.to(gpu), size_average=False)[3].backward()        # the indexing path of autograd itself
    assert torch.equal(a.grad.cpu(), g)
    assert bool((g[[0, 1, 2, 4]] == 0).all())


def test_upstream_gradient_scalar_of_a_batch(gpu):
    """size_average=True on a 4-D batch with the loss 0.2 * (1 - ssim): grad_out = -0.2 over N*C*H*W."""
    from hgs import loss
    x1, x2 = pair((3, 3, 45, 67), seed=13)
    _, g, _ = assert_within_yardstick(x1, x2, gpu, True, grad_out=-0.2, what="0.2 (1 - ssim)")
    a = x1.to(gpu).requires_grad_(True)
    (0.2 * (1.0 - loss.ssim(a, x2.to(gpu)))).backward()
    assert torch.equal(a.grad.cpu(), g)


@pytest.mark.parametrize("shape", [(64, 3, 37, 53), (3, 3, 540, 960), (1, 1, 16, 32)])
def test_batches_and_the_reduction(gpu, shape):
    """Per-image means and the overall mean of many images, of images with more partials (C * tiles) than the
    reduction's 1024 threads, and of one image of one tile.  Noise grows with n: every image has its own SSIM."""
    N, C_, H, W = shape
    g = torch.Generator().manual_seed(N)
    x1 = torch.stack([natural(C_, H, W, seed=100 + n) for n in range(N)]).float()
    noise = torch.randn(shape, generator=g) * (0.005 * 1.07 ** torch.arange(N, dtype=torch.float32)).reshape(N, 1, 1, 1)
    x2 = (x1 + noise).clamp(0, 1)
    v, _, _ = assert_within_yardstick(x1, x2, gpu, False, what="batch")
    assert N == 1 or bool((v[1:] < v[:-1] - 1e-4).all()), "per-image SSIM must fall as the noise grows"
    assert_within_yardstick(x1, x2, gpu, True, what="batch mean")


def _salt_and_pepper(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x2 = natural(*shape, seed).float()
    u = torch.rand(shape, generator=g)
    x1 = torch.where(u < 0.05, torch.zeros(()), torch.where(u > 0.95, torch.ones(()), x2))
    return x1, x2


def _checkerboard(shape):
    C_, H, W = shape
    b = ((torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2).float().expand(C_, H, W).contiguous()
    return b, 1 - b


DEGENERATE = {
    "two_constants": lambda s: (torch.full(s, 0.8), torch.full(s, 0.3)),
    "above_one": lambda s: (3 * torch.rand(s, generator=torch.Generator().manual_seed(3)),
                            torch.rand(s, generator=torch.Generator().manual_seed(4))),
    "checkerboard_vs_inverse": _checkerboard,
    "salt_and_pepper": lambda s: _salt_and_pepper(s, 5),
}


@pytest.mark.parametrize("kind", list(DEGENERATE))
def test_degenerate_content(gpu, kind):
    """Flat images (sigma = 0 inside, the constants only at the borders), rendered values above 1, binary
    high-contrast images and impulse noise: the parity rule."""
    x1, x2 = DEGENERATE[kind]((3, 45, 67))
    assert_within_yardstick(x1, x2, gpu, True, what=kind)


def _cancellation_scale(x1, x2):
    """Per pixel, in float64: the sum of the absolute values of the terms whose float32 evaluation makes the kernels'
    gradient before the factor g / count -- the parts of A (2 mu2 N2 / (D1 D2), 2 mu1 S / D1, 2 mu1 B, mu2 Cc) under
    the window, 2 |x1| F[|B|] and |x2| F[|Cc|]."""
    a1, a2 = ssim_spec._as4(x1).double(), ssim_spec._as4(x2).double()
    f = ssim_spec.filt
    mu1, mu2 = f(a1), f(a2)
    s1, s2, s12 = f(a1 * a1) - mu1 * mu1, f(a2 * a2) - mu2 * mu2, f(a1 * a2) - mu1 * mu2
    n1, n2 = 2 * mu1 * mu2 + ssim_spec.C1, 2 * s12 + ssim_spec.C2
    d1, d2 = mu1 * mu1 + mu2 * mu2 + ssim_spec.C1, s1 + s2 + ssim_spec.C2
    S = n1 * n2 / (d1 * d2)
    B, Cc = -S / d2, 2 * n1 / (d1 * d2)
    a_parts = (2 * mu2 * n2 / (d1 * d2)).abs() + (2 * mu1 * S / d1).abs() + (2 * mu1 * B).abs() + (mu2 * Cc).abs()
    return (f(a_parts) + 2 * a1.abs() * f(B.abs()) + a2.abs() * f(Cc.abs())).reshape(x1.shape)


@pytest.mark.parametrize("kind", ["natural", "constant", "binary", "above_one"])
def test_identical_images(gpu, kind):
    """x1 == x2: S = 1 at every pixel and the gradient is zero (the maximum of SSIM) -- A = 0 and 2 x F[B] + x F[Cc] = 0
    exactly, so the kernels' gradient is pure float32 rounding of terms that cancel.  Bound: per pixel,
    64 eps32 * (1 / count) * T, T the sum of the absolute values of those terms (_cancellation_scale).  Each term passes
    through fewer than 100 roundings of at most eps32 / 2 relative each (two 11-tap passes for the moments, the map
    formulas, two 11-tap passes for F[A], F[B], F[Cc], the final combination), so the worst case of their sum is about
    50 eps32 T.  The value: 1 within 2e-6."""
    g = torch.Generator().manual_seed(7)
    shape = (2, 3, 45, 67)
    x = {"natural": lambda: torch.stack([natural(3, 45, 67, s) for s in (1, 2)]).float(),
         "constant": lambda: torch.full(shape, 0.37),
         "binary": lambda: (torch.rand(shape, generator=g) > 0.5).float(),
         "above_one": lambda: 3 * torch.rand(shape, generator=g)}[kind]()
    vs, gs = ssim_spec.ssim_and_grad(x.double(), x.double(), size_average=False)
    assert (vs - 1).abs().max().item() <= 1e-12
    bound = 64 * EPS32 * _cancellation_scale(x, x) / x[0].numel()
    assert bool((gs.abs() <= 1e-6 * bound).all()), "the spec's gradient is zero up to float64 rounding"
    for size_average in (True, False):
        v, gr = hip(x, x.clone(), gpu, size_average)
        v, gr = v.cpu(), gr.cpu().double()
        assert (v.double() - 1).abs().max().item() <= 2e-6, v
        b = bound / x.shape[0] if size_average else bound
        assert bool((gr.abs() <= b).all()), f"{kind}: |grad| / bound up to {(gr.abs() / b).max().item():.3g}"


def test_all_zero_images(gpu):
    """x1 = x2 = 0: mu = sigma = 0, S = C1 C2 / (C1 C2) = 1 (within 2e-6 after float32 rounding), and the gradient is
    exactly zero: A = 2*0*N2/(D1 D2) - 2*0*S/D1 - 2*0*B - 0*Cc = 0 and x1 = x2 = 0 multiply F[B] and F[Cc]."""
    x = torch.zeros(2, 3, 21, 40)
    for size_average in (True, False):
        v, gr = hip(x, x.clone(), gpu, size_average)
        assert (v.cpu().double() - 1).abs().max().item() <= 2e-6
        assert bool((gr == 0).all())


def test_callers_stream_gives_the_default_streams_bits(gpu):
    """x1 produced on a side stream behind queued work, and ssim + backward enqueued under torch.cuda.stream(s): the
    kernels run on the caller's stream without a synchronisation of their own, and the results equal the default
    stream's bit for bit."""
    from hgs import loss
    x1, x2 = pair((2, 3, 270, 480), seed=21)
    v0, g0 = hip(x1, x2, gpu, False)
    base, t2 = x1.to(gpu), x2.to(gpu)
    m = torch.rand(2048, 2048, device=gpu)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(gpu)
    with torch.cuda.stream(s):
        for _ in range(8):                            # work queued on the side stream ahead of x1
            m = m @ m / 2048.0
        a = base.clone().requires_grad_(True)
        v = loss.ssim(a, t2, size_average=False)
        v.sum().backward()
        v, g = v.detach().clone(), a.grad.clone()
    s.synchronize()
    assert torch.equal(v.cpu(), v0.cpu()) and torch.equal(g.cpu(), g0.cpu())
