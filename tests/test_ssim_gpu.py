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


def yardstick(x1, x2, size_average):
    """float32 CPU: the reference's formula image by image, autograd for the gradient."""
    a = x1.clone().requires_grad_(True)
    if a.dim() == 3:
        v = tl.ssim(a, x2)
    else:
        per = torch.stack([tl.ssim(a[i], x2[i]) for i in range(a.shape[0])])
        v = per.mean() if size_average else per
    v.sum().backward()
    return v.detach(), a.grad


def errors(v, g, vs, gs):
    d = g.double().cpu() - gs
    return ((v.double().cpu() - vs).abs().max().item(), (d.norm() / gs.norm()).item(),
            d.abs().max().item() / gs.abs().max().item())


def hip(x1, x2, dev, size_average):
    from hgs import loss
    a = x1.to(dev).requires_grad_(True)
    v = loss.ssim(a, x2.to(dev), size_average=size_average)
    v.sum().backward()
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
