"""Inputs of the fused-loss tests: natural-image-like float32 tensors with every optional
input, repaired so that no pixel sits on a knife edge of the definition, and the parity rule.

Knife edges: a pixel may take either branch in float32 and in float64 when u is within 1e-5 of 0 or 1 without being
exactly 0 or 1, when 0 < |x - gt| < 1e-6, or when 0 < |(d - d_mono) m_d| < 1e-6.  No test leaves pixels out.  Instead
``repair`` moves the inputs: +3e-3 on r at the clamp band, +1e-3 on gt at the L1 band, +1e-3 on d_mono at the depth band,
for bands ten times wider (1e-4 / 1e-5 / 1e-5), in float32, until the float64 spec finds the wide bands empty.  The exact
cases -- a zero background under an identity exposure, masked pixels with x == gt == 0, d == d_mono -- stay in and
exercise the inclusive clamp gate and sign(0) = 0."""
import torch

import photometric_spec as spec
import train_loop as tl

OPTIONAL = ("exposure", "alpha_mask", "invdepth", "mono_invdepth", "depth_mask")
FLOOR = 2.0 ** -22          # two float32 roundings of one result


def natural(C_, H, W, seed):
    """A smooth image with texture, noise and a flat block, float64 in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64),
                            indexing="ij")
    img = torch.stack([0.5 + 0.3 * torch.sin(7 * xx + 5 * yy + k) * torch.cos(11 * yy - 3 * xx) for k in range(C_)])
    img = img + 0.08 * torch.rand(C_, H, W, generator=g, dtype=torch.float64)
    img[:, H // 3: H // 3 + max(1, H // 4), W // 3: W // 3 + max(1, W // 4)] = 0.25
    return img.clamp(0, 1)


def _one(C_, H, W, seed, exposure, mask, depth, identity):
    g = torch.Generator().manual_seed(1000 + seed)
    a = natural(C_, H, W, seed)
    r = 2.0 * a - 0.55                                        # leaves [0, 1] on both sides: the clamp has work
    r[:, : max(1, H // 5), : max(1, W // 4)] = 0.0            # a background of exact zeros
    gt = (0.8 * a + 0.2 * natural(C_, H, W, seed + 1)).clamp(0, 1)
    out = dict(rendered=r, gt=gt)
    if exposure:
        E = torch.eye(3, 4, dtype=torch.float64)
        if not identity:
            E = E + 0.06 * torch.randn(3, 4, generator=g, dtype=torch.float64)
        out["exposure"] = E
    if mask:
        m = (torch.rand(1, H, W, generator=g) > 0.1).double()
        m[:, :, W - max(1, W // 6):] = 0.0
        m[:, H // 2: H // 2 + max(1, H // 8)] *= 0.5           # a soft edge
        out["alpha_mask"] = m
        gt[:, :, W - max(1, W // 12):] = 0.0                   # masked and black: x == gt == 0
    if depth:
        d = 0.2 + 0.15 * natural(1, H, W, seed + 2) + 0.01 * torch.rand(1, H, W, generator=g, dtype=torch.float64)
        mono = d + 0.05 * torch.randn(1, H, W, generator=g, dtype=torch.float64)
        mono[:, : max(1, H // 6)] = d[:, : max(1, H // 6)]     # q == 0 exactly
        md = (torch.rand(1, H, W, generator=g) > 0.15).double()
        out.update(invdepth=d, mono_invdepth=mono, depth_mask=md)
    return out


def make(shape, seed=1, exposure=True, mask=True, depth=True, identity=False, clamp=True):
    """float32 inputs of shape (C,H,W) or (N,C,H,W) as keyword arguments of the spec / photometric_loss (without
    lambda_dssim and depth_weight), repaired."""
    if len(shape) == 3:
        inp = _one(*shape, seed, exposure, mask, depth, identity)
    else:
        per = [_one(*shape[1:], seed + 10 * n, exposure, mask, depth, identity) for n in range(shape[0])]
        inp = {k: torch.stack([p[k] for p in per]) for k in per[0]}
    inp = {k: v.float() for k, v in inp.items()}
    inp["clamp"] = clamp
    return repair(inp)


def band_counts(inp):
    return tuple(0 if b is None else int(b.sum()) for b in spec.bands(**inp))


def repair(inp, rounds=8):
    """Moves r, gt and d_mono off the wide bands (see the module docstring), in float32; raises if `rounds` do not
    empty them."""
    inp = dict(inp)
    for _ in range(rounds):
        cb, lb, db = spec.bands(**inp)
        if not (cb.any() or lb.any() or (db is not None and db.any())):
            return inp
        shape = inp["rendered"].shape
        # u_j leans on r_j (the exposures used here are near the identity): move the band channel itself
        inp["rendered"] = (inp["rendered"] + 3e-3 * cb.reshape(shape).float()).float()
        inp["gt"] = (inp["gt"] + 1e-3 * lb.reshape(shape).float()).float()
        if db is not None:
            inp["mono_invdepth"] = (inp["mono_invdepth"] +
                                    1e-3 * db.reshape(inp["mono_invdepth"].shape).float()).float()
    raise AssertionError(f"the knife-edge bands are not empty after {rounds} repairs: {band_counts(inp)}")


def formula(inp, lambda_dssim, depth_weight, dtype, grads=("rendered", "exposure", "invdepth")):
    """The reference's torch lines (photometric_spec.torch_formula with tests/train_loop.ssim) on the CPU in `dtype`,
    autograd for the gradients -> dict like the spec's."""
    t = {k: (v.to(dtype).clone() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    leaves = {k: t[k].requires_grad_(True) for k in grads if t.get(k) is not None}
    loss, l1, s, depth = spec.torch_formula(ssim_fn=spec.planes_ssim(tl.ssim), lambda_dssim=lambda_dssim,
                                            depth_weight=depth_weight, **t)
    loss.backward()
    out = dict(loss=loss.detach(), l1=l1.detach(), ssim=s.detach(), depth=depth.detach())
    for k in ("rendered", "exposure", "invdepth"):
        out["grad_" + k] = leaves[k].grad if k in leaves else None
    return out


def fused(inp, lambda_dssim, depth_weight, dev, grads=("rendered", "exposure", "invdepth")):
    """hgs.loss.photometric_loss on `dev` + backward -> dict like the spec's (CPU tensors)."""
    from hgs import loss
    t = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    leaves = {k: t[k].requires_grad_(True) for k in grads if t.get(k) is not None}
    res = loss.photometric_loss(t.pop("rendered"), t.pop("gt"), lambda_dssim=lambda_dssim, depth_weight=depth_weight, **t)
    res.loss.backward()
    out = {k: getattr(res, k).detach().cpu() for k in ("loss", "l1", "ssim", "depth")}
    for k in ("rendered", "exposure", "invdepth"):
        out["grad_" + k] = leaves[k].grad.cpu() if k in leaves else None
    return out


def assert_parity(got, yard, want, what=""):
    """The project's float32-yardstick rule: `got` (the kernels) against `want` (the float64 spec) may err at most
    max(2e-6, 3x) the float32 yardstick's error for each of the four values, max(2^-22, 1.5x) its relative L2 and
    max(2^-22, 3x) its largest deviation over the spec's maximum for each gradient.  Prints every figure first."""
    fails = []
    for k in ("loss", "l1", "ssim", "depth"):
        e, y = abs(float(got[k]) - float(want[k])), abs(float(yard[k]) - float(want[k]))
        print(f"{what} {k}: spec {float(want[k]):.9f} hip err {e:.3e} yardstick err {y:.3e}")
        if not e <= max(2e-6, 3 * y):
            fails.append((k, e, y))
    for k in ("grad_rendered", "grad_exposure", "grad_invdepth"):
        if want[k] is None:
            assert got[k] is None
            continue
        w = want[k].double()
        assert got[k].shape == w.shape, (k, got[k].shape, w.shape)
        dg, dy = got[k].double() - w, yard[k].double() - w
        scale_l2, scale_max = max(w.norm().item(), 1e-300), max(w.abs().max().item(), 1e-300)
        l2, yl2 = dg.norm().item() / scale_l2, dy.norm().item() / scale_l2
        mx, ymx = dg.abs().max().item() / scale_max, dy.abs().max().item() / scale_max
        print(f"{what} {k}: rel L2 hip {l2:.3e} yardstick {yl2:.3e}; max/max hip {mx:.3e} yardstick {ymx:.3e}")
        if not l2 <= max(FLOOR, 1.5 * yl2):
            fails.append((k, "l2", l2, yl2))
        if not mx <= max(FLOOR, 3 * ymx):
            fails.append((k, "max", mx, ymx))
    assert not fails, (what, fails)
