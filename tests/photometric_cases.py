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


def formula(inp, lambda_dssim, depth_weight, dtype, grads=("rendered", "exposure", "invdepth"), weight=None):
    """The reference's torch lines (photometric_spec.torch_formula with tests/train_loop.ssim) on the CPU in `dtype`,
    autograd for the gradients (of the loss, or of ``weight * loss``) -> dict like the spec's."""
    t = {k: (v.to(dtype).clone() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    leaves = {k: t[k].requires_grad_(True) for k in grads if t.get(k) is not None}
    loss, l1, s, depth = spec.torch_formula(ssim_fn=spec.planes_ssim(tl.ssim), lambda_dssim=lambda_dssim,
                                            depth_weight=depth_weight, **t)
    (loss if weight is None else weight * loss).backward()
    out = dict(loss=loss.detach(), l1=l1.detach(), ssim=s.detach(), depth=depth.detach())
    for k in ("rendered", "exposure", "invdepth"):
        out["grad_" + k] = leaves[k].grad if k in leaves else None
    return out


def fused(inp, lambda_dssim, depth_weight, dev, grads=("rendered", "exposure", "invdepth"), weight=None):
    """hgs.loss.photometric_loss on `dev` + backward (of the loss, or of ``weight * loss``) -> dict like the spec's
    (CPU tensors)."""
    from hgs import loss
    t = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    leaves = {k: t[k].requires_grad_(True) for k in grads if t.get(k) is not None}
    res = loss.photometric_loss(t.pop("rendered"), t.pop("gt"), lambda_dssim=lambda_dssim, depth_weight=depth_weight, **t)
    (res.loss if weight is None else weight * res.loss).backward()
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


# -- small and awkward images (tests/test_photometric_edges_gpu.py) -----------------------------------------------------
# `make` lays its special regions out as strips (W - max(1, W // 6) masked columns, max(1, H // 6) rows with q == 0), so
# at W = 1 its mask is all zero and at H = 1 its depth term has no gradient.  `small` places single pixels instead.

# (H, W, C, N or None for (C,H,W), content): the sizes of test_ssim_gpu.OFF_GRID -- every W of
# {1, 2, 5, 6, 11, 31, 32, 33, 64, 65} and every H of {1, 2, 5, 6, 15, 16, 17, 33}; 1x1, 1xW and Hx1; single rows and
# columns, images smaller than the window and one pixel either side of the 32x16 tile grid.  C = 3 comes with a
# per-image exposure, C in {1, 2, 4} without one.
SWEEP = [(1, 1, 1, None, "random"), (1, 65, 3, None, "random"), (33, 1, 4, 2, "smooth"), (2, 2, 3, 2, "random"),
         (5, 5, 2, None, "smooth"), (6, 6, 4, None, "random"), (15, 11, 3, 2, "smooth"), (16, 31, 2, 2, "random"),
         (17, 32, 3, None, "random"), (33, 33, 4, 2, "random"), (16, 64, 3, None, "smooth"),
         (17, 65, 1, 2, "smooth"), (1, 32, 1, 2, "random"), (2, 33, 4, None, "smooth"), (5, 64, 3, 2, "random"),
         (6, 1, 3, None, "random"), (15, 2, 1, 2, "random"), (16, 5, 4, 2, "smooth"), (17, 6, 3, None, "random"),
         (33, 11, 2, None, "random"), (2, 31, 3, 2, "smooth"), (15, 65, 4, None, "random"),
         (33, 64, 3, 2, "smooth"), (6, 32, 2, 2, "random"), (1, 5, 3, 2, "smooth"), (16, 33, 3, None, "random"),
         (1, 1, 3, None, "random"), (1, 1, 3, 2, "smooth")]
ROLES = 7                   # pixels `small` needs for one of each kind


def sweep_case(H, W, C_, N, content):
    return small((C_, H, W) if N is None else (N, C_, H, W), seed=H * 100 + W, content=content)


def _three_levels(shape, g, p0, p_half):
    """Values in {0, 0.5, 1} with probabilities p0, p_half and the rest, float64."""
    u = torch.rand(shape, generator=g)
    return 0.5 * (u >= p0).double() + 0.5 * (u >= p0 + p_half).double()


def _small_one(C_, H, W, seed, content, kind, exposure, mask, depth):
    g = torch.Generator().manual_seed(2000 + seed)
    if content == "smooth":
        a = natural(C_, H, W, seed)
        r = 2.0 * a - 0.55
        gt = (0.8 * a + 0.2 * natural(C_, H, W, seed + 1)).clamp(0, 1)
    else:
        assert content == "random", content
        a = torch.rand(C_, H, W, generator=g, dtype=torch.float64)
        r = 1.6 * a - 0.3
        gt = (0.6 * a + 0.4 * torch.rand(C_, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    # One pixel of each kind at distinct random places.  `live` carries a gradient whatever else the image holds: every
    # u_j inside (0.3, 0.7), a non-zero mask, x away from gt, a non-zero depth mask and q != 0.  The others (images of at
    # least ROLES pixels): mask 0, mask 0.5, q == 0 exactly, depth mask 0.5, every channel below 0, every channel above 1.
    perm = torch.randperm(H * W, generator=g)
    at = lambda p: (int(perm[p]) // W, int(perm[p]) % W)
    live = at(0)
    roles = [at(p) for p in range(1, ROLES)] if H * W >= ROLES else None
    out = dict(rendered=r, gt=gt)
    E = None
    if exposure:
        E = torch.eye(3, 4, dtype=torch.float64) + 0.06 * torch.randn(3, 4, generator=g, dtype=torch.float64)
        if kind == 0:
            E[:, :3] *= 2.0                                   # a gain of about 2
        elif kind == 1:
            E[:, 3] -= 0.3                                    # an offset of about -0.3
        out["exposure"] = E
    if roles:
        r[(slice(None),) + roles[4]] = -0.5
        r[(slice(None),) + roles[5]] = 1.8
    u_live = 0.3 + 0.4 * torch.rand(C_, generator=g, dtype=torch.float64)
    r[(slice(None),) + live] = u_live if E is None else torch.linalg.solve(E[:, :3].T, u_live - E[:, 3])
    m_live = 1.0
    if mask:
        m = _three_levels((1, H, W), g, 0.15, 0.2)
        if roles:
            m[(0,) + roles[0]] = 0.0
            m[(0,) + roles[1]] = 0.5
        if m[(0,) + live] == 0:
            m[(0,) + live] = 1.0
        m_live = float(m[(0,) + live])
        out["alpha_mask"] = m
    x_live = u_live * m_live
    gt[(slice(None),) + live] = torch.where(x_live < 0.4, x_live + 0.2, x_live - 0.2)
    if depth:
        d = 0.2 + 0.3 * torch.rand(1, H, W, generator=g, dtype=torch.float64)
        mono = d + 0.05 * torch.randn(1, H, W, generator=g, dtype=torch.float64)
        md = _three_levels((1, H, W), g, 0.15, 0.2)
        if roles:
            mono[(0,) + roles[2]] = d[(0,) + roles[2]]
            md[(0,) + roles[3]] = 0.5
        if md[(0,) + live] == 0:
            md[(0,) + live] = 1.0
        mono[(0,) + live] = d[(0,) + live] + 0.05
        out.update(invdepth=d, mono_invdepth=mono, depth_mask=md)
    return out


def small(shape, seed=1, content="random", exposure=None, mask=True, depth=True, clamp=True):
    """Like `make`, for any size down to 1x1: `rendered` leaves [0, 1] on both sides, the alpha and depth masks take
    values in {0, 0.5, 1}, the exposure (C = 3 unless switched off) is per image -- the noise of `make`, with a gain of
    about 2 on every third image and an offset of about -0.3 on the next (a single image takes its kind from the seed)
    -- and single pixels are forced so that no gradient vanishes (see _small_one).  Repaired."""
    C_ = shape[-3]
    exposure = (C_ == 3) if exposure is None else exposure
    one = lambda n, kind: _small_one(*shape[-3:], seed + 10 * n, content, kind, exposure, mask, depth)
    if len(shape) == 3:
        inp = one(0, seed % 3)
    else:
        per = [one(n, n % 3) for n in range(shape[0])]
        inp = {k: torch.stack([p[k] for p in per]) for k in per[0]}
    inp = {k: v.float() for k, v in inp.items()}
    inp["clamp"] = clamp
    return repair(inp)


def impulses():
    """test_ssim_gpu's 3x60x130 impulse image as a batch of two whose second image and second gt are all zero: each
    `rendered` impulse in one channel only (the first is exactly 1.0: the upper end of the inclusive gate), gt's in all
    three, under a mixing exposure without offsets, so that u = 0 wherever rendered = 0.  -> inputs, every impulse's
    (y, x)."""
    import test_ssim_gpu as ts
    r = torch.zeros(2, ts.IMP_C, ts.IMP_H, ts.IMP_W)
    gt = torch.zeros_like(r)
    for i, (y, x) in enumerate(ts.IMPULSES_1):
        r[0, i % 3, y, x] = 1.0 if i == 0 else 0.2 + 0.045 * i
    for i, (y, x) in enumerate(ts.IMPULSES_2):
        gt[0, :, y, x] = torch.tensor([0.9 - 0.07 * i, 0.3 + 0.05 * i, 0.6])
    E = torch.eye(3, 4) + 0.05 * torch.tensor([[0., 1, -1, 0], [1, 0, 1, 0], [-1, 1, 0, 0]])
    inp = dict(rendered=r, gt=gt, exposure=E.expand(2, 3, 4).contiguous(), clamp=True)
    return inp, ts.IMPULSES_1 + ts.IMPULSES_2


def l1_closed_form(inp, grad_out=1.0, dtype=torch.float32):
    """lambda_dssim = 0 without an exposure: grad_rendered = ((1 - 0) g / count) sign(x - gt) m [0 <= r <= 1] with
    x = clamp(r) m, every operation in `dtype`; g arrives in `dtype` and the constant is formed in double and rounded to
    it, as the kernel does."""
    r, gt = inp["rendered"].to(dtype), inp["gt"].to(dtype)
    m = inp["alpha_mask"].to(dtype).reshape(r.shape[:-3] + (1,) + r.shape[-2:])
    c = torch.tensor((1.0 - 0.0) / r.numel() * float(torch.tensor(grad_out, dtype=dtype)), dtype=torch.float64).to(dtype)
    x = (r.clamp(0, 1) if inp["clamp"] else r) * m
    gate = ((r >= 0) & (r <= 1)).to(dtype) if inp["clamp"] else torch.ones_like(r)
    return c * torch.sign(x - gt) * m * gate


def depth_closed_form(inp, depth_weight, grad_out=1.0, dtype=torch.float32):
    """grad_invdepth = (depth_weight / (N H W) * g) sign((d - mono) md) md, every operation in `dtype` and the constant
    formed in double in the kernel's order, then rounded to it."""
    d, mono, md = (inp[k].to(dtype) for k in ("invdepth", "mono_invdepth", "depth_mask"))
    c = torch.tensor(float(depth_weight) / d.numel() * float(torch.tensor(grad_out, dtype=dtype)), dtype=torch.float64).to(dtype)
    return c * torch.sign((d - mono) * md) * md
