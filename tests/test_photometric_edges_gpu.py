"""The fused training loss (hgs.loss.photometric_loss, csrc/photometric.hip) where a tiled kernel goes wrong: one pixel
either side of the 32x16 tile grid, single rows and columns, images smaller than the 11-tap window, footprints across
tile seams and image borders, batches and their reductions, upstream gradients, closed forms, degenerate content, every
subset of requires_grad and every layout the wrapper accepts.

The parity rule is tests/photometric_cases.assert_parity everywhere (the kernels against the float64 spec, measured by
the float32 CPU evaluation of the reference's torch lines); no pixel is left out: every test that applies it first
asserts that the knife-edge bands are empty.  Everything else is exact: zeros that the definition forces, and pairs of
calls whose per-pixel arithmetic is the same and therefore give the same bits.  tests/test_photometric_cpu.py checks the
inputs' own conditions (non-zero gradients, one pixel of every kind, the sweep's coverage) without a GPU."""
import itertools

import pytest
import torch

import photometric_cases as pc
import photometric_spec as spec
import ssim_spec
import test_ssim_gpu as ts

pytestmark = pytest.mark.gpu

LAM, DW = 0.2, 0.7
GRADS = ("grad_rendered", "grad_exposure", "grad_invdepth")
VALUES = ("loss", "l1", "ssim", "depth")


def check_case(inp, dev, what, lam=LAM, dw=DW, weight=None):
    assert pc.band_counts(inp) == (0, 0, 0), "a pixel sits in a knife-edge band"
    want = spec.loss_and_grads(lambda_dssim=lam, depth_weight=dw, grad_out=1.0 if weight is None else weight, **inp)
    yard = pc.formula(inp, lam, dw, torch.float32, weight=weight)
    got = pc.fused(inp, lam, dw, dev, weight=weight)
    pc.assert_parity(got, yard, want, what)
    return got, want


def same_bits(a, b, keys):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), \
                f"{k}: {int((a[k] != b[k]).sum())} elements differ, by up to {(a[k] - b[k]).abs().max().item():.3e}"


def image(inp, n):
    return {k: (v[n].clone() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}


# -- 2. one pixel either side of the tile grid, single rows and columns, images smaller than the window ------------------

@pytest.mark.parametrize("H,W,C_,N,content", pc.SWEEP)
def test_off_grid_and_tiny_images(gpu, H, W, C_, N, content):
    check_case(pc.sweep_case(H, W, C_, N, content), gpu, f"{content} {N}x{C_}x{H}x{W}")


# -- 3. the 11x11 footprint, and the backward's 21x21, across tile seams and image borders -------------------------------

def test_impulses_on_seams_and_borders(gpu):
    """Single pixels on a zero background (pc.impulses) at x mod 32 in {0, 4, 5, 26, 27, 31} and y mod 16 in
    {0, 4, 5, 10, 11, 15}, on the four borders and in the corners: the rule."""
    check_case(pc.impulses()[0], gpu, "impulses", dw=0.0)


def test_impulses_leave_exact_zeros_and_reach_every_channel(gpu):
    """No tolerance here.  grad_rendered is exactly 0.0 more than 10 pixels from every impulse -- u = 0 passes the
    inclusive gate, x = gt = 0, every window sees zeros, A = 0 and sign(0) = 0 -- and non-zero wherever the spec's
    exceeds 1e-6 of its largest value (u = 0 and the impulse of exactly 1.0 pass the gate); the all-zero second image
    gets exact zeros, the exposure's gradient too; an impulse in one channel of `rendered` reaches every channel of the
    gradient through the exposure."""
    inp, points = pc.impulses()
    got = pc.fused(inp, LAM, 0.0, gpu)
    gs = spec.loss_and_grads(lambda_dssim=LAM, **inp)["grad_rendered"]
    far = ts._far_from(points, ts.IMP_H, ts.IMP_W, 10)
    assert int(far.sum()) == 3919
    g = got["grad_rendered"]
    assert bool((g[0][:, far] == 0).all()), f"{int((g[0][:, far] != 0).sum())} non-zero gradients far from every impulse"
    big = gs.abs() > 1e-6 * gs.abs().max()
    assert int(big.sum()) > 3000
    assert bool((g[big] != 0).all()), f"{int((g[big] == 0).sum())} zero gradients where the spec's is not small"
    assert bool((g[1] == 0).all()) and bool((got["grad_exposure"][1] == 0).all())
    assert int((got["grad_exposure"][0] != 0).sum()) >= 10
    for i, (y, x) in enumerate(ts.IMPULSES_1):
        near = g[0][:, max(0, y - 5): y + 6, max(0, x - 5): x + 6]
        assert bool((near != 0).flatten(1).any(dim=1).all()), f"impulse {i} at {(y, x)} misses a channel"


def test_the_border_is_zero_padded_like_ssim_hip(gpu):
    """lambda_dssim = 1 without exposure, mask or clamp is -SSIM alone: the gradient has the bits of hgs.loss.ssim's.
    Both kernels evaluate gs * (F[A] + 2 x F[B] + gt F[Cc]) with gs = float32(-1 / count) from maps of the same
    expressions, and the L1 part adds 0.0 * sign.  The image is off the tile grid and has content on all four borders,
    so a halo or a padding that differed from ssim.hip's would show."""
    from hgs import loss
    inp = pc.small((2, 3, 37, 53), seed=31, exposure=False, mask=False, depth=False, clamp=False)
    got = pc.fused(inp, 1.0, 0.0, gpu)
    a = inp["rendered"].to(gpu).requires_grad_(True)
    s = loss.ssim(a, inp["gt"].to(gpu))
    (1.0 - s).backward()
    r = inp["rendered"]
    assert bool((r[:, :, (0, -1)] != 0).all()) and bool((r[:, :, :, (0, -1)] != 0).all())
    same_bits(got, dict(grad_rendered=a.grad.cpu()), ["grad_rendered"])
    assert abs(got["ssim"].item() - s.item()) <= 2e-6 and got["l1"].item() > 0


# -- 4. a batch against its images alone ----------------------------------------------------------------------------------

def test_a_batch_gives_each_images_own_bits(gpu):
    """N = 4, every optional input: image n's gradients in the batched call equal those of a call on image n alone,
    backpropagated through 0.25 * loss, bit for bit.  Both scales are a double divided by a count and multiplied by a
    power of two, and neither the per-tile partials nor the per-image reduction order depend on N.  A halo, a mask
    plane, an exposure or a partial taken from the neighbouring image fails this.  The four values are the means of the
    images' own, to 2e-6 (the rule's floor for values)."""
    N = 4
    inp = pc.small((N, 3, 37, 53), seed=41)
    got = pc.fused(inp, LAM, DW, gpu)
    singles = [pc.fused(image(inp, n), LAM, DW, gpu, weight=0.25) for n in range(N)]
    for n, one in enumerate(singles):
        same_bits({k: got[k][n] for k in GRADS}, one, GRADS)
        assert all(one[k].norm().item() > 0 for k in GRADS), n
    for k in VALUES:
        mean = sum(one[k].double().item() for one in singles) / N
        assert abs(got[k].item() - mean) <= 2e-6, (k, got[k].item(), mean)
    assert len({one["loss"].item() for one in singles}) == N, "every image has its own loss"


def test_a_batch_of_four_is_within_the_rule(gpu):
    check_case(pc.small((4, 3, 37, 53), seed=41), gpu, "batch of 4")


# -- 5. many images, more tiles than the reductions have threads, one tile ---------------------------------------------

@pytest.mark.parametrize("shape", [(64, 3, 37, 53), (3, 3, 540, 960), (1, 3, 16, 32)])
def test_batches_and_the_reductions(gpu, shape):
    """(3,3,540,960) has 1 020 tiles per image, more than the exposure reduction's 256 threads, and 3 060 workgroups,
    more than the value reduction's 1 024.  Noise on gt grows with n: every image has its own values."""
    N = shape[0]
    inp = pc.make(shape, seed=N)
    g = torch.Generator().manual_seed(N)
    noise = torch.randn(shape, generator=g) * (0.005 * 1.07 ** torch.arange(N, dtype=torch.float32)).reshape(N, 1, 1, 1)
    inp["gt"] = (inp["gt"] + noise).clamp(0, 1)
    check_case(pc.repair(inp), gpu, f"batch {shape}")


# -- 6. upstream gradients ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [0.0, -1.75, 1e-3, 40.0])
def test_upstream_gradient(gpu, w):
    got, _ = check_case(pc.small((2, 3, 37, 53), seed=61), gpu, f"{w} * loss", weight=w)
    if w == 0.0:
        assert all(bool((got[k] == 0).all()) for k in GRADS)


# -- 7. closed forms, to the bit, against float32 torch on the CPU -----------------------------------------------------

def _lambda_zero_case():
    """No exposure; exact zeros and exact ones under a non-zero mask, with x != gt: both ends of the gate carry gradient."""
    inp = pc.make((3, 37, 53), seed=11, exposure=False)
    inp["rendered"][:, 20:24, 5:30] = 1.0
    inp = pc.repair(inp)
    live = (inp["alpha_mask"] > 0).expand(3, -1, -1)
    for end in (0.0, 1.0):
        assert int(((inp["rendered"] == end) & live & (inp["gt"] != end * inp["alpha_mask"])).sum()) >= 50
    return inp, live


def test_l1_gradient_alone_at_lambda_zero(gpu):
    """lambda_dssim = 0, no exposure: the SSIM factor is float32(-0.0) times a finite bracket, so grad_rendered is
    float32(1 / count) * sign(x - gt) * m * [0 <= r <= 1] exactly, x = clamp(r) * m in float32."""
    inp, live = _lambda_zero_case()
    want = pc.l1_closed_form(inp)
    assert bool((want[(inp["rendered"] == 1) & live] != 0).any()) and bool((want[(inp["rendered"] == 0) & live] != 0).any())
    same_bits(pc.fused(inp, 0.0, DW, gpu), dict(grad_rendered=want), ["grad_rendered"])


def test_lambda_zero_is_within_the_rule(gpu):
    check_case(_lambda_zero_case()[0], gpu, "lambda 0", lam=0.0)


@pytest.mark.parametrize("lam,w", [(0.2, 1.0), (0.0, -1.75), (1.0, 40.0)])
def test_depth_gradient_is_a_sign_times_one_constant(gpu, lam, w):
    """grad_invdepth = float32(depth_weight / (N H W) * g) * sign((d - mono) * md) * md in float32 whatever lambda is,
    with depth-mask values of -0.75, 0, 0.3, 0.5 and 1; the depth value is within the rule."""
    inp = pc.small((2, 3, 33, 65), seed=71)
    g = torch.Generator().manual_seed(3)
    levels = torch.tensor([-0.75, 0.0, 0.3, 0.5, 1.0])
    inp["depth_mask"] = levels[torch.randint(0, 5, inp["depth_mask"].shape, generator=g)]
    inp = pc.repair(inp)
    got, _ = check_case(inp, gpu, f"depth, lambda {lam}", lam=lam, weight=w)
    want = pc.depth_closed_form(inp, DW, w)
    assert bool((want[inp["depth_mask"] < 0] != 0).any()) and bool((want == 0).any())
    same_bits(got, dict(grad_invdepth=want), ["grad_invdepth"])


def test_dssim_alone_and_a_zero_depth_weight(gpu):
    inp = pc.small((2, 3, 37, 53), seed=72)
    got, want = check_case(inp, gpu, "lambda 1, depth_weight 0", lam=1.0, dw=0.0)
    assert want["depth"].item() > 1e-3 and got["depth"].item() > 1e-3, "depth is reported whatever its weight"
    assert bool((got["grad_invdepth"] == 0).all())


# -- 8. exposures that change no bit -----------------------------------------------------------------------------------

def test_identity_exposure_changes_no_bit(gpu):
    """fmaf with 0 and 1 is exact and one `channel` body serves both template instantiations: under eye(3, 4) the four
    values and grad_rendered are those of the call without an exposure; grad_exposure is within the rule."""
    inp = pc.small((2, 3, 37, 53), seed=81)
    inp["exposure"] = torch.eye(3, 4).expand(2, 3, 4).contiguous()
    inp = pc.repair(inp)
    got, _ = check_case(inp, gpu, "identity exposure")
    plain = pc.fused({k: v for k, v in inp.items() if k != "exposure"}, LAM, DW, gpu)
    same_bits(got, plain, VALUES + ("grad_rendered", "grad_invdepth"))
    assert got["grad_exposure"].norm().item() > 0


@pytest.mark.parametrize("sigma", [(1, 2, 0), (2, 1, 0), (0, 2, 1)])
def test_permutation_exposure_changes_no_bit(gpu, sigma):
    """E[i, sigma(i)] = 1 sends r_i to u_sigma(i): the four values are those of the call without an exposure on the
    permuted image, and grad_rendered is that call's gradient, un-permuted."""
    inp = pc.small((3, 37, 53), seed=82, exposure=False)
    E = torch.zeros(3, 4)
    E[torch.arange(3), torch.tensor(sigma)] = 1.0
    inv = torch.argsort(torch.tensor(sigma))
    permuted = dict(inp, rendered=inp["rendered"][inv].contiguous())          # u_j = r_{sigma^-1(j)}
    assert pc.band_counts(permuted) == (0, 0, 0)
    plain = pc.fused(permuted, LAM, DW, gpu)
    with_E = dict(inp, exposure=E)
    got, _ = check_case(with_E, gpu, f"permutation {sigma}")
    same_bits(got, plain, VALUES + ("grad_invdepth",))
    same_bits(got, dict(grad_rendered=plain["grad_rendered"][list(sigma)]), ["grad_rendered"])
    assert got["grad_rendered"].norm().item() > 0


# -- 9. degenerate content ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [2.0, -1.0])
def test_everything_clamped(gpu, r):
    inp = pc.small((2, 3, 37, 53), seed=91)
    inp["rendered"] = torch.full_like(inp["rendered"], r)
    inp = pc.repair(inp)
    u, _ = spec.transform(inp["rendered"].double(), inp["exposure"].double(), True, None)
    assert bool(((u < 0) | (u > 1)).all())
    got, _ = check_case(inp, gpu, f"r = {r}")
    assert bool((got["grad_rendered"] == 0).all()) and bool((got["grad_exposure"] == 0).all())
    assert got["grad_invdepth"].norm().item() > 0


def test_everything_masked(gpu):
    """alpha_mask = 0: x = 0, no gradient reaches rendered or the exposure, and the loss is
    (1 - lambda) mean|gt| + lambda (1 - SSIM(0, gt))."""
    inp = pc.small((2, 3, 37, 53), seed=92)
    inp["alpha_mask"] = torch.zeros_like(inp["alpha_mask"])
    inp = pc.repair(inp)
    got, want = check_case(inp, gpu, "mask 0", dw=0.0)
    gt = inp["gt"].double()
    closed = (1 - LAM) * gt.abs().mean() + LAM * (1 - ssim_spec.ssim(torch.zeros_like(gt), gt))
    assert abs(want["loss"].item() - closed.item()) <= 1e-12
    assert bool((got["grad_rendered"] == 0).all()) and bool((got["grad_exposure"] == 0).all())


def test_a_zero_depth_mask(gpu):
    inp = pc.small((2, 3, 37, 53), seed=93)
    inp["depth_mask"] = torch.zeros_like(inp["depth_mask"])
    got, _ = check_case(inp, gpu, "depth mask 0")
    assert got["depth"].item() == 0.0 and bool((got["grad_invdepth"] == 0).all())


@pytest.mark.parametrize("kind", ["natural", "constant", "binary", "above_one"])
def test_rendered_equal_to_gt(gpu, kind):
    """No exposure, no mask, clamp off: l1 == 0.0, S within 2e-6 of 1, and the gradient is the float32 rounding of terms
    that cancel: |grad_rendered| <= lambda * 64 eps32 * T / count with T = test_ssim_gpu._cancellation_scale (derived in
    its test_identical_images); the L1 part adds (1 - lambda) / count * sign(0) = 0 exactly."""
    g = torch.Generator().manual_seed(7)
    shape = (2, 3, 45, 67)
    x = {"natural": lambda: torch.stack([pc.natural(3, 45, 67, s) for s in (1, 2)]).float(),
         "constant": lambda: torch.full(shape, 0.37),
         "binary": lambda: (torch.rand(shape, generator=g) > 0.5).float(),
         "above_one": lambda: 3 * torch.rand(shape, generator=g)}[kind]()
    inp = dict(rendered=x, gt=x.clone(), clamp=False)
    assert pc.band_counts(inp) == (0, 0, 0)
    got = pc.fused(inp, LAM, 0.0, gpu)
    assert got["l1"].item() == 0.0
    assert abs(got["ssim"].double().item() - 1) <= 2e-6
    bound = LAM * 64 * ts.EPS32 * ts._cancellation_scale(x, x) / x.numel()
    ratio = (got["grad_rendered"].double().abs() / bound).max().item()
    print(f"{kind}: |grad| / bound up to {ratio:.3g}")
    assert ratio <= 1


@pytest.mark.parametrize("exposure", [False, True])
def test_all_zero_images(gpu, exposure):
    """rendered = gt = 0 and d = mono: A = 0, x = gt = 0 multiply F[B] and F[Cc], sign(0) = 0 three times over.  With an
    exposure without offsets u is still 0 and passes the gate."""
    z = torch.zeros(2, 3, 21, 40)
    d = torch.full((2, 1, 21, 40), 0.3)
    inp = dict(rendered=z, gt=z.clone(), alpha_mask=torch.ones(2, 1, 21, 40), invdepth=d, mono_invdepth=d.clone(),
               depth_mask=torch.ones(2, 1, 21, 40), clamp=True)
    if exposure:
        inp["exposure"] = pc.impulses()[0]["exposure"]
    got = pc.fused(inp, LAM, DW, gpu)
    assert got["l1"].item() == 0.0 and got["depth"].item() == 0.0 and abs(got["ssim"].double().item() - 1) <= 2e-6
    for k in GRADS:
        assert got[k] is None or bool((got[k] == 0).all()), k
    assert (got["grad_exposure"] is not None) == exposure


def test_clamp_off_far_outside_the_unit_interval(gpu):
    inp = pc.small((2, 3, 37, 53), seed=94, clamp=False)
    g = torch.Generator().manual_seed(94)
    inp["rendered"] = 7.0 * torch.rand(inp["rendered"].shape, generator=g) - 3.0
    inp = pc.repair(inp)
    assert inp["rendered"].min().item() < -2.9 and inp["rendered"].max().item() > 3.9
    check_case(inp, gpu, "clamp off, r in [-3, 4]")


@pytest.mark.parametrize("kind", ["two_constants", "checkerboard_vs_inverse", "salt_and_pepper"])
def test_flat_binary_and_impulse_noise_content(gpu, kind):
    """test_ssim_gpu's degenerate pairs as rendered and gt, with the mask and the depth inputs of a small case and the
    clamp on: the checkerboard and the salt-and-pepper image sit on u == 0 and u == 1 exactly."""
    r, gt = ts.DEGENERATE[kind]((3, 45, 67))
    inp = dict(pc.small((3, 45, 67), seed=95, exposure=False), rendered=r.contiguous(), gt=gt.contiguous())
    check_case(pc.repair(inp), gpu, kind)


# -- 10. every subset of requires_grad ---------------------------------------------------------------------------------

SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(("rendered", "exposure", "invdepth"), n)]


@pytest.mark.parametrize("subset", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_every_subset_of_requires_grad(gpu, subset):
    """grad_exposure == NULL and grad_invdepth == NULL switch code paths of the backward: the gradients that are asked
    for have the bits of the full set's, the others are None."""
    inp = pc.small((2, 3, 37, 53), seed=101)
    full = pc.fused(inp, LAM, DW, gpu)
    got = pc.fused(inp, LAM, DW, gpu, grads=subset)
    same_bits(got, full, VALUES + tuple("grad_" + k for k in subset))
    for k in ("rendered", "exposure", "invdepth"):
        assert (got["grad_" + k] is not None) == (k in subset), k


# -- 11. layouts -------------------------------------------------------------------------------------------------------

def _call(dev, inp, leaves=("rendered", "exposure", "invdepth")):
    """photometric_loss on tensors that are already on the device, as they are -> values and the leaves' own .grad."""
    from hgs.loss import photometric_loss
    t = dict(inp)
    res = photometric_loss(t.pop("rendered"), t.pop("gt"), lambda_dssim=LAM, depth_weight=DW, **t)
    res.loss.backward()
    out = {k: getattr(res, k).detach().cpu() for k in VALUES}
    for k in leaves:
        assert inp[k].grad.shape == inp[k].shape, k
        out["grad_" + k] = inp[k].grad.cpu()
    return out


def test_layouts_give_the_contiguous_calls_bits(gpu):
    """A channels-last `rendered`, an `alpha_mask` made by expand (stride 0), planes given as (N,1,H,W) and as (N,H,W),
    and a non-contiguous `invdepth` that requires grad: the same bits, gradients in the caller's shapes."""
    N, H, W = 2, 37, 53
    inp = pc.small((N, 3, H, W), seed=111)
    column = inp["alpha_mask"][:, :, :, :1].clone()                         # (N,1,H,1): one value per row
    column[:, :, ::3] = 1.0
    inp["alpha_mask"] = column.expand(N, 1, H, W).contiguous()
    inp = pc.repair(inp)
    ref = pc.fused(inp, LAM, DW, gpu)
    keys = VALUES + GRADS

    def leaves(t):
        for k in ("rendered", "exposure", "invdepth"):
            t[k] = t[k].detach().requires_grad_(True)
        return t

    on = lambda: {k: (v.to(gpu) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    t = on()
    t["rendered"] = t["rendered"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not t["rendered"].is_contiguous()
    same_bits(_call(gpu, leaves(t)), ref, keys)

    t = on()
    t["alpha_mask"] = column.to(gpu).expand(N, 1, H, W)
    assert t["alpha_mask"].stride(3) == 0
    same_bits(_call(gpu, leaves(t)), ref, keys)

    t = on()
    for k in ("alpha_mask", "invdepth", "mono_invdepth", "depth_mask"):
        t[k] = t[k].reshape(N, H, W)
    got = _call(gpu, leaves(t))
    assert got["grad_invdepth"].shape == (N, H, W)
    same_bits(dict(got, grad_invdepth=got["grad_invdepth"].reshape(N, 1, H, W)), ref, keys)

    t = on()
    wide = torch.zeros(N, 1, H, 2 * W, device=gpu)
    wide[..., ::2] = t["invdepth"]
    t["invdepth"] = wide[..., ::2]
    assert not t["invdepth"].is_contiguous()
    same_bits(_call(gpu, leaves(t)), ref, keys)
