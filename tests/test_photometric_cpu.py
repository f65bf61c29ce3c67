"""The fused training loss without a GPU: the float64 spec (tests/photometric_spec.py) against torch autograd of the
reference's lines and against the fixture recorded from the reference's own code, the C ABI's size checks and workspace
query, hgs.loss.photometric_loss's argument checks, and the kernels' resources."""
import ctypes as C
import math
import os
import shutil
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import photometric_cases as pc
import photometric_spec as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_photometric_golden.npz")

# shape, exposure, mask, depth, clamp: off-grid (not multiples of 32x16) and sub-window (< 11) sizes, a batch, each
# optional input on and off
CASES = [((3, 23, 31), True, True, True, True), ((3, 40, 52), True, False, True, True),
         ((3, 37, 53), False, True, True, True), ((3, 16, 16), True, True, False, True),
         ((3, 21, 19), True, True, True, False), ((3, 7, 30), False, False, False, True),
         ((1, 30, 5), False, True, True, True), ((3, 8, 9), True, True, True, True),
         ((4, 1, 1), False, False, True, False), ((2, 3, 33, 65), True, True, True, True),
         ((2, 4, 12, 20), False, True, False, True)]


def _close(a, b, rel=1e-12):
    a, b = a.double(), b.double()
    return (a - b).abs().max().item() <= rel * max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("shape,exposure,mask,depth,clamp", CASES)
def test_spec_matches_autograd_of_the_reference_lines(shape, exposure, mask, depth, clamp):
    inp = pc.make(shape, seed=3, exposure=exposure, mask=mask, depth=depth, clamp=clamp)
    assert pc.band_counts(inp) == (0, 0, 0)
    inp = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    lam, dw = 0.2, 0.7
    want = pc.formula(inp, lam, dw, torch.float64)
    got = spec.loss_and_grads(lambda_dssim=lam, depth_weight=dw, **inp)
    for k in ("loss", "l1", "ssim", "depth"):
        assert abs(got[k].item() - want[k].item()) <= 1e-12 * max(abs(want[k].item()), 1e-300), k
    for k in ("grad_rendered", "grad_exposure", "grad_invdepth"):
        if want[k] is None:
            assert got[k] is None
        else:
            assert got[k].shape == want[k].shape and _close(got[k], want[k]), k


def test_spec_upstream_gradient_and_lambda_ends():
    inp = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in pc.make((3, 20, 24), seed=5).items()}
    for lam in (0.0, 1.0):
        want = pc.formula(inp, lam, 0.3, torch.float64)
        got = spec.loss_and_grads(lambda_dssim=lam, depth_weight=0.3, **inp)
        assert _close(got["grad_rendered"], want["grad_rendered"]) and _close(got["grad_exposure"], want["grad_exposure"])
    a = spec.loss_and_grads(lambda_dssim=0.2, depth_weight=0.3, grad_out=-2.5, **inp)
    b = spec.loss_and_grads(lambda_dssim=0.2, depth_weight=0.3, **inp)
    for k in ("grad_rendered", "grad_exposure", "grad_invdepth"):
        assert _close(a[k], -2.5 * b[k])


def test_exact_cases_stay_in_the_inputs():
    """A zero background under an identity exposure sits exactly on the clamp's lower end and still passes the gradient;
    masked black pixels have x == gt == 0 and d == d_mono rows have q == 0: sign(0) = 0 there."""
    inp = pc.make((3, 40, 56), seed=7, identity=True)
    r, E = inp["rendered"].double(), inp["exposure"].double()[None]
    u, x = spec.transform(r[None], E, True, inp["alpha_mask"].double()[None])
    assert int((u == 0).sum()) >= 100 and int(((x == 0) & (inp["gt"].double()[None] == 0)).sum()) >= 100
    assert int((inp["invdepth"] == inp["mono_invdepth"]).sum()) >= 100
    got = spec.loss_and_grads(lambda_dssim=0.2, depth_weight=0.5, **inp)
    edge = (u[0] == 0) & (inp["alpha_mask"].double() > 0)
    assert bool((got["grad_rendered"][edge] != 0).any()), "the gate includes u == 0"
    assert bool((got["grad_invdepth"][inp["invdepth"] == inp["mono_invdepth"]] == 0).all())


# -- the fixture: numbers recorded from the reference's own code (tests/golden/make_photometric_golden.py) -------------

def golden_cases():
    z = np.load(GOLDEN)
    for name in z["case_names"]:
        name = str(name)
        get = lambda k: torch.from_numpy(z[f"{name}.{k}"]) if f"{name}.{k}" in z.files else None
        inp = {k: get("in." + k) for k in ("rendered", "gt") + pc.OPTIONAL if get("in." + k) is not None}
        lam, dw, clamp, exposure_grad = z[f"{name}.scalars"]
        inp["clamp"] = bool(clamp)
        want = {k: get("out." + k) for k in ("loss", "l1", "ssim", "depth", "grad_rendered", "grad_exposure",
                                             "grad_invdepth")}
        yield name, inp, float(lam), float(dw), bool(exposure_grad), want


def _reference_window_filt(t):
    """The reference's window as data (utils/loss_utils.py:23-31): eleven float32 taps, their float32 outer product,
    cast to the image's dtype, one 2-D convolution with zero padding.  Symmetric, so still its own adjoint."""
    g = torch.tensor([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)])
    g = g / g.sum()
    w2 = g[:, None].mm(g[None, :]).to(t.dtype)
    return F.conv2d(t.reshape(-1, 1, *t.shape[-2:]), w2[None, None], padding=5).reshape(t.shape)


def test_spec_reproduces_the_reference_fixture(monkeypatch):
    """With the reference's float32-built window in place of the exact one, the spec agrees with the reference's own
    float64 run to rounding (1e-11 of each result's largest value).  With the exact window the difference is the
    window's: its taps are off by up to 3 * 2^-24 relative, printed below, not asserted."""
    names = []
    for exact in (True, False):
        if not exact:
            monkeypatch.setattr(spec.ssim_spec, "filt", _reference_window_filt)
        for name, inp, lam, dw, exposure_grad, want in golden_cases():
            assert pc.band_counts(inp) == (0, 0, 0), name
            got = spec.loss_and_grads(lambda_dssim=lam, depth_weight=dw, **inp)
            if exact:
                rel = lambda k: ((got[k] - want[k]).abs().max() / want[k].abs().max()).item()
                print(f"{name}, exact window: loss off by {abs(got['loss'].item() - want['loss'].item()):.2e}, "
                      f"grad_rendered by {rel('grad_rendered'):.2e} of its maximum")
                continue
            names.append(name)
            for k in ("loss", "l1", "ssim", "depth"):
                assert abs(got[k].item() - want[k].item()) <= 1e-11 * max(abs(want[k].item()), 1e-300), (name, k)
            assert _close(got["grad_rendered"], want["grad_rendered"], 1e-11), name
            if exposure_grad:
                assert _close(got["grad_exposure"], want["grad_exposure"], 1e-11), name
            else:
                assert want["grad_exposure"] is None
            if want["grad_invdepth"] is not None:
                assert _close(got["grad_invdepth"], want["grad_invdepth"], 1e-11), name
    assert names == ["exposure_mask_depth", "identity_zero_background", "train_post", "train_coarse"]


# -- C ABI: no GPU needed -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from hgs import _lib
    return _lib.lib()


def _args(**kw):
    from hgs import _lib
    base = dict(rendered=256, gt=256, exposure=None, alpha_mask=None, invdepth=None, mono_invdepth=None,
                depth_mask=None, N=1, C=3, H=8, W=8, clamp=1, reserved=0, lambda_dssim=0.2, depth_weight=0.0)
    base.update(kw)
    return _lib.PhotoArgs(**base)


def test_struct_layout_matches_the_header():
    from hgs import _lib
    assert C.sizeof(_lib.PhotoArgs) == 7 * 8 + 6 * 4 + 2 * 8
    assert _lib.PhotoArgs.N.offset == 56 and _lib.PhotoArgs.lambda_dssim.offset == 80


def test_tmp_bytes_query_needs_no_gpu(lib):
    # twelve doubles (the exposure partials; the forward uses three) per 32x16 tile of every image, 256-byte aligned
    n = lib.hgs_photo_tmp_bytes(1, 3, 1080, 1920)
    assert n >= 60 * 68 * 12 * 8 and n % 256 == 0 and n <= 512 * 1024
    assert lib.hgs_photo_tmp_bytes(8, 3, 1080, 1920) >= 8 * 60 * 68 * 12 * 8
    assert lib.hgs_photo_tmp_bytes(1, 1, 1, 1) >= 96


@pytest.mark.parametrize("dims", [(0, 3, 10, 10), (1, 0, 10, 10), (1, 3, 0, 10), (1, 3, 10, -1), (-2, 3, 10, 10),
                                  (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (1, 1, 65536, 131072)])
def test_bad_sizes_are_refused_before_any_hip_call(lib, dims):
    assert lib.hgs_photo_tmp_bytes(*dims) == 0
    assert b"bad sizes" in lib.hgs_last_error()
    p = C.c_void_p(256)      # never dereferenced: the checks come first
    N, C_, H, W = dims
    a = _args(N=N, C=C_, H=H, W=W)
    assert lib.hgs_photo_fwd(C.byref(a), p, None, p, None, 0) != 0
    assert b"bad sizes" in lib.hgs_last_error()
    assert lib.hgs_photo_bwd(C.byref(a), p, p, p, None, None, p, None, 0) != 0
    assert b"bad sizes" in lib.hgs_last_error()


def test_bad_argument_combinations_are_refused_before_any_hip_call(lib):
    p = C.c_void_p(256)
    fwd = lambda a: lib.hgs_photo_fwd(C.byref(a), p, None, p, None, 0)
    bwd = lambda a, gE=None, gd=None: lib.hgs_photo_bwd(C.byref(a), p, p, p, gE, gd, p, None, 0)
    for a, msg in [(_args(exposure=256, C=4), b"needs C = 3"), (_args(invdepth=256), b"depth triple"),
                   (_args(mono_invdepth=256, depth_mask=256), b"depth triple"),
                   (_args(lambda_dssim=1.5), b"lambda_dssim"), (_args(lambda_dssim=float("nan")), b"lambda_dssim"),
                   (_args(lambda_dssim=-0.1), b"lambda_dssim"), (_args(depth_weight=float("inf")), b"depth_weight"),
                   (_args(rendered=None), b"null argument"), (_args(gt=None), b"null argument")]:
        assert fwd(a) != 0 and msg in lib.hgs_last_error(), msg
        assert bwd(a) != 0 and msg in lib.hgs_last_error(), msg
    assert lib.hgs_photo_fwd(None, p, None, p, None, 0) != 0 and b"null argument" in lib.hgs_last_error()
    assert lib.hgs_photo_fwd(C.byref(_args()), None, None, p, None, 0) != 0 and b"null argument" in lib.hgs_last_error()
    assert lib.hgs_photo_fwd(C.byref(_args()), p, None, C.c_void_p(260), None, 0) != 0
    assert b"8-byte aligned" in lib.hgs_last_error()
    assert lib.hgs_photo_bwd(C.byref(_args()), None, p, p, None, None, p, None, 0) != 0
    assert b"null argument" in lib.hgs_last_error()
    assert bwd(_args(), gE=p) != 0 and b"grad_exposure without" in lib.hgs_last_error()
    assert bwd(_args(), gd=p) != 0 and b"grad_invdepth without" in lib.hgs_last_error()


# -- hgs.loss.photometric_loss: argument checks (they come before any device work) -------------------------------------

def test_photometric_loss_rejects_bad_arguments_and_cpu_tensors():
    from hgs.loss import photometric_loss as pl
    r, gt = torch.rand(3, 16, 16), torch.rand(3, 16, 16)
    plane = torch.rand(1, 16, 16)
    with pytest.raises(ValueError, match="shapes differ"):
        pl(r, gt[:, :8], lambda_dssim=0.2)
    with pytest.raises(ValueError, match=r"\(C,H,W\) or \(N,C,H,W\)"):
        pl(r[0], gt[0], lambda_dssim=0.2)
    for lam in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lambda_dssim"):
            pl(r, gt, lambda_dssim=lam)
    with pytest.raises(ValueError, match="depth_weight"):
        pl(r, gt, lambda_dssim=0.2, depth_weight=float("nan"))
    with pytest.raises(ValueError, match="exposure needs C = 3"):
        pl(torch.rand(4, 16, 16), torch.rand(4, 16, 16), lambda_dssim=0.2, exposure=torch.eye(3, 4))
    with pytest.raises(ValueError, match="exposure has shape"):
        pl(r, gt, lambda_dssim=0.2, exposure=torch.eye(4, 4))
    with pytest.raises(ValueError, match="exposure has shape"):
        pl(r[None], gt[None], lambda_dssim=0.2, exposure=torch.eye(3, 4))          # a batch wants (N,3,4)
    with pytest.raises(ValueError, match="incomplete depth triple"):
        pl(r, gt, lambda_dssim=0.2, invdepth=plane)
    with pytest.raises(ValueError, match="incomplete depth triple"):
        pl(r, gt, lambda_dssim=0.2, mono_invdepth=plane, depth_mask=plane)
    with pytest.raises(ValueError, match="alpha_mask has shape"):
        pl(r, gt, lambda_dssim=0.2, alpha_mask=torch.rand(3, 16, 16))
    with pytest.raises(ValueError, match="invdepth has shape"):
        pl(r, gt, lambda_dssim=0.2, invdepth=plane[:, :8], mono_invdepth=plane, depth_mask=plane)
    for name in ("gt", "alpha_mask", "mono_invdepth", "depth_mask"):
        kw = dict(alpha_mask=plane.clone(), invdepth=plane.clone(), mono_invdepth=plane.clone(), depth_mask=plane.clone())
        g = gt.clone()
        (g if name == "gt" else kw[name]).requires_grad_(True)
        with pytest.raises(ValueError, match=f"{name} requires grad"):
            pl(r, g, lambda_dssim=0.2, **kw)
    with pytest.raises(ValueError, match="float32"):
        pl(r.double(), gt.double(), lambda_dssim=0.2)
    with pytest.raises(ValueError, match="float32"):
        pl(r, gt, lambda_dssim=0.2, alpha_mask=plane.half())
    with pytest.raises(ValueError, match="GPU tensor"):
        pl(r, gt, lambda_dssim=0.2)
    with pytest.raises(ValueError, match="GPU tensor"):
        pl(r[None], gt[None], lambda_dssim=0.2, exposure=torch.eye(3, 4)[None], alpha_mask=plane[None])


def test_existing_loss_functions_are_untouched():
    """l1_loss is still the reference's expression, and ssim's checks still speak for themselves."""
    from hgs import loss
    a, b = torch.rand(3, 5, 7), torch.rand(3, 5, 7)
    assert torch.equal(loss.l1_loss(a, b), torch.abs(a - b).mean())
    with pytest.raises(ValueError, match="hgs.loss.ssim"):
        loss.ssim(a, b)


# -- kernel resources ---------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("c++filt")),
                    reason="needs hipcc (cross-compiles without a GPU) and c++filt")
def test_photometric_kernels_compile_for_gfx950_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    rows = kernel_resources.collect([os.path.join(CSRC, "photometric.hip")])
    names = {r["kernel"].split("<")[0] for r in rows}
    assert {"photo_fwd_kernel", "photo_bwd_kernel", "photo_reduce_kernel", "photo_exposure_reduce_kernel"} <= names, names
    for r in rows:
        print(f"{r['kernel']}: {min(r['waves_regs'], r['waves_lds'])} waves per SIMD (registers {r['waves_regs']}, "
              f"LDS {r['waves_lds']}), LDS {r['lds']} bytes, VGPRs {r['vgpr']}, scratch {r['scratch']}")
        assert r["scratch"] == 0, r


# -- the inputs of tests/test_photometric_edges_gpu.py: their conditions hold, checked without a GPU -------------------

def _u_of(inp):
    four = inp["rendered"].dim() == 4
    r = (inp["rendered"] if four else inp["rendered"][None]).double()
    E = inp.get("exposure")
    u, _ = spec.transform(r, None if E is None else E.double().reshape(-1, 3, 4), inp["clamp"], None)
    return u


@pytest.mark.parametrize("H,W,C_,N,content", pc.SWEEP)
def test_small_cases_are_not_degenerate(H, W, C_, N, content):
    """Every case of the off-grid sweep: empty bands, the three gradients of the spec non-zero (a kernel that writes
    zeros cannot pass), masks in {0, 0.5, 1}, a per-image exposure at C = 3, and from 16 pixels per image on one pixel
    of every special kind."""
    inp = pc.sweep_case(H, W, C_, N, content)
    assert pc.band_counts(inp) == (0, 0, 0)
    assert inp["rendered"].shape == ((C_, H, W) if N is None else (N, C_, H, W))
    assert all(v.dtype == torch.float32 for v in inp.values() if isinstance(v, torch.Tensor))
    assert ("exposure" in inp) == (C_ == 3)
    want = spec.loss_and_grads(lambda_dssim=0.2, depth_weight=0.7, **inp)
    for k in ("grad_rendered", "grad_invdepth") + (("grad_exposure",) if C_ == 3 else ()):
        assert want[k].norm().item() > 0, k
    for k in ("alpha_mask", "depth_mask"):
        assert set(inp[k].unique().tolist()) <= {0.0, 0.5, 1.0}, k
    if C_ == 3 and N is not None:
        E = inp["exposure"]
        assert E.shape == (N, 3, 4) and not torch.equal(E[0], E[1])
        assert 1.7 < E[0, :, :3].diagonal().mean().item() < 2.3 and -0.4 < E[1, :, 3].mean().item() < -0.2
        for n in range(N):       # every image of the batch carries gradient of its own
            assert want["grad_rendered"][n].norm().item() > 0 and want["grad_exposure"][n].norm().item() > 0
            assert want["grad_invdepth"][n].norm().item() > 0
    if H * W >= 16:
        u = _u_of(inp)
        out, r = (u < 0) | (u > 1), inp["rendered"]
        assert bool(out.any()) and bool((~out).any())
        assert bool((r < 0).any()) and bool((r > 1).any())
        q = (inp["invdepth"].double() - inp["mono_invdepth"].double()) * inp["depth_mask"].double()
        assert bool((inp["alpha_mask"] == 0).any()) and bool((inp["alpha_mask"] == 0.5).any())
        assert bool((q == 0).any()) and bool((inp["invdepth"] == inp["mono_invdepth"]).any())
        assert bool((inp["depth_mask"] == 0.5).any())


def test_the_sweep_covers_every_size_batch_and_channel_count():
    assert {w for _, w, *_ in pc.SWEEP} == {1, 2, 5, 6, 11, 31, 32, 33, 64, 65}
    assert {h for h, *_ in pc.SWEEP} == {1, 2, 5, 6, 15, 16, 17, 33}
    hw = {(h, w) for h, w, *_ in pc.SWEEP}
    assert (1, 1) in hw and any(h == 1 and w > 1 for h, w in hw) and any(w == 1 and h > 1 for h, w in hw)
    assert {n for *_, n, _ in pc.SWEEP} == {None, 2}
    assert {c for _, _, c, *_ in pc.SWEEP} == {1, 2, 3, 4}
    assert {k for *_, k in pc.SWEEP} == {"random", "smooth"}
    assert len(set(pc.SWEEP)) == len(pc.SWEEP)


def test_make_degenerates_where_small_does_not():
    """Why the sweep has a generator of its own: at W = 1 `make` masks every pixel, at H = 1 its depth term has q == 0
    everywhere; the spec's gradients are then identically zero."""
    a = spec.loss_and_grads(lambda_dssim=0.2, depth_weight=0.7, **pc.make((3, 33, 1), seed=1))
    assert a["grad_rendered"].norm().item() == 0 and a["grad_exposure"].norm().item() == 0
    b = spec.loss_and_grads(lambda_dssim=0.2, depth_weight=0.7, **pc.make((3, 1, 9), seed=1))
    assert b["grad_invdepth"].norm().item() == 0
    for shape in ((3, 33, 1), (3, 1, 9), (3, 1, 1)):
        c = spec.loss_and_grads(lambda_dssim=0.2, depth_weight=0.7, **pc.small(shape, seed=1))
        assert all(c[k].norm().item() > 0 for k in ("grad_rendered", "grad_exposure", "grad_invdepth")), shape


def test_impulse_image_has_exact_zeros_far_from_every_impulse():
    """The spec on the impulse batch: more than 10 pixels (Chebyshev) from every impulse grad_rendered is exactly zero
    in all three channels -- u = 0 passes the inclusive gate, x = gt = 0, every window that reaches the pixel sees
    zeros, A = 0 and sign(0) = 0 -- and the all-zero second image has zero gradients."""
    import test_ssim_gpu as ts
    inp, points = pc.impulses()
    assert pc.band_counts(inp) == (0, 0, 0)
    assert {x % 32 for _, x in ts.IMPULSES_1[:12]} == {0, 4, 5, 26, 27, 31}
    assert {y % 16 for y, _ in ts.IMPULSES_1[:12]} == {0, 4, 5, 10, 11, 15}
    far = ts._far_from(points, ts.IMP_H, ts.IMP_W, 10)
    print("pixels far from every impulse:", int(far.sum()))
    assert int(far.sum()) == 3919
    want = spec.loss_and_grads(lambda_dssim=0.2, **inp)
    g = want["grad_rendered"]
    assert bool((g[0][:, far] == 0).all()) and bool((g[0][:, ~far] != 0).any())
    assert bool((g[1] == 0).all()) and bool((want["grad_exposure"][1] == 0).all())
    assert bool((want["grad_exposure"][0] != 0).sum() >= 10)     # r_0 du_2 and r_2 du_0 are clamped away: u = -0.05 r
    for i, (y, x) in enumerate(ts.IMPULSES_1):      # one channel in, every channel out
        near = g[0][:, max(0, y - 5): y + 6, max(0, x - 5): x + 6]
        assert bool((near != 0).flatten(1).any(dim=1).all()), (i, y, x)


def test_closed_forms_agree_with_the_spec():
    """lambda_dssim = 0 without an exposure leaves the L1 gradient alone, and the depth gradient is a sign times one
    constant whatever lambda is -- with a soft and a negative depth mask too.  In float64 the L1 restatement is the
    spec's own expression, to the bit.  The depth restatement forms its constant in the kernel's order,
    (depth_weight / count) * g, and the spec in the order depth_weight * g / count: two roundings of a double apart, so
    it is held to 1e-15 of its largest value."""
    inp = pc.make((3, 37, 53), seed=11, exposure=False)
    inp = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    assert int((inp["rendered"] == 0).sum()) > 50
    got = spec.loss_and_grads(lambda_dssim=0.0, depth_weight=0.7, grad_out=-1.75, **inp)
    assert torch.equal(got["grad_rendered"], pc.l1_closed_form(inp, -1.75, torch.float64))
    assert got["grad_rendered"].norm().item() > 0
    g = torch.Generator().manual_seed(3)
    levels = torch.tensor([-0.75, 0.0, 0.3, 0.5, 1.0], dtype=torch.float64)
    inp["depth_mask"] = levels[torch.randint(0, 5, inp["depth_mask"].shape, generator=g)]
    for lam in (0.0, 0.2, 1.0):
        got = spec.loss_and_grads(lambda_dssim=lam, depth_weight=0.7, grad_out=-1.75, **inp)
        want = pc.depth_closed_form(inp, 0.7, -1.75, torch.float64)
        assert (got["grad_invdepth"] - want).abs().max().item() <= 1e-15 * want.abs().max().item()
        assert bool((got["grad_invdepth"][inp["depth_mask"] < 0] != 0).any())
