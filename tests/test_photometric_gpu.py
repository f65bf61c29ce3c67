"""The fused training loss on the device (hgs.loss.photometric_loss, csrc/photometric.hip) against the float64 spec
(tests/photometric_spec.py).

Parity follows the project's "as good as float32" rule (tests/test_ssim_gpu.py): the yardstick is the float32 CPU
evaluation of the reference's torch lines (photometric_spec.torch_formula with tests/train_loop.ssim, autograd for the
gradients).  The kernels' errors against the spec may be at most max(2e-6, 3x) the yardstick's for each of the four
values, max(2^-22, 1.5x) its relative L2 and max(2^-22, 3x) its largest deviation over the spec's maximum for each
gradient.  2^-22 is two float32 roundings of one result: the float32 yardstick's depth gradient, a sign times one
constant, is off by only 2e-9.

No pixel is left out.  The inputs (tests/photometric_cases.py) are repaired until the float64 spec finds the knife-edge
bands, taken ten times wider than the condition (1e-4 / 1e-5 / 1e-5), empty; every test asserts that."""
import ctypes as C

import pytest
import torch

import photometric_cases as pc
import photometric_spec as spec
import train_loop as tl
import ws_guard

pytestmark = pytest.mark.gpu

LAM, DW = 0.2, 0.7


def check_case(inp, dev, what, lam=LAM, dw=DW):
    assert pc.band_counts(inp) == (0, 0, 0), "a pixel sits in a knife-edge band"
    want = spec.loss_and_grads(lambda_dssim=lam, depth_weight=dw, **inp)
    yard = pc.formula(inp, lam, dw, torch.float32)
    got = pc.fused(inp, lam, dw, dev)
    pc.assert_parity(got, yard, want, what)
    return got, want


@pytest.mark.parametrize("shape", [(3, 1080, 1920), (3, 37, 53), (2, 3, 270, 480), (3, 8, 9)])
def test_parity_with_the_spec(gpu, shape):
    check_case(pc.make(shape, seed=1), gpu, str(shape))


@pytest.mark.parametrize("off", ["exposure", "alpha_mask", "depth", "clamp"])
def test_parity_with_each_optional_input_off(gpu, off):
    inp = pc.make((3, 270, 480), seed=2, exposure=off != "exposure", mask=off != "alpha_mask", depth=off != "depth",
                  clamp=off != "clamp")
    got, _ = check_case(inp, gpu, f"without {off}")
    if off == "depth":
        assert got["depth"].item() == 0.0 and got["grad_invdepth"] is None


def test_the_reference_fixture_on_the_device(gpu):
    """The inputs recorded with the reference's own numbers (tests/golden/ref_photometric_golden.npz), rounded to
    float32, under the same rule; the train_post-shaped case asks for no exposure gradient."""
    from test_photometric_cpu import golden_cases
    for name, inp, lam, dw, exposure_grad, _ in golden_cases():
        inp = pc.repair({k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()})
        grads = ("rendered", "exposure", "invdepth") if exposure_grad else ("rendered", "invdepth")
        want = spec.loss_and_grads(lambda_dssim=lam, depth_weight=dw, **inp)
        if not exposure_grad:
            want["grad_exposure"] = None
        pc.assert_parity(pc.fused(inp, lam, dw, gpu, grads), pc.formula(inp, lam, dw, torch.float32, grads), want, name)


def _same(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in a)


def test_two_calls_and_two_streams_are_bit_identical(gpu):
    inp = pc.make((2, 3, 135, 241), seed=3)
    a, b = pc.fused(inp, LAM, DW, gpu), pc.fused(inp, LAM, DW, gpu)
    assert _same(a, b)
    m = torch.rand(2048, 2048, device=gpu)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(gpu)
    with torch.cuda.stream(s):
        for _ in range(8):                            # work queued on the side stream ahead of the loss
            m = m @ m / 2048.0
        c = pc.fused(inp, LAM, DW, gpu)
    s.synchronize()
    assert _same(a, c)


def _requested(dev, what):
    """Bytes the code asked the caching allocator for (``what``: "current" or "peak").  Not allocated_bytes: a block of
    more than 1 MB that leaves less than 1 MB of its 2 MB-rounded segment over is handed out whole, so that figure
    carries up to 1 MB of the allocator's own rounding per large tensor."""
    return torch.cuda.memory_stats(dev)[f"requested_bytes.all.{what}"]


def _on(inp, dev):
    t = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    return t.pop("rendered"), t.pop("gt"), t


def test_no_grad_gives_the_same_values_and_allocates_no_maps(gpu):
    from hgs.loss import photometric_loss
    inp = pc.make((3, 540, 960), seed=4)
    ref = pc.fused(inp, LAM, DW, gpu)
    r, gt, kw = _on(inp, gpu)
    maps_bytes = 3 * r.numel() * 4
    for mode in ("no_grad", "nothing requires grad"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(gpu)
        before = _requested(gpu, "current")
        if mode == "no_grad":
            with torch.no_grad():
                res = photometric_loss(r.clone().requires_grad_(True), gt, lambda_dssim=LAM, depth_weight=DW, **kw)
        else:
            res = photometric_loss(r, gt, lambda_dssim=LAM, depth_weight=DW, **kw)
        torch.cuda.synchronize()
        extra = _requested(gpu, "peak") - before
        assert not res.loss.requires_grad
        for k in ("loss", "l1", "ssim", "depth"):
            assert torch.equal(getattr(res, k).cpu(), ref[k]), (mode, k)
        # the rendered clone of the no_grad branch (one image) and the workspace, but not the three maps
        assert extra <= r.numel() * 4 + (1 << 20) < maps_bytes, (mode, extra)


def test_the_four_values_share_one_buffer(gpu):
    from hgs.loss import photometric_loss
    r, gt, kw = _on(pc.make((3, 37, 53), seed=5), gpu)
    for rg in (False, True):
        res = photometric_loss(r.clone().requires_grad_(rg), gt, lambda_dssim=LAM, depth_weight=DW, **kw)
        base = res.loss.data_ptr()
        assert [t.data_ptr() - base for t in res] == [0, 4, 8, 12]
        assert all(t.dim() == 0 and t.dtype == torch.float32 for t in res)
        assert res.loss.requires_grad == rg and not (res.l1.requires_grad or res.ssim.requires_grad or res.depth.requires_grad)


def test_gradient_is_exactly_zero_where_the_mask_is_zero_or_the_clamp_is_active(gpu):
    inp = pc.make((3, 270, 480), seed=6)
    # a mixing exposure without offsets: the flat block of the input (r = -0.05 in every channel) stays below 0
    inp["exposure"] = torch.eye(3, 4) + 0.05 * torch.tensor([[0., 1, -1, 0], [1, 0, 1, 0], [-1, 1, 0, 0]])
    inp = pc.repair(inp)
    got = pc.fused(inp, LAM, DW, gpu)
    masked = (inp["alpha_mask"] == 0).expand(3, -1, -1)
    assert int(masked.sum()) > 1000 and bool((got["grad_rendered"][masked] == 0).all())
    u, _ = spec.transform(inp["rendered"].double()[None], inp["exposure"].double()[None], True, None)
    out_all = ((u[0] < 0) | (u[0] > 1)).all(dim=0)          # every output channel clamped: no path to any r_i
    assert int(out_all.sum()) > 100 and bool((got["grad_rendered"][:, out_all] == 0).all())
    # without an exposure the channels do not mix: zero exactly where that channel's u is outside [0, 1]
    inp = pc.make((3, 270, 480), seed=6, exposure=False)
    got = pc.fused(inp, LAM, DW, gpu)
    outside = (inp["rendered"] < 0) | (inp["rendered"] > 1)
    assert int(outside.sum()) > 1000 and bool((got["grad_rendered"][outside] == 0).all())
    inside = ~outside & (inp["alpha_mask"] > 0).expand(3, -1, -1)
    assert (got["grad_rendered"][inside] != 0).float().mean().item() > 0.99


def test_the_plain_case_agrees_with_l1_and_the_fused_ssim(gpu):
    """exposure=None, clamp=False, no mask, no depth: the call against (1 - l) l1_loss + l (1 - hgs.loss.ssim), both
    within the rule of the spec."""
    from hgs import loss
    inp = pc.make((3, 270, 480), seed=7, exposure=False, mask=False, depth=False, clamp=False)
    got, want = check_case(inp, gpu, "plain")
    a = inp["rendered"].to(gpu).requires_grad_(True)
    g = inp["gt"].to(gpu)
    l = (1.0 - LAM) * loss.l1_loss(a, g) + LAM * (1.0 - loss.ssim(a, g))
    l.backward()
    comp = dict(got, loss=l.detach().cpu(), grad_rendered=a.grad.cpu())
    pc.assert_parity(comp, pc.formula(inp, LAM, DW, torch.float32), want, "l1_loss + hgs.loss.ssim")
    print("fused vs composition: loss", abs(got["loss"].item() - comp["loss"].item()), "grad max",
          (got["grad_rendered"] - comp["grad_rendered"]).abs().max().item())


GUARD_SHAPES = [(2, 3, 37, 53), (3, 8, 9), (3, 16, 32)]
# one pixel, one row, one column per image and one tile of one channel: pc.small's inputs (pc.make has no gradient at
# W = 1 and takes C = 3)
GUARD_SMALL = [(1, 3, 1, 1), (3, 1, 65), (2, 3, 33, 1), (1, 1, 16, 32)]


@pytest.mark.parametrize("shape", GUARD_SHAPES + GUARD_SMALL)
def test_buffers_handed_to_the_c_abi_stay_in_bounds(gpu, shape):
    """Every buffer of hgs_photo_fwd / hgs_photo_bwd between guard bytes, outputs pre-filled with 0x00 and with 0xFF:
    the guards are intact, the inputs unchanged and the results the same bits (nothing unwritten is read).  Once with
    every optional input the shape admits, and once with every optional pointer, grad_exposure and grad_invdepth NULL."""
    inp = pc.make(shape, seed=8) if shape in GUARD_SHAPES else pc.small(shape, seed=8)
    _guarded_calls(gpu, shape, inp)
    off = dict(exposure=False, mask=False, depth=False)
    _guarded_calls(gpu, shape, pc.make(shape, seed=8, **off) if shape in GUARD_SHAPES else pc.small(shape, seed=8, **off))


def _guarded_calls(gpu, shape, inp):
    from hgs import _lib
    lib = _lib.lib()
    assert pc.band_counts(inp) == (0, 0, 0)
    N, Ch, H, W = shape if len(shape) == 4 else (1,) + shape
    up = torch.tensor([-1.75])
    stream = lambda: C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def run(fill):
        gs, t = [], {}

        def buf(name, like=None, nbytes=None):
            g = ws_guard.guarded(like.numel() * 4 if like is not None else nbytes, gpu, fill, name)
            if like is not None:
                g.view(torch.float32).copy_(like.reshape(-1).to(gpu))
            gs.append(g)
            return g

        for k in ("rendered", "gt") + pc.OPTIONAL:
            if k in inp:
                t[k] = buf(k, like=inp[k])
        g_up = buf("grad_out", like=up)
        out, maps = buf("out", nbytes=16), buf("maps", nbytes=3 * N * Ch * H * W * 4)
        tmp_f, tmp_b = (buf(n, nbytes=lib.hgs_photo_tmp_bytes(N, Ch, H, W)) for n in ("tmp fwd", "tmp bwd"))
        grad_r = buf("grad_rendered", nbytes=N * Ch * H * W * 4)
        grad_E = buf("grad_exposure", nbytes=N * 48) if "exposure" in inp else None
        grad_d = buf("grad_invdepth", nbytes=N * H * W * 4) if "invdepth" in inp else None
        addr = lambda g: None if g is None else g.addr
        args = _lib.PhotoArgs(**{k: t[k].addr for k in t}, N=N, C=Ch, H=H, W=W, clamp=1, reserved=0, lambda_dssim=LAM,
                              depth_weight=DW)
        _lib.check(lib.hgs_photo_fwd(C.byref(args), out.addr, maps.addr, tmp_f.addr, stream(), gpu.index or 0), "fwd")
        _lib.check(lib.hgs_photo_bwd(C.byref(args), maps.addr, g_up.addr, grad_r.addr, addr(grad_E), addr(grad_d),
                                     tmp_b.addr, stream(), gpu.index or 0), "bwd")
        out0 = buf("out (maps = NULL)", nbytes=16)
        tmp0 = buf("tmp (maps = NULL)", nbytes=lib.hgs_photo_tmp_bytes(N, Ch, H, W))
        _lib.check(lib.hgs_photo_fwd(C.byref(args), out0.addr, None, tmp0.addr, stream(), gpu.index or 0), "fwd")
        ws_guard.check(*gs)
        for k in t:
            assert torch.equal(t[k].view(torch.float32).cpu(), inp[k].reshape(-1)), f"{k} was modified"
        assert torch.equal(out.view(torch.float32), out0.view(torch.float32))
        return {n: g.view(torch.float32).cpu().clone() for n, g in
                (("out", out), ("maps", maps), ("grad_rendered", grad_r), ("grad_exposure", grad_E),
                 ("grad_invdepth", grad_d)) if g is not None}

    a, b = run(0x00), run(0xFF)
    for k in a:
        assert torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k]).all()), k
    want = spec.loss_and_grads(lambda_dssim=LAM, depth_weight=DW, grad_out=-1.75, **inp)
    assert abs(a["out"][0].item() - want["loss"].item()) <= 1e-5
    for k in ("grad_rendered", "grad_exposure", "grad_invdepth"):
        assert (k in a) == (want[k] is not None), k
        if k in a:
            w = want[k].reshape(-1)
            assert w.norm().item() > 0, k
            assert ((a[k].double() - w).norm() / w.norm()).item() <= 1e-4, k


def test_peak_memory_is_the_maps_and_the_gradients(gpu):
    from hgs.loss import photometric_loss
    r, gt, kw = _on(pc.make((3, 1080, 1920), seed=9), gpu)
    r.requires_grad_(True)
    kw["exposure"].requires_grad_(True)
    kw["invdepth"].requires_grad_(True)
    photometric_loss(r, gt, lambda_dssim=LAM, depth_weight=DW, **kw).loss.backward()       # warm-up
    r.grad = kw["exposure"].grad = kw["invdepth"].grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    before = _requested(gpu, "current")
    photometric_loss(r, gt, lambda_dssim=LAM, depth_weight=DW, **kw).loss.backward()
    torch.cuda.synchronize()
    extra = _requested(gpu, "peak") - before
    allowed = 3 * r.numel() * 4 + (r.numel() + 12 + kw["invdepth"].numel()) * 4 + (1 << 20)
    print(f"peak above the inputs {extra} bytes, allowed {allowed}")
    assert extra <= allowed


def test_training_with_the_fused_loss_matches_the_torch_composition(gpu, monkeypatch):
    """test_ssim_gpu's training problem on the HIP renderer: thirty steps with train_loop.optimise's torch lines, and
    thirty with its colour and depth terms computed by one photometric_loss call, from the same jittered start."""
    from hgs.loss import photometric_loss
    cams, scene = tl.make_problem(P=8000, size=320, height=192, n_views=6, seed=1)
    steps, dssim, dw = 30, 0.2, 0.1
    bg = torch.zeros(3)
    oracle = tl.oracle_render_fn(bg, 3, torch.float64)
    hipr = tl.hip_render_fn(bg, 3, gpu)
    with torch.no_grad():
        gt = {k: v.detach() for k, v in tl.activate(tl.raw_params_from_scene(scene, "cpu")).items()}
        targets = [oracle(c, gt) for c in cams]
    raw_t = tl.raw_params_from_scene(scene, gpu, jitter_seed=5)
    loss_t = tl.optimise(hipr, raw_t, cams, targets, steps, depth_weight=dw, lambda_dssim=dssim)
    p_t = tl.evaluate(hipr, raw_t, cams, targets)

    raw_f = tl.raw_params_from_scene(scene, gpu, jitter_seed=5)
    opt = torch.optim.Adam([dict(params=[raw_f[k]], lr=tl.LRS[k], name=k) for k in tl.LRS], eps=1e-15)
    ones = torch.ones(1, 192, 320, device=gpu)
    loss_f = []
    for it in range(steps):                     # tl.optimise with the loss lines replaced by the one call
        k = it % len(cams)
        color, invd = hipr(cams[k], tl.activate(raw_f))
        tc, td = targets[k]
        res = photometric_loss(color, tc.to(color), lambda_dssim=dssim, clamp=False, invdepth=invd,
                               mono_invdepth=td.to(invd), depth_mask=ones, depth_weight=dw)
        opt.zero_grad(set_to_none=True)
        res.loss.backward()
        opt.step()
        loss_f.append(res.loss.item())
    p_f = tl.evaluate(hipr, raw_f, cams, targets)
    print(f"loss {loss_t[0]:.6f}->{loss_t[-1]:.6f} (torch) / {loss_f[0]:.6f}->{loss_f[-1]:.6f} (fused); "
          f"PSNR {p_t:.4f} / {p_f:.4f} dB")
    assert abs(loss_f[0] - loss_t[0]) <= 1e-5 * abs(loss_t[0])
    assert abs(p_f - p_t) <= 0.01


def test_rejections_on_the_device(gpu):
    from hgs.loss import photometric_loss as pl
    r, gt = torch.rand(3, 16, 16, device=gpu), torch.rand(3, 16, 16, device=gpu)
    plane, E = torch.rand(1, 16, 16, device=gpu), torch.eye(3, 4, device=gpu)
    with pytest.raises(ValueError, match="float32"):
        pl(r.half(), gt.half(), lambda_dssim=0.2)
    with pytest.raises(ValueError, match="float32"):
        pl(r, gt, lambda_dssim=0.2, exposure=E.double())
    with pytest.raises(ValueError, match="shapes differ"):
        pl(r, gt[:, :, :15], lambda_dssim=0.2)
    with pytest.raises(ValueError, match="exposure needs C = 3"):
        pl(torch.rand(4, 16, 16, device=gpu), torch.rand(4, 16, 16, device=gpu), lambda_dssim=0.2, exposure=E)
    with pytest.raises(ValueError, match="incomplete depth triple"):
        pl(r, gt, lambda_dssim=0.2, invdepth=plane, depth_mask=plane)
    with pytest.raises(ValueError, match="gt requires grad"):
        pl(r, gt.clone().requires_grad_(True), lambda_dssim=0.2)
    with pytest.raises(ValueError, match="alpha_mask requires grad"):
        pl(r, gt, lambda_dssim=0.2, alpha_mask=plane.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="mono_invdepth requires grad"):
        pl(r, gt, lambda_dssim=0.2, invdepth=plane, mono_invdepth=plane.clone().requires_grad_(True), depth_mask=plane)
    with pytest.raises(ValueError, match="lambda_dssim"):
        pl(r, gt, lambda_dssim=1.0001)
    with pytest.raises(ValueError, match="GPU tensor"):
        pl(r, gt, lambda_dssim=0.2, alpha_mask=plane.cpu())
    res = pl(r, gt, lambda_dssim=0.2, exposure=E, alpha_mask=plane[0], invdepth=plane, mono_invdepth=plane[0],
             depth_mask=plane)                  # (H,W) and (1,H,W) planes both pass
    assert bool(torch.isfinite(torch.stack(list(res))).all())
