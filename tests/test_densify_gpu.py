"""hgs.densify on the GPU: the kernels against the reference's recorded outputs (tests/golden/ref_densify_golden.npz)
and against the torch statement of the rule (tests/densify_spec.py) run on the same device; corner classes; the C ABI
called directly between guard bytes; determinism and streams; the model-level switch-over with real optimizers, an
optimizer step and a rasterizer forward + backward at the new row count; error paths that leave the model untouched.

Inputs never hold a row within 1e-4 (relative, float64) of a threshold: such rows are re-drawn on the host
(tests/densify_cases.py), and the re-drawn share is asserted to stay at or below 1 %."""
import ctypes as C
import math

import pytest
import torch

import densify_cases as dc
import parity as pa
import ws_guard as wg
from densify_spec import NAMES, classes, densify_and_prune_spec
from hgs import _lib, densify, optim, synth

pytestmark = pytest.mark.gpu

ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
             rotation="_rotation")
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=5e-2, scaling=5e-3, rotation=1e-3)


def _fused(case, **kw):
    return densify.densify_and_prune_tensors(*dc.call_args(case), **kw)


def _spec(case, **kw):
    return densify_and_prune_spec(*dc.call_args(case), **kw)


@pytest.mark.parametrize("name", dc.golden_case_names())
def test_kernels_reproduce_the_reference(gpu, name):
    case = dc.load_case(name, gpu)
    got = _fused(case, noise=case["noise"])
    print(name, "totals", got[2])
    dc.assert_same_result(got, (case["out"], case["out_m"], case["totals"]), name)
    again = dc.load_case(name, gpu)
    for n in NAMES:                                     # the inputs are untouched
        assert dc.same_bits(case["tensors"][n], again["tensors"][n])


@pytest.mark.parametrize("K", [0, 3, 15])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 257, 1_000, 100_003, 1_000_000])
def test_kernels_against_the_spec(gpu, P, K):
    for F in (0, P // 2, P):
        case = dc.make_inputs(P, K, 1000 + P % 997 + K, gpu)
        case["F"] = F
        assert case["redrawn"] <= 0.01, case["redrawn"]
        S = _spec_split_rows(case)
        noise = torch.randn((2 * S, 3), generator=torch.Generator(device=gpu).manual_seed(P + K), device=gpu)
        ref = _spec(case, noise=noise)
        got = _fused(case, noise=noise)
        print(f"P {P} K {K} F {F}: totals {got[2]}, re-drawn share {case['redrawn']:.1e}")
        dc.assert_same_result(got, ref, f"P={P} K={K} F={F}")


def _spec_split_rows(case):
    return int(classes(case["accum"], case["radii"], case["tensors"]["opacity"], case["tensors"]["scaling"], case["F"],
                       case["max_grad"], case["min_opacity"], case["d"])[1].sum())


def _corner(gpu, P, K, kind, with_moments=True):
    """Inputs in which every row has the same class: 'split', 'clone', 'prune', 'none'."""
    case = dc.make_inputs(P, K, 77, gpu, with_moments=with_moments)
    case["F"] = 0
    case["accum"] = torch.full((P, 1), 5.0, device=gpu)
    case["radii"] = torch.full((P,), 10.0, device=gpu)
    case["tensors"]["opacity"] = torch.full((P, 1), 2.0, device=gpu)            # sigmoid = 0.88
    case["max_grad"], case["min_opacity"] = 1.0, 0.1
    m_mid = math.exp(-3.0)
    if kind == "split":
        case["d"] = m_mid * 1e-3
    elif kind == "clone":
        case["d"] = m_mid * 1e3
    elif kind == "prune":
        case["max_grad"] = 1e9
        case["tensors"]["opacity"] = torch.full((P, 1), -5.0, device=gpu)       # sigmoid = 0.0067 < 0.1
    else:
        case["max_grad"] = 1e9
    return case


@pytest.mark.parametrize("kind,expect", [("split", lambda P: (0, 0, P, P)), ("clone", lambda P: (P, P, 0, 0)),
                                         ("prune", lambda P: (0, 0, 0, 0)), ("none", lambda P: (P, 0, 0, 0))])
def test_corner_classes(gpu, kind, expect):
    P = 1000
    case = _corner(gpu, P, 3, kind)
    noise = torch.randn((2 * P, 3), generator=torch.Generator().manual_seed(3)).to(gpu)[:2 * expect(P)[2]].contiguous()
    got = _fused(case, noise=noise)
    assert got[2] == expect(P)
    dc.assert_same_result(got, _spec(case, noise=noise), kind)
    if kind == "prune":
        assert all(got[0][n].shape[0] == 0 for n in NAMES)


def test_moments_absent_and_partly_absent(gpu):
    case = dc.make_inputs(777, 3, 5, gpu, with_moments=False)
    case["F"] = 10
    S = _spec_split_rows(case)
    noise = torch.randn((2 * S, 3), generator=torch.Generator().manual_seed(4)).to(gpu)
    got = _fused(case, noise=noise)
    assert all(got[1][n] is None for n in NAMES)
    dc.assert_same_result(got, _spec(case, noise=noise), "no moments")
    full = dc.make_inputs(777, 3, 5, gpu)
    full["F"] = 10
    full["moments"]["f_dc"] = None                      # a parameter without optimizer state gets none
    del full["moments"]["rotation"]
    got = _fused(full, noise=noise)
    assert got[1]["f_dc"] is None and got[1]["rotation"] is None and got[1]["xyz"] is not None
    dc.assert_same_result(got, _spec(full, noise=noise), "some moments")


def test_f_rest_of_zero_width_is_skipped(gpu):
    case = dc.make_inputs(300, 0, 9, gpu)
    case["F"] = 0
    S = _spec_split_rows(case)
    noise = torch.randn((2 * S, 3), generator=torch.Generator().manual_seed(4)).to(gpu)
    got = _fused(case, noise=noise)
    assert tuple(got[0]["f_rest"].shape) == (got[0]["xyz"].shape[0], 0, 3)
    dc.assert_same_result(got, _spec(case, noise=noise), "K=0")


def test_noise_from_a_generator_is_reproducible(gpu):
    case = dc.make_inputs(5000, 3, 21, gpu)
    case["F"] = 0
    a = _fused(case, generator=torch.Generator(device=gpu).manual_seed(11))
    b = _fused(case, generator=torch.Generator(device=gpu).manual_seed(11))
    z = torch.randn((2 * a[2][2], 3), generator=torch.Generator(device=gpu).manual_seed(11), device=gpu)
    c = _fused(case, noise=z)
    for n in NAMES:
        assert dc.same_bits(a[0][n], b[0][n]) and dc.same_bits(a[0][n], c[0][n]), n


def test_two_calls_are_bit_identical_and_streams_agree(gpu):
    case = dc.make_inputs(100_003, 15, 31, gpu)
    case["F"] = 1234
    S = _spec_split_rows(case)
    noise = torch.randn((2 * S, 3), generator=torch.Generator().manual_seed(4)).to(gpu)
    a = _fused(case, noise=noise)
    b = _fused(case, noise=noise)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        c = _fused(case, noise=noise)
    side.synchronize()
    assert a[2] == b[2] == c[2]
    for n in NAMES:
        for x, y in ((a, b), (a, c)):
            assert dc.same_bits(x[0][n], y[0][n]), n
            assert dc.same_bits(x[1][n][0], y[1][n][0]) and dc.same_bits(x[1][n][1], y[1][n][1]), n


@pytest.mark.parametrize("P", [1, 65, 257, 1003])
def test_c_abi_between_guard_bytes(gpu, P):
    """Plan and apply called directly with separately allocated workspace, totals and outputs, each between two guards,
    once with the free buffers filled with 0x00 and once with 0xFF: intact guards, bitwise equal results, spec values."""
    lib = _lib.lib()
    K = 3
    case = dc.make_inputs(P, K, 400 + P, gpu)
    case["F"] = P // 3
    S = _spec_split_rows(case)
    noise = torch.randn((2 * S + 2, 3), generator=torch.Generator().manual_seed(4)).to(gpu)[:2 * S].contiguous()
    ref = _spec(case, noise=noise)
    rows = ref[0]["xyz"].shape[0]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = []
    for fill in (0x00, 0xFF):
        gs = []

        def new(name, nbytes):
            g = wg.guarded(nbytes, gpu, fill, name)
            gs.append(g)
            return g
        tmp = new("tmp", lib.hgs_densify_tmp_bytes(P))
        totals = new("totals", 32)
        _lib.check(lib.hgs_densify_plan(_lib.ptr(case["accum"]), _lib.ptr(case["radii"]), _lib.ptr(case["tensors"]["opacity"]),
                                        _lib.ptr(case["tensors"]["scaling"]), P, case["F"], case["max_grad"],
                                        case["min_opacity"], case["d"], C.c_void_p(tmp.addr), C.c_void_p(totals.addr), 0,
                                        stream, 0), "hgs_densify_plan")
        tot = tuple(int(v) for v in totals.view(torch.int64).cpu())
        assert tot == ref[2], (tot, ref[2])
        out, out_m, descs = {}, {}, []
        for n in NAMES:
            t = case["tensors"][n]
            row_len = t[0].numel()
            bufs = [new(f"{n}.{w}", max(rows, 0) * row_len * 4) for w in ("dst", "exp_avg", "exp_avg_sq")]
            shape = (rows,) + tuple(t.shape[1:])
            out[n] = bufs[0].view(torch.float32, *shape)
            out_m[n] = (bufs[1].view(torch.float32, *shape), bufs[2].view(torch.float32, *shape))
            mv = case["moments"][n]
            descs.append(_lib.DensifyTensor(src=t.data_ptr(), exp_avg=mv[0].data_ptr(), exp_avg_sq=mv[1].data_ptr(),
                                            dst=bufs[0].addr, dst_exp_avg=bufs[1].addr, dst_exp_avg_sq=bufs[2].addr,
                                            row_len=row_len, kind={"xyz": 1, "scaling": 2}.get(n, 0)))
        arr = (_lib.DensifyTensor * len(descs))(*descs)
        _lib.check(lib.hgs_densify_apply(arr, len(descs), P, (C.c_int64 * 4)(*tot), _lib.ptr(case["tensors"]["scaling"]),
                                         _lib.ptr(case["tensors"]["rotation"]), _lib.ptr(noise) if S else None,
                                         C.c_void_p(tmp.addr), stream, 0), "hgs_densify_apply")
        wg.check(*gs)
        dc.assert_same_result((out, out_m, tot), ref, f"P={P} fill={fill:#x}")
        results.append((out, out_m))
    for n in NAMES:
        assert dc.same_bits(results[0][0][n], results[1][0][n]), n
        assert dc.same_bits(results[0][1][n][0], results[1][1][n][0]) and dc.same_bits(results[0][1][n][1], results[1][1][n][1]), n


# ---- model level ---------------------------------------------------------------------------------------------------
class Model:
    """The reference's GaussianModel as far as densify_and_prune sees it (duck typed)."""

    def __init__(self, tensors, make_optimizer, F, percent_dense=0.01):
        for n in NAMES:
            setattr(self, ATTRS[n], torch.nn.Parameter(tensors[n].clone().requires_grad_(True)))
        self.optimizer = make_optimizer([dict(params=[getattr(self, ATTRS[n])], lr=LRS[n], name=n) for n in NAMES])
        P = tensors["xyz"].shape[0]
        dev = tensors["xyz"].device
        self.xyz_gradient_accum, self.denom = torch.zeros(P, 1, device=dev), torch.zeros(P, 1, device=dev)
        self.max_radii2D = torch.zeros(P, device=dev)
        self.percent_dense, self.scaffold_points = percent_dense, F

    def params(self):
        return {n: getattr(self, ATTRS[n]) for n in NAMES}


OPTIMIZERS = {
    "hgs": (lambda groups: optim.Adam(groups, lr=0.0, eps=1e-15), lambda o, g: o.step_masked(g)),
    "torch": (lambda groups: torch.optim.Adam(groups, lr=0.0, eps=1e-15), lambda o, g: o.step()),
}


def _scene_model(gpu, P, make_optimizer, F, seed=3):
    cam = synth.make_camera(96, 64)
    sc = synth.make_scene(P, cam, seed=seed).to(gpu)
    op = sc.opacities.clamp(1e-4, 1 - 1e-4).reshape(P, 1)
    tensors = dict(xyz=sc.means3D, f_dc=sc.shs[:, :1].contiguous(), f_rest=sc.shs[:, 1:].contiguous(),
                   opacity=torch.log(op / (1 - op)), scaling=torch.log(sc.scales), rotation=sc.rotations)
    return Model({n: t.contiguous() for n, t in tensors.items()}, make_optimizer, F), cam


def _render_backward(model, cam, gpu):
    import diff_gaussian_rasterization as dgr
    P = model._xyz.shape[0]
    rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(cam, torch.zeros(3), 3, do_depth=True, device=gpu))
    means2D = torch.zeros(P, 3, device=gpu, requires_grad=True)
    color, radii, invd = dgr.GaussianRasterizer(rs)(
        means3D=model._xyz, means2D=means2D, shs=torch.cat((model._features_dc, model._features_rest), dim=1),
        opacities=torch.sigmoid(model._opacity), scales=torch.exp(model._scaling),
        rotations=torch.nn.functional.normalize(model._rotation))
    color.sum().backward()
    assert radii.shape[0] == P and bool(torch.isfinite(color).all())
    for n, p in model.params().items():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), n
    return radii, means2D


def _set_stats(model, seed, gpu):
    """Accumulator and radii of the size the training loop would leave, then every row cleared of the band."""
    P = model._xyz.shape[0]
    g = torch.Generator().manual_seed(seed)
    accum = torch.randn(P, 1, generator=g).abs() * 0.4
    accum[torch.rand(P, generator=g) < 0.04] = float("nan")
    model.xyz_gradient_accum = accum.to(gpu)
    model.max_radii2D = (torch.rand(P, generator=g) * 60.0).to(gpu)
    model.denom = torch.ones(P, 1, device=gpu)
    return g


@pytest.mark.parametrize("which", ["hgs", "torch", "stateless"])
def test_model_switch_over_with_real_optimizers(gpu, which):
    make, step = OPTIMIZERS["hgs" if which == "stateless" else which]
    model, cam = _scene_model(gpu, 3000, make, 100)
    if which != "stateless":
        for it in range(2):
            model.optimizer.zero_grad(set_to_none=True)
            _render_backward(model, cam, gpu)
            step(model.optimizer, model._opacity.grad)
    steps = {n: float(model.optimizer.state[p]["step"]) for n, p in model.params().items()} if which != "stateless" else {}
    g = _set_stats(model, 8, gpu)
    extent = float(torch.exp(model._scaling.detach()).max(dim=1).values.median()) / model.percent_dense
    max_grad, min_opacity = 4.0, 0.1
    share = dc.clear_band(model.params(), model.xyz_gradient_accum, model.max_radii2D, max_grad, min_opacity,
                          model.percent_dense * extent, g)
    assert share <= 0.01
    before = {n: p.detach().clone() for n, p in model.params().items()}
    state = model.optimizer.state
    moments = {n: (state[p]["exp_avg"].clone(), state[p]["exp_avg_sq"].clone()) if which != "stateless" else None
               for n, p in model.params().items()}
    ref_in = (before, moments, model.xyz_gradient_accum.clone(), model.max_radii2D.clone(), 100, max_grad, min_opacity,
              model.percent_dense * extent)
    S = int(classes(ref_in[2], ref_in[3], before["opacity"], before["scaling"], 100, max_grad, min_opacity, ref_in[7])[1].sum())
    noise = torch.randn((2 * S, 3), generator=torch.Generator().manual_seed(6)).to(gpu)
    ref = densify_and_prune_spec(*ref_in, noise=noise)
    old = model.params()
    totals = densify.densify_and_prune(model, max_grad, min_opacity, extent, noise=noise)
    assert totals == ref[2] and totals[1] > 0 and totals[3] > 0
    new = model.params()
    P_new = new["xyz"].shape[0]
    assert P_new == ref[0]["xyz"].shape[0] != 3000
    for i, n in enumerate(NAMES):
        group = model.optimizer.param_groups[i]
        assert group["name"] == n and group["params"][0] is new[n] and new[n] is not old[n]
        assert isinstance(new[n], torch.nn.Parameter) and new[n].requires_grad and new[n].shape[0] == P_new
        assert old[n] not in model.optimizer.state
        if which == "stateless":
            assert new[n] not in model.optimizer.state
        else:
            st = model.optimizer.state[new[n]]
            assert float(st["step"]) == steps[n] and st["exp_avg"].shape == new[n].shape == st["exp_avg_sq"].shape
    got_m = {n: (model.optimizer.state[p]["exp_avg"], model.optimizer.state[p]["exp_avg_sq"]) if which != "stateless"
             else None for n, p in new.items()}
    dc.assert_same_result(({n: p.detach() for n, p in new.items()}, got_m, totals), ref, which)
    assert tuple(model.xyz_gradient_accum.shape) == (P_new, 1) == tuple(model.denom.shape)
    assert tuple(model.max_radii2D.shape) == (P_new,)
    assert not model.xyz_gradient_accum.any() and not model.denom.any() and not model.max_radii2D.any()
    # an optimizer step and a rasterizer forward + backward at the new row count
    model.optimizer.zero_grad(set_to_none=True)
    _render_backward(model, cam, gpu)
    step(model.optimizer, model._opacity.grad)
    torch.cuda.synchronize()
    for n, p in new.items():
        st = model.optimizer.state[p]
        assert st["exp_avg"].shape == p.shape and bool(torch.isfinite(p.detach()).all()), n
        assert float(st["step"]) == steps.get(n, 0.0) + 1


def test_model_level_peak_stays_below_old_plus_new(gpu):
    """The groups are rebuilt and released one by one, the widest (f_rest) first: the peak above the model's own
    tensors is f_rest's three outputs -- 3 * 45 of the 3 * 59 floats of a new row at K = 15, 0.76 of all outputs -- plus
    the plan's 8 B per source row and the noise (about 0.01).  Bound: 0.9 of the bytes of all outputs (allocator
    rounding included); building everything before switching over would need 1.0 and more."""
    case = dc.make_inputs(200_000, 15, 12, gpu)
    model = Model(case["tensors"], OPTIMIZERS["hgs"][0], 0)
    for n, p in model.params().items():
        st = model.optimizer.state[p]
        st["step"], (st["exp_avg"], st["exp_avg_sq"]) = torch.tensor(3.0), case["moments"][n]
    model.xyz_gradient_accum, model.max_radii2D = case["accum"], case["radii"]
    extent = case["d"] / model.percent_dense
    del case, p, st
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    totals = densify.densify_and_prune(model, 4.0, 0.1, extent, generator=torch.Generator(device=gpu).manual_seed(0))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    rows = totals[0] + totals[1] + 2 * totals[3]
    everything = rows * 3 * 59 * 4
    print(f"peak above the model {peak} bytes = {peak / everything:.3f} of all outputs ({everything} bytes)")
    assert model._xyz.shape[0] == rows > 200_000
    assert peak <= 0.9 * everything, (peak, everything)


def test_install_binds_the_method(gpu):
    class M(Model):
        pass
    assert densify.install(M) is M
    model, _ = _scene_model(gpu, 500, OPTIMIZERS["hgs"][0], None)
    model.__class__ = M
    _set_stats(model, 2, gpu)
    totals = model.densify_and_prune(4.0, 0.005, 10.0, generator=torch.Generator(device=gpu).manual_seed(0))
    assert model._xyz.shape[0] == totals[0] + totals[1] + 2 * totals[3]


def test_three_rounds_of_steps_and_densification(gpu):
    """Each round: a few seeded hgs.optim.Adam.step_masked steps, then the fused call on the model and the spec on a
    copy of the very tensors it receives; the chain goes on from the fused result."""
    model, _ = _scene_model(gpu, 5000, OPTIMIZERS["hgs"][0], 200)
    g = torch.Generator().manual_seed(99)
    max_grad, min_opacity = 4.0, 0.1
    sizes = [model._xyz.shape[0]]
    for rnd in range(3):
        P = model._xyz.shape[0]
        for it in range(3):
            for n, p in model.params().items():
                p.grad = (torch.randn(p.shape, generator=g) * 0.01).to(gpu)
            model._opacity.grad[(torch.rand(P, generator=g) < 0.5).to(gpu)] = 0.0
            model.optimizer.step_masked(model._opacity.grad)
        _set_stats(model, 50 + rnd, gpu)
        extent = float(torch.exp(model._scaling.detach()).max(dim=1).values.median()) / model.percent_dense
        d = model.percent_dense * extent
        share = dc.clear_band(model.params(), model.xyz_gradient_accum, model.max_radii2D, max_grad, min_opacity, d, g)
        assert share <= 0.01, share
        state = model.optimizer.state
        ref_in = ({n: p.detach().clone() for n, p in model.params().items()},
                  {n: (state[p]["exp_avg"].clone(), state[p]["exp_avg_sq"].clone()) for n, p in model.params().items()},
                  model.xyz_gradient_accum.clone(), model.max_radii2D.clone(), model.scaffold_points, max_grad,
                  min_opacity, d)
        assert all(bool(m[0].any()) and bool(m[1].any()) for m in ref_in[1].values())       # moments are non-trivial
        S = int(classes(ref_in[2], ref_in[3], ref_in[0]["opacity"], ref_in[0]["scaling"], 200, max_grad, min_opacity, d)[1].sum())
        noise = torch.randn((2 * S, 3), generator=g).to(gpu)
        ref = densify_and_prune_spec(*ref_in, noise=noise)
        totals = densify.densify_and_prune(model, max_grad, min_opacity, extent, noise=noise)
        state = model.optimizer.state
        got = ({n: p.detach() for n, p in model.params().items()},
               {n: (state[p]["exp_avg"], state[p]["exp_avg_sq"]) for n, p in model.params().items()}, totals)
        print(f"round {rnd}: P {P} -> {model._xyz.shape[0]}, totals {totals}, re-drawn share {share:.1e}")
        dc.assert_same_result(got, ref, f"round {rnd}")
        sizes.append(model._xyz.shape[0])
    assert len(set(sizes)) == 4, sizes


def test_errors_leave_model_and_optimizer_untouched(gpu):
    model, cam = _scene_model(gpu, 800, OPTIMIZERS["hgs"][0], 10)
    model.optimizer.zero_grad(set_to_none=True)
    _render_backward(model, cam, gpu)
    model.optimizer.step_masked(model._opacity.grad)
    _set_stats(model, 1, gpu)

    def snapshot():
        ps = model.params()
        st = model.optimizer.state
        return ([(id(p), p.data_ptr(), id(st[p]["exp_avg"]), st[p]["exp_avg"].data_ptr(), st[p]["exp_avg_sq"].data_ptr())
                 for p in ps.values()],
                [id(g["params"][0]) for g in model.optimizer.param_groups], len(st),
                id(model.xyz_gradient_accum), id(model.denom), id(model.max_radii2D),
                [p.detach().clone() for p in ps.values()])
    before = snapshot()

    def unchanged():
        after = snapshot()
        assert after[:-1] == before[:-1]
        assert all(dc.same_bits(a, b) for a, b in zip(after[-1], before[-1]))
    bad_calls = [
        dict(max_grad=0.0), dict(max_grad=-1.0), dict(max_grad=float("nan")), dict(max_grad=float("inf")),
        dict(noise=torch.zeros(4, 3)),                                  # CPU noise
        dict(noise=torch.zeros(4, 2, device=gpu)),                      # bad shape, seen before the plan
        dict(noise=torch.zeros(2 * 799 + 2, 3, device=gpu)),            # wrong S, seen after the plan
        dict(noise=torch.zeros(4, 3, device=gpu, dtype=torch.float64)),
        dict(extent="far"),
    ]
    for change in bad_calls:
        args = dict(max_grad=4.0, min_opacity=0.1, extent=5.0)
        args.update(change)
        noise = args.pop("noise", None)
        with pytest.raises(ValueError):
            densify.densify_and_prune(model, args["max_grad"], args["min_opacity"], args["extent"], noise=noise)
        unchanged()
    for attr, value in (("xyz_gradient_accum", model.xyz_gradient_accum[:-1].clone()),
                        ("max_radii2D", model.max_radii2D.double()), ("scaffold_points", 801),
                        ("xyz_gradient_accum", model.xyz_gradient_accum.cpu())):
        keep = getattr(model, attr)
        setattr(model, attr, value)
        with pytest.raises(ValueError):
            densify.densify_and_prune(model, 4.0, 0.1, 5.0)
        setattr(model, attr, keep)
        unchanged()
    keep = model._rotation
    model._rotation = torch.nn.Parameter(keep.detach().clone())            # the group holds another object
    with pytest.raises(ValueError):
        densify.densify_and_prune(model, 4.0, 0.1, 5.0)
    model._rotation = keep
    unchanged()
    densify.densify_and_prune(model, 4.0, 0.1, 5.0)                         # and the good call still works
