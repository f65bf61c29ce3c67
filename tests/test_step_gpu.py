"""hgs.step on the GPU: the kernels against what the reference's own scripts did (tests/golden/ref_step_golden.npz);
bit identity with the composition torch lock zeroing -> hgs.optim.Adam.step(relevant) -> the spec's clamp
(tests/step_spec.py) in the single / post / coarse configurations over sizes, SH widths, visible shares and locks; the
statistics in both input forms; the dense fallback; skipped rows; determinism, streams and guard bytes; no torch-level
device-to-host wait; and thirty steps of a small scene with photometric_loss + post_backward + hgs.densify.

Inputs never hold a row within 1e-4 (relative) of the clamp threshold, before or after the step: rows near it are moved
away (tests/step_cases.py) and the reference composition's post-step values are asserted to be clear of the band."""
import ctypes as C

import pytest
import torch

import parity as pa
import step_cases as sc
import train_loop as tl
import ws_guard as wg
from step_spec import NAMES, clamp, locked_rows, post_backward_spec, relevant_rows, statistics, zero_locked
from hgs import _lib, densify, optim, step

pytestmark = pytest.mark.gpu

ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
             rotation="_rotation")


# ---- the reference's own scripts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.golden_case_names())
def test_kernels_reproduce_the_reference(gpu, name):
    c = sc.load_case(name, gpu)
    params = {n: torch.nn.Parameter(c["params"][n].clone()) for n in NAMES}
    opt = optim.Adam([dict(params=[params[n]], lr=c["lrs"][n], name=n) for n in NAMES], lr=0.0, eps=sc.EPS)
    for n in NAMES:
        params[n].grad = c["grads"][n].clone()
        if c["steps"][n] > 0:
            opt.state[params[n]] = dict(step=torch.tensor(c["steps"][n]), exp_avg=c["exp_avg"][n].clone(),
                                        exp_avg_sq=c["exp_avg_sq"][n].clone())
    stats = {}
    if c["single"]:
        stats = dict(radii=c["radii"], visible=c["visible"], means2D_grad=c["means2D_grad"], max_radii2D=c["max_radii2D"],
                     accum=c["accum"], denom=c["denom"])
    step.post_backward_tensors(params, opt, **stats, **c["config"])
    for n in NAMES:
        st = opt.state[params[n]]
        errs = (sc.rel_err(params[n].detach(), c["after"][n]), sc.rel_err(st["exp_avg"], c["after_exp_avg"][n]),
                sc.rel_err(st["exp_avg_sq"], c["after_exp_avg_sq"][n]))
        print(name, n, "rel err param / exp_avg / exp_avg_sq", errs)
        assert max(errs) <= sc.TOL, (name, n, errs)
        assert params[n].grad is None and float(st["step"]) == c["steps"][n] + 1
    assert torch.equal(c["max_radii2D"], c["after_max_radii2D"])
    if c["single"]:
        assert torch.equal(c["denom"], c["after_denom"])
        a, b = c["accum"], c["after_accum"]
        assert bool(((a - b).abs() <= sc.ACCUM_TOL * b.abs()).all())
        c64 = sc.load_case(name, dtype=torch.float64)                    # the clamped rows, from the float64 statement
        cfg = dict(c64["config"])
        big = post_backward_spec(c64["params"], c64["grads"], state={n: [c64["exp_avg"][n], c64["exp_avg_sq"][n], c64["steps"][n]] for n in NAMES},
                                 lrs=c64["lrs"], eps=sc.EPS, clamp_args=cfg.pop("clamp"), **cfg)["clamped"].to(gpu)
        assert big.any()
        ok, worst = sc.child_bound_ok(params["scaling"].detach()[big], c["after"]["scaling"][big])
        assert ok, (name, worst)


# ---- bit identity with the composition ------------------------------------------------------------------------------
def _config(kind, P, L, gpu, seed):
    """-> (fused keyword arguments, clamp_args) of the three scripts' configurations with L locked rows."""
    if kind == "single":                     # train_single.py: head lock of all six, opacity selection, clamp
        return dict(lock_head=L, select="opacity_grad"), (None, 0)
    if kind == "post":                       # train_post.py: tail lock + anchors, every row, no clamp
        mask = torch.rand(P, generator=torch.Generator(device=gpu).manual_seed(seed), device=gpu) < 0.05
        return dict(lock_tail=L, lock_mask=mask, select="all"), None
    return dict(lock_head=L, lock_names=("scaling",), select="opacity_grad"), (None, L)   # train_coarse.py


def _compose(model, kw, clamp_args, moments_seed):
    """The composition on code that exists without hgs.step: torch lock zeroing, hgs.optim.Adam.step(relevant) or
    .step(), the spec's clamp.  -> (state, clamped mask or None, post-step band distance)."""
    params, opt = sc.build(model, moments_seed)
    P = model["P"]
    dev = params["xyz"].device
    grads = {n: params[n].grad for n in NAMES}
    if model["K"] == 0:
        params["f_rest"].grad = None         # hgs.optim.Adam refuses a tensor of zero width; hgs.step skips it
    zero_locked(grads, locked_rows(P, kw.get("lock_head", 0), kw.get("lock_tail", 0), kw.get("lock_mask"), dev),
                kw.get("lock_names", NAMES))
    if kw["select"] == "all":
        opt.step()
    else:
        opt.step(relevant_rows(grads["opacity"]))
    mask, dist = None, float("inf")
    if clamp_args is not None:
        dist = sc.band_distance(params["scaling"].detach(), clamp_args[0])
        mask = clamp(params["scaling"].data, *clamp_args)
    return sc.state_of(params, opt), mask, dist


def _fused(model, kw, clamp_args, moments_seed, **more):
    params, opt = sc.build(model, moments_seed)
    step.post_backward_tensors(params, opt, clamp=clamp_args, **kw, **more)
    assert all(params[n].grad is None for n in NAMES)
    return sc.state_of(params, opt)


def _assert_identical(got, ref, mask, where):
    for n in NAMES:
        if not got[n][0].numel():
            continue
        for k, what in ((1, "exp_avg"), (2, "exp_avg_sq")):
            assert sc.same_bits(got[n][k], ref[n][k]), (where, n, what)
        if n == "scaling" and mask is not None:
            assert sc.same_bits(got[n][0][~mask], ref[n][0][~mask]), (where, n, "unclamped rows")
            ok, worst = sc.child_bound_ok(got[n][0][mask], ref[n][0][mask])
            assert ok, (where, "clamped rows", worst)
        else:
            assert sc.same_bits(got[n][0], ref[n][0]), (where, n)


def _one(gpu, kind, P, K, vis, lock, seed):
    L = {"0": 0, "half": P // 2, "P": P}[lock]
    model = sc.make_model(P, K, seed, gpu, visible_fraction=vis)
    kw, clamp_args = _config(kind, P, L, gpu, seed)
    if clamp_args is not None:
        thr = float(torch.exp(model["params"]["scaling"]).max(dim=1).values.median()) * 1.001
        sc.clear_band(model["params"]["scaling"], thr)
        clamp_args = (thr, clamp_args[1])
    ref, mask, dist = _compose(model, kw, clamp_args, seed + 1)
    assert dist >= sc.BAND, (kind, P, K, vis, lock, dist)
    got = _fused(model, kw, clamp_args, seed + 1)
    _assert_identical(got, ref, mask, (kind, P, K, vis, lock))
    return mask


SMALL = [1, 63, 64, 65, 1_000]
LARGE = [375_000, 1_000_000]
# at the large sizes every K, visible share and lock appears once per configuration (a Latin triple), not the product
TRIPLES = [(0, 0.0, "0"), (3, 0.3, "half"), (15, 1.0, "P"), (15, 0.3, "0")]


@pytest.mark.parametrize("kind", ["single", "post", "coarse"])
@pytest.mark.parametrize("P", SMALL)
def test_bit_identical_to_the_composition_small(gpu, kind, P):
    seen = 0
    for K in (0, 3, 15):
        for vis in (0.0, 0.3, 1.0):
            for lock in ("0", "half", "P"):
                mask = _one(gpu, kind, P, K, vis, lock, 1000 * P + 10 * K + int(10 * vis))
                seen += 0 if mask is None else int(mask.sum())
    if kind != "post" and P >= 63:
        assert seen > 0                          # the clamp acted somewhere


@pytest.mark.parametrize("kind", ["single", "post", "coarse"])
@pytest.mark.parametrize("P", LARGE)
def test_bit_identical_to_the_composition_large(gpu, kind, P):
    for K, vis, lock in TRIPLES:
        mask = _one(gpu, kind, P, K, vis, lock, P + K)
        if mask is not None and lock != "P":
            assert 0.3 * P < int(mask.sum()) * (2 if lock == "half" and kind == "coarse" else 1) < 0.7 * P


# ---- statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 65, 1_000, 375_000])
def test_statistics_in_both_forms(gpu, P):
    model = sc.make_model(P, 0, 7 + P, gpu, visible_fraction=0.3 if P > 1 else 1.0)
    model["accum"][::7] = float("nan")
    model["means2D_grad"][3::11] = float("nan")
    ref = {k: model[k].clone() for k in ("max_radii2D", "accum", "denom")}
    statistics(ref["max_radii2D"], ref["accum"], ref["denom"], model["means2D_grad"], model["radii"])
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(P)).to(gpu)
    forms = {
        "raw": dict(radii=model["radii"]),
        "raw with indices": dict(radii=model["radii"][perm].contiguous(), indices=perm.int()),
        "compacted": dict(radii=model["radii"][model["visible"]].contiguous(), visible=model["visible"]),
    }
    for what, form in forms.items():
        got = {k: model[k].clone() for k in ("max_radii2D", "accum", "denom")}
        params, opt = sc.build(model)
        step.post_backward_tensors(params, opt, means2D_grad=model["means2D_grad"], optimize=False, **form, **got)
        assert all(params[n].grad is not None for n in NAMES)              # optimize=False leaves the gradients
        assert torch.equal(got["max_radii2D"], ref["max_radii2D"]), what
        assert torch.equal(got["denom"], ref["denom"]), what
        a, b = got["accum"], ref["accum"]
        assert torch.equal(a.isnan(), b.isnan()), what                     # NaN propagates as in torch.maximum
        fin = ~b.isnan()
        assert bool(((a[fin] - b[fin]).abs() <= sc.ACCUM_TOL * b[fin].abs()).all()), what
        if what != "raw":
            assert sc.same_bits(got["accum"].nan_to_num(7.0), first.nan_to_num(7.0)), what   # the forms agree bit for bit
        first = got["accum"]
    # max_radii2D alone (no accumulator)
    got = model["max_radii2D"].clone()
    params, opt = sc.build(model)
    step.post_backward_tensors(params, opt, radii=model["radii"], max_radii2D=got, optimize=False)
    assert torch.equal(got, ref["max_radii2D"])


# ---- fallback, locks, skipped rows -----------------------------------------------------------------------------------
def test_dense_fallback_when_no_opacity_gradient_is_set(gpu):
    model = sc.make_model(10_007, 3, 5, gpu, visible_fraction=1.0)
    model["grads"]["opacity"].zero_()
    params, opt = sc.build(model, 6)
    opt.step(torch.empty(0))
    ref = sc.state_of(params, opt)
    got = _fused(model, dict(select="opacity_grad"), None, 6)
    _assert_identical(got, ref, None, "dense fallback")
    assert not sc.same_bits(got["xyz"][0], model["params"]["xyz"])
    # the same when the lock is what empties the selection
    model = sc.make_model(10_007, 3, 5, gpu, visible_fraction=1.0)
    ref, _, _ = _compose(model, dict(lock_head=10_007, select="opacity_grad"), None, 6)
    got = _fused(model, dict(lock_head=10_007, select="opacity_grad"), None, 6)
    _assert_identical(got, ref, None, "everything locked")


def test_coarse_lock_decays_the_moments_of_a_selected_locked_row(gpu):
    P, L = 4_099, 1_000
    model = sc.make_model(P, 3, 8, gpu, visible_fraction=1.0)
    got = _fused(model, dict(lock_head=L, lock_names=("scaling",), select="opacity_grad"), None, 9)
    params, opt = sc.build(model, 9)
    before = sc.state_of(params, opt)
    m0, v0 = before["scaling"][1][:L], before["scaling"][2][:L]
    assert sc.same_bits(got["scaling"][1][:L], m0 * 0.9) and sc.same_bits(got["scaling"][2][:L], v0 * 0.999)
    assert not sc.same_bits(got["scaling"][0][:L], before["scaling"][0][:L])          # moved by the decayed moment
    assert not sc.same_bits(got["xyz"][1][:L], before["xyz"][1][:L] * 0.9)            # xyz is not locked: real gradient


def test_skipped_rows_are_unchanged_bit_for_bit(gpu):
    P, L = 20_011, 5_000
    model = sc.make_model(P, 3, 10, gpu, visible_fraction=0.3)
    thr = float(torch.exp(model["params"]["scaling"]).max(dim=1).values.median()) * 1.001
    sc.clear_band(model["params"]["scaling"], thr)
    params, opt = sc.build(model, 11)
    before = sc.state_of(params, opt)
    got = _fused(model, dict(lock_head=0, select="opacity_grad"), (thr, L), 11)
    unsel = (model["grads"]["opacity"].flatten() == 0)
    assert 0.5 * P < int(unsel.sum()) < 0.9 * P
    for n in NAMES:
        for k in range(3):
            rows = unsel if not (n == "scaling" and k == 0) else unsel & (torch.arange(P, device=gpu) < L)
            assert sc.same_bits(got[n][k][rows], before[n][k][rows]), (n, k)          # unselected (and protected) rows
    big = torch.exp(got["scaling"][0][:L]).max(dim=1).values > thr
    assert big.any()                                                                  # protected rows above the threshold stay
    # locked rows under select="all" with zero moments: gradient 0, moments 0 -> nothing moves
    params, opt = sc.build(model)
    for n in NAMES:
        opt.state[params[n]] = dict(step=torch.tensor(2.), exp_avg=torch.zeros_like(params[n]), exp_avg_sq=torch.zeros_like(params[n]))
    step.post_backward_tensors(params, opt, select="all", lock_tail=L)
    for n in NAMES:
        st = opt.state[params[n]]
        assert sc.same_bits(params[n].detach()[P - L:], model["params"][n][P - L:]), n
        assert not st["exp_avg"][P - L:].any() and not st["exp_avg_sq"][P - L:].any(), n
    assert not sc.same_bits(params["xyz"].detach()[:P - L], model["params"]["xyz"][:P - L])


def test_clamp_runs_without_gradients(gpu):
    """A densification iteration leaves no gradients: part 2 is skipped without error, the clamp still runs."""
    P = 3_001
    model = sc.make_model(P, 3, 12, gpu)
    thr = float(torch.exp(model["params"]["scaling"]).max(dim=1).values.median()) * 1.001
    sc.clear_band(model["params"]["scaling"], thr)
    params, opt = sc.build(model, 13)
    for n in NAMES:
        params[n].grad = None
    before = sc.state_of(params, opt)
    step.post_backward_tensors(params, opt, clamp=(thr, 100))
    after = sc.state_of(params, opt)
    ref = before["scaling"][0].clone()
    mask = clamp(ref, thr, 100)
    assert 0.3 * P < int(mask.sum()) < 0.7 * P
    assert sc.same_bits(after["scaling"][0][~mask], ref[~mask]) and sc.child_bound_ok(after["scaling"][0][mask], ref[mask])[0]
    for n in NAMES:
        assert float(opt.state[params[n]]["step"]) == 2.0
        for k in (1, 2):
            assert sc.same_bits(after[n][k], before[n][k])
        if n != "scaling":
            assert sc.same_bits(after[n][0], before[n][0])


# ---- determinism and buffers -----------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical_and_streams_agree(gpu):
    P = 100_003
    model = sc.make_model(P, 15, 21, gpu)
    thr = float(torch.exp(model["params"]["scaling"]).max(dim=1).values.median()) * 1.001
    sc.clear_band(model["params"]["scaling"], thr)

    def run():
        stats = {k: model[k].clone() for k in ("max_radii2D", "accum", "denom")}
        st = _fused(model, dict(lock_head=1234, select="opacity_grad"), (thr, 77), 22, radii=model["radii"],
                    means2D_grad=model["means2D_grad"], **stats)
        return st, stats
    a, b = run(), run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        c = run()
    side.synchronize()
    for x in (b, c):
        for n in NAMES:
            for k in range(3):
                assert sc.same_bits(a[0][n][k], x[0][n][k]), (n, k)
        for k in a[1]:
            assert sc.same_bits(a[1][k], x[1][k]), k


@pytest.mark.parametrize("P", [1, 65, 257, 1003])
def test_c_abi_between_guard_bytes(gpu, P):
    """Select and apply called directly; EVERY buffer they are handed lies between two guards, the workspace filled once
    with 0x00 and once with 0xFF: intact guards, bitwise equal results, the Python path's values."""
    lib = _lib.lib()
    K = 3
    model = sc.make_model(P, K, 300 + P, gpu, visible_fraction=0.5 if P > 1 else 1.0)
    thr = float(torch.exp(model["params"]["scaling"]).max(dim=1).values.median()) * 1.001
    sc.clear_band(model["params"]["scaling"], thr)
    L = P // 3
    mask = (torch.arange(P, device=gpu) % 5 == 0)
    stats0 = {k: model[k].clone() for k in ("max_radii2D", "accum", "denom")}
    ref_stats = {k: v.clone() for k, v in stats0.items()}
    ref = _fused(model, dict(lock_head=L, lock_mask=mask, select="opacity_grad"), (thr, L // 2), 301 + P,
                 radii=model["radii"], means2D_grad=model["means2D_grad"], **ref_stats)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = []
    for fill in (0x00, 0xFF):
        gs = []

        def put(name, t):
            t = t.contiguous()
            g = wg.guarded(t.numel() * t.element_size(), gpu, 0x00, name)
            gs.append(g)
            g.body.copy_(t.reshape(-1).view(torch.uint8))
            return g
        params, opt = sc.build(model, 301 + P)
        tmp = wg.guarded(lib.hgs_step_tmp_bytes(P), gpu, fill, "tmp")
        gs.append(tmp)
        bufs, descs = {}, []
        for n in NAMES:
            p = params[n]
            st = opt.state[p]
            bufs[n] = [put(f"{n}.{w}", t) for w, t in (("param", p.detach()), ("grad", p.grad), ("exp_avg", st["exp_avg"]),
                                                     ("exp_avg_sq", st["exp_avg_sq"]))]
            step_no = 3.0
            bc1, bc2 = 1 - 0.9 ** step_no, 1 - 0.999 ** step_no
            ad = _lib.AdamTensor(param=bufs[n][0].addr, grad=bufs[n][1].addr, exp_avg=bufs[n][2].addr,
                                 exp_avg_sq=bufs[n][3].addr, row_len=p[0].numel(), step_size=sc.LRS[n] / bc1, beta1=0.9,
                                 one_minus_beta1=1 - 0.9, beta2=0.999, one_minus_beta2=1 - 0.999, eps=sc.EPS,
                                 weight_decay=0.0, bias_correction2_sqrt=bc2 ** 0.5)
            descs.append(_lib.StepTensor(adam=ad, flags=_lib.STEP_LOCKABLE | (_lib.STEP_SCALING if n == "scaling" else 0)))
        io = {k: put(k, v) for k, v in stats0.items()}
        radii, m2g, lm = put("radii", model["radii"]), put("means2D_grad", model["means2D_grad"]), put("lock_mask", mask.view(torch.uint8))
        a = _lib.StepArgs(P=P, n=P, radii=radii.addr, means2D_grad=m2g.addr, max_radii2D=io["max_radii2D"].addr,
                          accum=io["accum"].addr, denom=io["denom"].addr, opacity_grad=bufs["opacity"][1].addr,
                          lock_mask=lm.addr, lock_head=L, lock_tail=0, protect_head=L // 2, select_all=0, lock_opacity=1,
                          clamp=1, clamp_threshold=thr)
        _lib.check(lib.hgs_step_select(C.byref(a), C.c_void_p(tmp.addr), stream, 0), "hgs_step_select")
        arr = (_lib.StepTensor * len(descs))(*descs)
        _lib.check(lib.hgs_step_apply(C.byref(a), arr, len(descs), C.c_void_p(tmp.addr), stream, 0), "hgs_step_apply")
        wg.check(*gs)
        out = {n: [b.view(torch.float32).clone() for b in bufs[n]] for n in NAMES}
        out_stats = {k: io[k].view(torch.float32).clone() for k in io}
        for n in NAMES:
            for k, j in ((0, 0), (1, 2), (2, 3)):
                assert sc.same_bits(out[n][j], ref[n][k].reshape(-1)), (P, fill, n, k)
            assert sc.same_bits(out[n][1], model["grads"][n].reshape(-1)), (n, "the gradient is read only")
        for k in io:
            assert sc.same_bits(out_stats[k].nan_to_num(7.0), ref_stats[k].reshape(-1).nan_to_num(7.0)), (P, fill, k)
        results.append(out)
    for n in NAMES:
        for j in range(4):
            assert sc.same_bits(results[0][n][j], results[1][n][j]), (n, j)


# ---- no torch-level device-to-host wait --------------------------------------------------------------------------------
def test_no_sync_at_torch_level_and_the_statement_has_some(gpu):
    P = 50_000
    model = sc.make_model(P, 3, 40, gpu)
    thr = float(torch.exp(model["params"]["scaling"]).max(dim=1).values.median()) * 1.001
    sc.clear_band(model["params"]["scaling"], thr)
    lock_mask = step.row_mask(P, torch.arange(0, P, 9, device=gpu))
    params, opt = sc.build(model, 41)
    stats = {k: model[k].clone() for k in ("max_radii2D", "accum", "denom")}
    sparams, sopt = sc.build(model, 41)
    sgrads = {n: sparams[n].grad for n in NAMES}
    sstats = {k: model[k].clone() for k in ("max_radii2D", "accum", "denom")}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step.post_backward_tensors(params, opt, radii=model["radii"], means2D_grad=model["means2D_grad"], lock_head=100,
                                   lock_mask=lock_mask, clamp=(thr, 50), **stats)
        with pytest.raises(RuntimeError, match="synchroniz"):              # the check bites: the statement waits
            post_backward_spec({n: p.data for n, p in sparams.items()}, sgrads, optimizer=sopt, radii=model["radii"],
                               means2D_grad=model["means2D_grad"], lock_head=100, lock_mask=lock_mask,
                               clamp_args=(thr, 50), **sstats)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(p.grad is None for p in params.values())


# ---- model level -----------------------------------------------------------------------------------------------------
class Model:
    """The reference's GaussianModel as far as post_backward and densify_and_prune see it (duck typed)."""

    def __init__(self, raw, lrs):
        for n in NAMES:
            setattr(self, ATTRS[n], torch.nn.Parameter(raw[n].detach().clone()))
        self.optimizer = optim.Adam([dict(params=[getattr(self, ATTRS[n])], lr=lrs[n], name=n) for n in NAMES], lr=0.0, eps=1e-15)
        P, dev = raw["xyz"].shape[0], raw["xyz"].device
        self.xyz_gradient_accum, self.denom = torch.zeros(P, 1, device=dev), torch.zeros(P, 1, device=dev)
        self.max_radii2D = torch.zeros(P, device=dev)
        self.percent_dense, self.scaffold_points = 0.01, 0

    def params(self):
        return {n: getattr(self, ATTRS[n]) for n in NAMES}


def _render(model, cam, bg, gpu):
    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(cam, bg, 3, do_depth=True, device=gpu))
    a = tl.activate(model.params())
    m2 = torch.zeros(a["means3D"].shape[0], 3, device=gpu, requires_grad=True)
    color, radii, invd = dgr.GaussianRasterizer(raster_settings=rs)(
        means3D=a["means3D"], means2D=m2, shs=a["shs"], colors_precomp=None, opacities=a["opacities"], scales=a["scales"],
        rotations=a["rotations"], cov3D_precomp=None)
    return color, radii, invd, m2


def _train(gpu, fused, cams, targets, raw, steps, thr, extent, first, max_grad=None):
    from hgs.loss import photometric_loss
    model = Model(raw, tl.LRS)
    bg = torch.zeros(3)
    for it in range(steps):
        k = it % len(cams)
        color, radii, invd, m2 = _render(model, cams[k], bg, gpu)
        tc, td = targets[k]
        res = photometric_loss(color, tc, lambda_dssim=0.2, clamp=False, invdepth=invd, mono_invdepth=td,
                               depth_mask=torch.ones_like(td), depth_weight=0.1)
        res.loss.backward()
        if fused:
            step.post_backward(model, radii=radii, viewspace_points=m2, lock_head=20, clamp=(thr, 10))
        else:
            p = model.params()
            out = post_backward_spec({n: t.data for n, t in p.items()}, {n: t.grad for n, t in p.items()},
                                     optimizer=model.optimizer, radii=radii, means2D_grad=m2.grad,
                                     max_radii2D=model.max_radii2D, accum=model.xyz_gradient_accum, denom=model.denom,
                                     lock_head=20, clamp_args=(thr, 10))
        if it == 0:
            first.append((sc.state_of(model.params(), model.optimizer), model.max_radii2D.clone(), model.denom.clone(),
                          model.xyz_gradient_accum.clone(), None if fused else out["clamped"]))
        if it == steps // 2:
            if max_grad is None:             # a threshold that a fifth of the rows pass, from the statement's own run
                w = model.max_radii2D * torch.sigmoid(model._opacity.detach()).flatten() ** 0.2
                max_grad = float((model.xyz_gradient_accum.flatten() * w).quantile(0.8))
            densify.densify_and_prune(model, max_grad, 0.005, extent, generator=torch.Generator(device=gpu).manual_seed(3))
    with torch.no_grad():
        vals = [tl.psnr(_render(model, c, bg, gpu)[0].clamp(0, 1).cpu(), t[0].clamp(0, 1).cpu()) for c, t in zip(cams, targets)]
    return sum(vals) / len(vals), model._xyz.shape[0], max_grad


def test_thirty_steps_with_the_fused_step_match_the_statement(gpu):
    cams, scene = tl.make_problem(P=4000, size=256, height=160, n_views=6, seed=1)
    bg = torch.zeros(3)
    gt = Model(tl.raw_params_from_scene(scene, gpu), tl.LRS)
    with torch.no_grad():
        targets = []
        for c in cams:
            color, _, invd, _ = _render(gt, c, bg, gpu)
            targets.append((color.detach(), invd.detach()))
    raw = tl.raw_params_from_scene(scene, gpu, jitter_seed=5)
    thr = float(torch.exp(raw["scaling"].detach()).max(dim=1).values.quantile(0.9))
    sc.clear_band(raw["scaling"].data, thr)
    extent = 4.0
    fa, fb = [], []
    p_s, rows_s, max_grad = _train(gpu, False, cams, targets, raw, 30, thr, extent, fa)
    p_f, rows_f, _ = _train(gpu, True, cams, targets, raw, 30, thr, extent, fb, max_grad)
    print(f"PSNR {p_s:.4f} (statement) / {p_f:.4f} (fused) dB; rows {rows_s} / {rows_f}; max_grad {max_grad:.3g}")
    (sa, ra, da, aa, mask), (sb, rb, db, ab, _) = fa[0], fb[0]
    before_clamp = torch.where(mask[:, None], sa["scaling"][0] - torch.log(torch.tensor(0.8)), sa["scaling"][0])
    assert mask.any() and sc.band_distance(before_clamp, thr) >= sc.BAND
    _assert_identical(sb, sa, mask, "first step")
    assert torch.equal(ra, rb) and torch.equal(da, db)
    assert bool(((aa - ab).abs() <= sc.ACCUM_TOL * aa.abs()).all())
    assert rows_s > 4000 and rows_f > 4000
    assert abs(p_f - p_s) <= 0.01


def test_peak_memory_above_the_model_is_the_workspace(gpu):
    P = 200_000
    model = sc.make_model(P, 15, 50, gpu)
    m = Model(model["params"], sc.LRS)
    for n, p in m.params().items():
        m.optimizer.state[p] = dict(step=torch.tensor(2.), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.ones_like(p) * 1e-4)
        p.grad = model["grads"][n]
    m2 = model["means2D_grad"]
    radii = model["radii"]
    tmp_bytes = _lib.lib().hgs_step_tmp_bytes(P)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step.post_backward(m, radii=radii, means2D_grad=m2, lock_head=100, clamp=(0.05, 10))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak above the model {peak} bytes; workspace {tmp_bytes} bytes")
    assert peak <= tmp_bytes + (1 << 20), (peak, tmp_bytes)
    assert all(p.grad is None for p in m.params().values())


def test_install_binds_the_method(gpu):
    class M(Model):
        pass
    assert step.install(M) is M
    model = sc.make_model(500, 3, 60, gpu)
    m = M(model["params"], sc.LRS)
    for n, p in m.params().items():
        p.grad = model["grads"][n].clone()
    m.post_backward(radii=model["radii"][model["visible"]].contiguous(), visible=model["visible"],
                    means2D_grad=model["means2D_grad"], select="all", lock_tail=5)
    assert all(p.grad is None for p in m.params().values()) and bool(m.denom.any())
