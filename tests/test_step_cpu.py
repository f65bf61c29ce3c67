"""hgs.step without a GPU: the torch statement of the rule (tests/step_spec.py) in float64 against what the reference's
own train_single.py and train_post.py did between ``loss.backward()`` and the next iteration
(tests/golden/ref_step_golden.npz), argument validation before the library is touched, the host-only size query, the
C ABI's checks, and the kernels' resources as the compiler reports them for gfx950."""
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

import step_cases as sc
from step_spec import NAMES, post_backward_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_holds_numbers_only_and_covers_the_rule():
    z = np.load(sc.GOLDEN)                              # allow_pickle=False: numeric and string arrays only
    assert os.path.getsize(sc.GOLDEN) <= 1_000_000
    names = sc.golden_case_names()
    assert any(n.startswith("single") for n in names) and any(n.startswith("post") for n in names)
    for name in names:
        c = sc.load_case(name)
        P = c["P"]
        assert 0 < c["visible"].numel() < P, name                        # visible and invisible rows
        cfg = c["config"]
        locked = torch.zeros(P, dtype=torch.bool)
        locked[:cfg.get("lock_head", 0)] = True
        locked[P - cfg.get("lock_tail", 0):] = True
        if cfg.get("lock_mask") is not None:
            locked |= cfg["lock_mask"].bool()
        assert locked.any() and not locked.all(), name
        assert any(bool(c["grads"][n][locked].any()) for n in NAMES), name   # locked rows with non-zero raw gradients
        if c["single"]:
            thr = cfg["clamp"][0]
            assert min(sc.band_distance(c["params"]["scaling"], thr), sc.band_distance(c["after"]["scaling"], thr)) >= sc.BAND
            big = torch.exp(c["params"]["scaling"].double()).max(dim=1).values > thr
            assert big.any() and not big.all(), name                      # clamped and unclamped rows


@pytest.mark.parametrize("name", sc.golden_case_names())
def test_float64_spec_reproduces_the_reference(name):
    c = sc.load_case(name, dtype=torch.float64)
    ref = sc.load_case(name)
    state = {n: [c["exp_avg"][n], c["exp_avg_sq"][n], c["steps"][n]] for n in NAMES}
    stats = {}
    if c["single"]:
        stats = dict(radii=c["radii"], visible=c["visible"], means2D_grad=c["means2D_grad"], max_radii2D=c["max_radii2D"],
                     accum=c["accum"], denom=c["denom"])
    cfg = dict(c["config"])
    out = post_backward_spec(c["params"], c["grads"], state=state, lrs=c["lrs"], eps=sc.EPS, clamp_args=cfg.pop("clamp"),
                             **stats, **cfg)
    for n in NAMES:
        errs = (sc.rel_err(c["params"][n], ref["after"][n]), sc.rel_err(state[n][0], ref["after_exp_avg"][n]),
                sc.rel_err(state[n][1], ref["after_exp_avg_sq"][n]))
        print(name, n, "rel err param / exp_avg / exp_avg_sq", errs)
        assert max(errs) <= sc.TOL, (name, n, errs)
    assert torch.equal(c["max_radii2D"].float(), ref["after_max_radii2D"]), name
    if c["single"]:
        assert torch.equal(c["denom"].float(), ref["after_denom"]), name
        a, b = c["accum"], ref["after_accum"].double()
        assert bool(((a - b).abs() <= sc.ACCUM_TOL * b.abs()).all()), (name, float(((a - b).abs() / b.abs().clamp_min(1e-300)).max()))
        assert out["clamped"].any() and not out["clamped"].all()
        assert 0 < out["relevant"].numel() < c["P"]
    # form (a) of the statistics gives what form (b) gives
    if c["single"]:
        d = sc.load_case(name, dtype=torch.float64)
        from step_spec import statistics
        statistics(d["max_radii2D"], d["accum"], d["denom"], d["means2D_grad"], sc.raw_radii(d["P"], d["visible"], d["radii"]))
        assert torch.equal(d["max_radii2D"], c["max_radii2D"]) and torch.equal(d["accum"], c["accum"]) and torch.equal(d["denom"], c["denom"])


class FakeCuda(torch.Tensor):                       # passes the device test; everything else is checked for real
    is_cuda = True


def fake(t):
    return t.as_subclass(FakeCuda)


def _good():
    from hgs.optim import Adam
    c = sc.load_case("single_1")
    params = {n: fake(c["params"][n]) for n in NAMES}
    for n in NAMES:
        params[n].grad = fake(c["grads"][n])
    opt = Adam([dict(params=[params[n]], lr=c["lrs"][n], name=n) for n in NAMES], lr=0.0, eps=sc.EPS)
    args = dict(radii=fake(c["radii"]), visible=fake(c["visible"]), means2D_grad=fake(c["means2D_grad"]),
                max_radii2D=fake(c["max_radii2D"]), accum=fake(c["accum"]), denom=fake(c["denom"]), **c["config"])
    return c, params, opt, args


def test_validation_raises_before_the_library_is_touched_and_changes_nothing(monkeypatch):
    from hgs import _lib, step

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    c, params, opt, good = _good()
    P = c["P"]
    before = {n: (params[n].clone(), params[n].grad.clone()) for n in NAMES}
    stats_before = {k: good[k].clone() for k in ("max_radii2D", "accum", "denom")}

    def unchanged():
        for n in NAMES:
            assert torch.equal(params[n], before[n][0]) and params[n].grad is not None and torch.equal(params[n].grad, before[n][1])
            assert len(opt.state[params[n]]) == 0                       # not even a step count
        for k, v in stats_before.items():
            assert torch.equal(good[k], v)

    def expect(match, params_=None, opt_=None, **change):
        args = dict(good)
        args.update(change)
        with pytest.raises(ValueError, match=match):
            step.post_backward_tensors(params_ or params, opt_ or opt, **args)
        unchanged()

    with pytest.raises(AssertionError, match="touched"):                # the good arguments reach the library
        step.post_backward_tensors(params, opt, **good)
    unchanged()
    plain = {n: c["params"][n].clone() for n in NAMES}
    expect("GPU tensor", params_=plain)                                 # CPU tensors: no fallback
    expect("dict with the keys", params_={"xyz": params["xyz"]})
    expect("float32", params_=dict(params, rotation=fake(c["params"]["rotation"].double())))
    expect("not contiguous", params_=dict(params, rotation=fake(c["params"]["rotation"].t().contiguous().t())))
    expect("rows expected", params_=dict(params, f_dc=fake(c["params"]["f_dc"][:-1].clone())))
    expect("floats per row", params_=dict(params, rotation=fake(torch.zeros(P, 3))))
    expect("not a parameter of the optimizer", params_=dict(params, rotation=fake(torch.zeros(P, 4))))
    expect("hgs.optim.Adam", opt_=torch.optim.Adam([torch.zeros(3, requires_grad=True)]))
    expect("torch.int32", radii=fake(c["radii"].long()))
    expect("torch.int32", radii=fake(c["radii"].float()))
    expect("rows expected", radii=fake(c["radii"][:-1].clone()))
    expect("torch.int64", visible=fake(c["visible"].int()))
    expect("expected without indices", visible=None)                               # compacted radii without their rows
    expect("not both forms", indices=fake(c["visible"].int()))
    expect("statistics need radii", radii=None)                         # neither form
    expect("torch.int32", visible=None, radii=fake(sc.raw_radii(P, c["visible"], c["radii"])), indices=fake(torch.arange(P)))
    expect("rows expected", visible=None, radii=fake(sc.raw_radii(P, c["visible"], c["radii"])),
           indices=fake(torch.arange(P - 1, dtype=torch.int32)))
    expect("statistics need max_radii2D", max_radii2D=None)
    expect("come together", denom=None)
    expect("accum needs means2D_grad", means2D_grad=None)
    expect(r"\(%d,3\) expected" % P, means2D_grad=fake(torch.zeros(P, 2)))
    expect("one value per row", accum=fake(torch.zeros(P, 2)))
    expect("torch.bool or torch.uint8", lock_mask=fake(torch.zeros(P, dtype=torch.int32)))
    expect("rows expected", lock_mask=fake(torch.zeros(P + 1, dtype=torch.bool)))
    expect("must be an integer", lock_head=P + 1)
    expect("must be an integer", lock_tail=-1)
    expect("exceed", lock_head=P - 1, lock_tail=2)
    expect("unknown names", lock_names=("scale",))
    expect("select must be", select="none")
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-50):
        expect("threshold", clamp=(bad, 0))
    expect("must be an integer", clamp=(1.0, P + 1))
    expect("threshold, protect_head", clamp=1.0)
    params["xyz"].grad = None
    try:
        with pytest.raises(ValueError, match="some have none"):
            step.post_backward_tensors(params, opt, **good)
    finally:
        params["xyz"].grad = fake(before["xyz"][1].clone())


def test_row_mask_and_install():
    from hgs import step
    m = step.row_mask(10, torch.tensor([1, 7, 7]))
    assert m.dtype == torch.uint8 and m.tolist() == [0, 1, 0, 0, 0, 0, 0, 1, 0, 0]
    assert step.row_mask(4, torch.empty(0, dtype=torch.int64)).tolist() == [0, 0, 0, 0]

    class Model:
        pass
    assert step.install(Model) is Model and callable(Model.post_backward)


def test_tmp_bytes_answers_without_a_gpu_and_rejects_a_bad_P():
    from hgs import _lib
    lib = _lib.lib()
    for P in (0, 1, 255, 256, 257, 1_000_000, 2 ** 31 - 1):
        n = lib.hgs_step_tmp_bytes(P)
        assert P + 4 <= n <= P + 1024 and n % 256 == 0, (P, n)             # one byte per row and the word
    assert lib.hgs_step_tmp_bytes(-1) == 0
    assert b"bad sizes" in lib.hgs_last_error()
    assert lib.hgs_step_tmp_bytes(2 ** 31) == 0


def test_select_and_apply_check_their_arguments_before_any_hip_call():
    """No GPU here: a call that got as far as HIP would fail with HGS_ERR_HIP, these fail with HGS_ERR_INVALID; and the
    calls with nothing to do return HGS_OK without a launch."""
    import ctypes as C
    from hgs import _lib
    lib = _lib.lib()
    src = open(os.path.join(ROOT, "include", "hgs.h")).read()
    invalid = int(re.search(r"HGS_ERR_INVALID\s*=\s*(\d+)", src).group(1))
    p = 256                                            # never dereferenced: every call below is refused first

    def args(**kw):
        base = dict(P=10, n=10, radii=p, max_radii2D=p, accum=p, denom=p, means2D_grad=p, opacity_grad=p)
        base.update(kw)
        return _lib.StepArgs(**base)
    sel = lambda a, tmp=C.c_void_p(p): lib.hgs_step_select(C.byref(a), tmp, None, 0)
    assert lib.hgs_step_select(None, C.c_void_p(p), None, 0) == invalid
    assert sel(args(P=-1)) == invalid and b"bad sizes" in lib.hgs_last_error()
    assert sel(args(P=2 ** 31)) == invalid
    assert sel(args(n=-1)) == invalid
    assert sel(args(lock_head=6, lock_tail=5)) == invalid and b"exceed" in lib.hgs_last_error()
    assert sel(args(lock_head=-1)) == invalid
    assert sel(args(protect_head=11)) == invalid and b"protected" in lib.hgs_last_error()
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        assert sel(args(clamp=1, clamp_threshold=thr)) == invalid and b"threshold" in lib.hgs_last_error()
    assert sel(args(radii=None)) == invalid
    assert sel(args(max_radii2D=None)) == invalid
    assert sel(args(indices=p, visible=p)) == invalid and b"not both" in lib.hgs_last_error()
    assert sel(args(n=11)) == invalid and b"no indices" in lib.hgs_last_error()
    assert sel(args(denom=None)) == invalid and b"together" in lib.hgs_last_error()
    assert sel(args(means2D_grad=None)) == invalid
    assert sel(args(), tmp=None) == invalid and b"tmp" in lib.hgs_last_error()
    assert sel(args(P=0, n=0)) == 0                    # nothing to do: no launch

    def tensor(flags=0, **kw):
        base = dict(param=p, grad=p, exp_avg=p, exp_avg_sq=p, row_len=3)
        base.update(kw)
        return (_lib.StepTensor * 1)(_lib.StepTensor(adam=_lib.AdamTensor(**base), flags=flags))
    app = lambda a, t, n=1, tmp=C.c_void_p(p): lib.hgs_step_apply(C.byref(a), t, n, tmp, None, 0)
    assert app(args(), tensor(), n=9) == invalid
    assert app(args(), None) == invalid
    assert app(args(P=-1), tensor()) == invalid
    assert app(args(), tensor(), tmp=None) == invalid
    assert app(args(), tensor(row_len=0)) == invalid
    assert app(args(), tensor(param=None)) == invalid
    assert app(args(), tensor(exp_avg=None)) == invalid
    assert app(args(), tensor(flags=8)) == invalid and b"flags" in lib.hgs_last_error()
    assert app(args(), tensor(flags=_lib.STEP_SCALING, row_len=4)) == invalid and b"3 floats" in lib.hgs_last_error()
    assert app(args(clamp=1, clamp_threshold=1.0), tensor()) == invalid and b"exactly one" in lib.hgs_last_error()
    assert app(args(P=2 ** 31 - 1, n=0), tensor(row_len=2 ** 31 - 1)) == invalid and b"overflow" in lib.hgs_last_error()
    assert app(args(), tensor(), n=0) == 0
    assert app(args(P=0, n=0), tensor()) == 0
    assert app(args(), tensor(grad=None, exp_avg=None, exp_avg_sq=None)) == 0       # no gradient, no clamp: no launch
    assert C.sizeof(_lib.StepTensor) == C.sizeof(_lib.AdamTensor) + 8
    assert C.sizeof(_lib.StepArgs) == 2 * 8 + 9 * 8 + 3 * 8 + 4 * 4


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("c++filt")),
                    reason="needs hipcc (cross-compiles without a GPU) and c++filt")
def test_step_kernels_compile_for_gfx950_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    rows = {r["kernel"]: r for r in kernel_resources.collect(
        [os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc", "train_step.hip")])}
    for name in ("step_select_kernel", "step_apply_kernel<unsigned int>", "step_apply_kernel<long>"):
        assert name in rows, (name, sorted(rows))
        r = rows[name]
        print(name, {k: r[k] for k in ("vgpr", "agpr", "sgpr", "lds", "scratch", "waves_regs", "waves_lds")})
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
        assert r["lds"] == 0
        assert min(r["waves_regs"], r["waves_lds"]) >= 4, (name, r["waves_regs"], r["waves_lds"])   # HBM-bound streams
