"""The named edge cases of the raw-parameter path (tests/raw_cases.py), checked with no GPU: every case runs through the
float64 oracle alone and must (a) keep its share of knife-edge pixels under ``parity.FRAGILE_FRAC`` with finite
gradients, (b) contain what it is named for, counted on the oracle's own outputs, and (c) give raw-parameter gradients
that agree with ``parity.chain_to_raw`` applied to the standard oracle run on torch-activated inputs -- two independent
float64 derivations of the same chain rule, so that a kernel bug cannot hide behind a bug of the specification
(``ro.activate_raw``).  tests/test_raw_edges_gpu.py runs the kernels on the same cases."""
import functools

import numpy as np
import pytest
import torch

import parity as pa
import raw_cases as rc
from oracle import raster_oracle as ro

# (c): the two derivations differ by the float32 rounding of the activated values -- the oracle of the raw path rounds the
# float64 activation once, torch activates in float32 -- which moves a gradient by a few float32 ulps times its
# conditioning.  Measured over all cases: max|d| / max|ref| <= 1.82e-6 (rotation, accum_s3_v1), relative L2 <= 5.64e-7
# (rotation, degree0); the bounds are those figures times 10.
CHAIN_MAXREL = 1.82e-5
CHAIN_L2 = 5.64e-6


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(case, oracle output, {raw tensor: float64 gradient}) of the full, unmasked loss; computed once per case."""
    case = rc.build(name)
    raw, cam, bg, gc, gd, stored, active, act = case
    orc = rc._oracle_raw(raw, cam, bg, active, act)
    out = orc()
    ((out.color * gc.double()).sum() + (out.invdepth * gd.double()).sum()).backward()
    return case, out, orc.grads()


def _activated(raw, act):
    """float32 values of the activated attributes as ``ro.activate_raw`` defines them."""
    with torch.no_grad():
        s, r, o = ro.activate_raw(raw["scaling"], raw["rotation"], raw["opacity"], act)
    return s.float(), r.float(), o.float()


@pytest.mark.parametrize("name", list(rc.CASES))
def test_case_is_decidable_and_finite(name):
    (raw, *_), out, grads = _oracle(name)
    ff = float(out.fragile.mean())
    print(f"{name}: fragile fraction {ff:.3e} ({int(out.fragile.sum())} pixels), {int(out.geom.visible.sum())} of "
          f"{raw['xyz'].shape[0]} rows visible")
    assert ff <= pa.FRAGILE_FRAC, (name, ff)
    for k, g in grads.items():
        assert g is None and k == "f_rest" and raw[k].numel() == 0 or bool(torch.isfinite(g).all()), (name, k)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_raw_gradients_agree_with_the_chained_standard_run(name):
    (raw, cam, bg, gc, gd, stored, active, act), out, grads = _oracle(name)
    o2, og = pa.run_oracle(rc.activated_scene(raw, active, act), cam, bg, gc, gd, mask_fragile=False)
    ch = pa.chain_to_raw(dict(xyz=raw["xyz"], scaling=raw["scaling"], rotation=raw["rotation"], opacity=raw["opacity"],
                              features_dc=raw["f_dc"], features_rest=raw["f_rest"]), og, act)
    ch = dict(xyz=ch["xyz"], f_dc=ch["features_dc"], f_rest=ch["features_rest"], opacity=ch["opacity"],
              scaling=ch["scaling"], rotation=ch["rotation"], means2D=og["means2D"])
    skip = rc.rows_touching_fragile(out) | rc.rows_touching_fragile(o2)     # a knife edge may fall either way
    assert float(o2.fragile.mean()) <= pa.FRAGILE_FRAC
    for k, b in ch.items():
        a = grads[k]
        if a is None or a.numel() == 0:
            assert raw[k].numel() == 0, (name, k)
            continue
        a, b = a.clone(), b.reshape(a.shape).clone()
        a[skip], b[skip] = 0, 0
        st = pa.err_stats(a, b)
        print(f"{name}: d_{k} maxrel {st['maxrel']:.2e} l2 {st['l2']:.2e}")
        assert st["maxrel"] <= CHAIN_MAXREL and st["l2"] <= CHAIN_L2, (name, k, st)


# ---- every case contains what it is named for ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in rc.CASES if n.startswith("split_")])
def test_split_cases_leave_a_scalar_tail(name):
    (raw, *_, stored, _, _), out, grads = _oracle(name)
    P, nr = raw["xyz"].shape[0], raw["f_rest"].shape[1] * 3
    assert nr == ((stored + 1) ** 2 - 1) * 3 and bool(out.geom.visible.all())    # every workgroup takes its block route
    last = P - (P - 1) // 256 * 256                                               # rows of the last workgroup
    if P % 4:        # the 16-byte body of a workgroup's 3- and nr-float rows ends before the block does
        assert (last * 3) % 4 != 0 and (nr % 4 == 0 or (last * nr) % 4 != 0), (P, nr)
    if P > 256:
        assert last == 1
    if P > 1:
        assert bool(grads["f_rest"].any()) and bool(grads["f_dc"].any())


@pytest.mark.parametrize("name", ["degree0"] + [f"degree_s{s}_a{a}" for s, a in rc.DEGREE_PAIRS])
def test_degree_cases_stop_at_the_active_coefficients(name):
    (raw, *_, stored, active, _), out, grads = _oracle(name)
    assert raw["f_rest"].shape[1] == (stored + 1) ** 2 - 1 and active <= stored
    if stored == 0:
        assert raw["f_rest"].numel() == 0
        return
    nb = (active + 1) ** 2
    g = grads["f_rest"]
    assert not bool(g[:, nb - 1:].any()) and (active == 0 or bool(g[:, :nb - 1].any()))


@pytest.mark.parametrize("name", ["culled_s3", "culled_s2"])
def test_culled_case_has_a_mostly_culled_workgroup_and_clamped_colours(name):
    (raw, cam, *_, active, _), out, grads = _oracle(name)
    vis = torch.from_numpy(out.geom.tiles_touched > 0)
    behind, beside = rc.culled_rows(600)
    assert 0 < int(vis[:256].sum()) < 128 and int(vis[256:512].sum()) >= 128
    assert 0 < int(vis[512:].sum()) < 88 and not bool(vis[behind | beside].any())
    for k, g in grads.items():                                        # a culled row takes no gradient
        assert not bool(g[~vis].any()), k
    d = raw["xyz"].double() - cam.camera_center.double()
    rgb = ro.eval_sh_torch(active, torch.cat([raw["f_dc"], raw["f_rest"]], 1).double(),
                           d / d.norm(dim=1, keepdim=True)) + 0.5
    clamped = (rgb < 0) & vis[:, None]
    red_only = clamped[:, 0] & ~clamped[:, 1] & ~clamped[:, 2]
    assert int(red_only.sum()) >= 30 and int(clamped.all(1).sum()) >= 30 and int((clamped[:, 1] & clamped[:, 2]).sum()) >= 30
    assert not bool(grads["f_dc"][red_only][:, 0, 0].any()) and bool(grads["f_dc"][red_only][:, 0, 1].any())


@pytest.mark.parametrize("name", [n for n in rc.CASES if n.startswith("accum_")])
def test_accumulation_views_both_see_the_scene(name):
    (raw, *_), out, grads = _oracle(name)
    assert raw["xyz"].shape[0] == 257 and int(out.geom.visible.sum()) >= 200
    other = name[:-1] + ("1" if name.endswith("0") else "0")
    assert torch.equal(raw["f_rest"], rc.build(other)[0]["f_rest"])              # the same Gaussians ...
    assert not torch.equal(grads["f_rest"], _oracle(other)[2]["f_rest"])          # ... from two cameras


def _special(values, rows):
    """{value index: rows that hold it} of a case whose special ``rows`` cycle through ``values``."""
    return {i: rows[i::len(values)] for i in range(len(values))}


def test_sigmoid_case_saturates_both_ways():
    (raw, *_), out, grads = _oracle("act_sigmoid")
    sp = _special(rc.SIGMOID_RAW, rc._special_rows(rc.P_ACT))
    for i, v in enumerate(rc.SIGMOID_RAW):
        assert bool((raw["opacity"][sp[i], 0] == v).all()) and sp[i].numel() >= 11
    _, _, o = _activated(raw, "sigmoid")
    o = o.reshape(-1)
    one = torch.cat([sp[7], sp[8]])                                   # raw 30 and 90: exactly 1.0f
    assert bool((o[one] == 1.0).all()) and one.numel() >= 22
    assert bool((o[sp[6]] == 1.0 - 2.0 ** -24).all())                 # raw 17: the last float32 below 1
    tiny = o[sp[0]]                                                   # raw -90: a float32 denormal
    assert bool(((tiny > 0) & (tiny < torch.finfo(torch.float32).tiny)).all())
    never = torch.cat([sp[0], sp[1], sp[2], sp[3]])                   # below 1/255: nothing to blend, no gradient at all
    assert bool((o[never] < 1.0 / 255.0).all()) and never.numel() >= 44
    for k in ("opacity", "xyz", "f_dc", "scaling", "rotation"):
        assert not bool(grads[k][never].any()), k
    live = torch.cat([sp[4], sp[5], sp[6], sp[7]])                    # up to raw 30 the tiny derivative is a normal number
    assert int((grads["opacity"][live, 0] != 0).sum()) >= 30


def test_abs_case_has_zeros_and_denormals_of_both_signs():
    (raw, *_), out, grads = _oracle("act_abs")
    sp = _special(rc.ABS_RAW, rc._special_rows(rc.P_ACT))
    r = raw["opacity"].reshape(-1)
    assert bool((r[sp[0]] == 0).all()) and not bool(torch.signbit(r[sp[0]]).any())
    assert bool((r[sp[1]] == 0).all()) and bool(torch.signbit(r[sp[1]]).all())
    tiny = torch.finfo(torch.float32).tiny
    assert bool(((r[sp[2]] > 0) & (r[sp[2]] < tiny)).all()) and bool(((r[sp[3]] < 0) & (r[sp[3]] > -tiny)).all())
    never = torch.cat([sp[0], sp[1], sp[2], sp[3]])
    assert never.numel() >= 48 and not bool(grads["opacity"][never].any())
    g = grads["opacity"].reshape(-1)
    for pos, neg in ((4, 5), (6, 7)):          # d|x|/dx = sign(x): the same Gaussian mirrored would flip its gradient
        assert int((g[sp[pos]] != 0).sum()) >= 8 and int((g[sp[neg]] != 0).sum()) >= 8


def test_none_case_has_rows_that_never_blend():
    (raw, *_), out, grads = _oracle("act_none")
    sp = rc._special_rows(rc.P_ACT)[::2]
    r = raw["opacity"].reshape(-1)
    assert sp.numel() >= 50 and bool((r[sp] <= 0).all()) and int((r[sp] < 0).sum()) >= 25
    for k in ("opacity", "xyz", "f_dc", "scaling", "rotation"):
        assert not bool(grads[k][sp].any()), k
    rest = torch.ones(rc.P_ACT, dtype=torch.bool)
    rest[sp] = False
    assert bool((r[rest] > 0.04).all()) and int((grads["opacity"][rest, 0] != 0).sum()) >= 100


def test_scaling_case_spans_low_pass_to_screen_filling():
    (raw, *_), out, grads = _oracle("act_scaling")
    sp = _special(rc.SCALING_RAW, rc._special_rows(rc.P_ACT)[::2])
    radii = torch.from_numpy(out.geom.radii)
    for i, v in enumerate(rc.SCALING_RAW):
        assert bool((raw["scaling"][sp[i]] == torch.tensor(v)).all()) and sp[i].numel() >= 10
    # exp(-12): the low-pass filter alone, ceil(3 sqrt(0.3 + sqrt(0.1))) pixels (the eigenvalue's discriminant floor of 0.1)
    assert bool((radii[sp[0]] == 3).all())
    assert bool((radii[sp[3]] >= 24).all())           # exp(1.5) world units: wider than half the picture
    assert bool((radii[sp[4]] >= 5).all())            # (-9, 0, 1): a sheet
    assert int((grads["scaling"][sp[0]] != 0).sum()) >= 10


def test_rotation_case_spans_ten_decades_of_norm():
    (raw, *_), out, grads = _oracle("act_rotation")
    sp = _special(rc.ROTATION_NORMS, rc._special_rows(rc.P_ACT))
    n = raw["rotation"].double().norm(dim=1)
    for i, v in enumerate(rc.ROTATION_NORMS):
        assert torch.allclose(n[sp[i]], torch.full((sp[i].numel(),), v, dtype=torch.float64), rtol=1e-6), v
    assert int((raw["rotation"][rc._special_rows(rc.P_ACT), 0] < 0).sum()) >= 25
    # the raw gradient is (I - q q^T) dq / |raw|: times |raw| it is orthogonal to q and of one magnitude over all norms
    g = grads["rotation"] * n[:, None]
    _, q, _ = _activated(raw, "sigmoid")
    assert float((g * q.double()).sum(1).abs().max()) <= 1e-6 * float(g.abs().max())
    per_norm = [float(g[sp[i]].abs().max()) for i in range(len(rc.ROTATION_NORMS))]
    assert max(per_norm) <= 1e3 * min(per_norm), per_norm


def test_zero_quaternion_case():
    (raw, *_), out, grads = _oracle("act_zero_quat")
    z = rc.ZERO_QUAT_ROW
    assert not bool(raw["rotation"][z].any()) and bool(out.geom.visible[z])
    _, q, _ = _activated(raw, "sigmoid")
    assert not bool(q[z].any())                       # behind max(|q|, 1e-12): the activated quaternion is zero, R = I
    assert not bool(grads["rotation"][z].any())       # R is quadratic in q: no first-order term at q = 0
    assert bool(grads["scaling"][z].any()) and bool(grads["opacity"][z].any())
