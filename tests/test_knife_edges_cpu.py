"""Without a GPU: the admissible-outcome enumerator, forced decisions, the band model and the matcher that the
``-m gpu`` parity tests rest on (tests/parity.py ``verify``; oracle/raster_oracle.py ``admissible_outcomes``)."""
import math

import numpy as np
import pytest
import torch

import knife_edges as ke
import parity as pa
from hgs import synth
from oracle import raster_oracle as ro

BG = torch.tensor([0.1, 0.2, 0.3])


def _one_gaussian_scene(opacities, z=(4.0,), size=32):
    """Isotropic Gaussians 3 px wide, centred 2.3 px right and 1.7 px below pixel (16, 16), colours handed in."""
    cam = synth.make_camera(size, size)
    n = len(opacities)
    zs = torch.tensor(z, dtype=torch.float64)
    fx = size / (2 * cam.tanfovx)
    cx, cy = 18.3, 17.7
    xyz = torch.stack([((2 * cx + 1) / size - 1) * zs * cam.tanfovx, ((2 * cy + 1) / size - 1) * zs * cam.tanfovy, zs], 1)
    scene = synth.Scene(xyz.float(), (3.0 * zs / fx)[:, None].repeat(1, 3).float(), torch.tensor([[1.0, 0, 0, 0]] * n),
                        torch.tensor(opacities, dtype=torch.float32)[:, None], torch.zeros(n, 16, 3), 0)
    cols = torch.tensor([[0.9, 0.5, 0.1], [0.2, 0.7, 0.4]][:n])
    return cam, scene, cols


def _oracle(cam, scene, cols, **kw):
    return pa.oracle_run(scene, cam, BG, colors_precomp=cols)(**kw)


def test_alpha_edge_pixel_has_two_outcomes_with_known_values():
    cam, scene, cols = _one_gaussian_scene([0.5])
    f = 16 * 32 + 16
    power = float(_oracle(cam, scene, cols, capture=[f]).rows[f].power[0])
    for delta in (1e-7, -1e-7):
        o = np.float32(ro.ALPHA_MIN * (1 + delta) / math.exp(power))
        scene.opacities[:] = float(o)
        out = _oracle(cam, scene, cols)
        assert out.fragile[16, 16]
        a = float(o) * math.exp(power)                                 # the float64 alpha at the pixel
        assert abs(a / ro.ALPHA_MIN - 1) < 2e-7
        outs, over = ro.admissible_outcomes(out, [f])
        assert over == [] and len(outs[f]) == 2
        live, skip = sorted(outs[f], key=lambda o: -o.n_contrib)
        c, bg = cols[0].double().numpy(), BG.double().numpy()
        assert live.n_contrib == 1 and abs(live.final_T - (1 - a)) < 1e-15
        assert np.abs(live.color - (c * a + (1 - a) * bg)).max() < 1e-15 and abs(live.invdepth - a / 4.0) < 1e-7
        assert skip.n_contrib == 0 and skip.final_T == 1.0 and np.abs(skip.color - bg).max() < 1e-15
        assert skip.invdepth == 0.0
        assert live.decisions == (("alpha", "live"),) and skip.decisions == (("alpha", "skip"),)
        # the float64 decision comes first
        assert outs[f][0] is (live if a >= ro.ALPHA_MIN else skip)


def test_capped_stack_stops_after_one_or_two():
    """Two Gaussians capped at 0.99 on the same pixel: float64 gives T = 1.0000000000000018e-4 (continue, two blended),
    float32 9.99998e-5 (stop after one): n_contrib 1 with T = 0.01, or 2 with T = 1e-4."""
    cam, scene, cols = _one_gaussian_scene([1.9, 1.9], z=(4.0, 4.5))
    cx = (18.3, 17.7)
    f = 18 * 32 + 18
    out = _oracle(cam, scene, cols)
    assert out.fragile[18, 18] and out.n_contrib[18, 18] == 2
    outs, _ = ro.admissible_outcomes(out, [f])
    got = sorted((o.n_contrib, o.final_T) for o in outs[f])
    assert len(got) == 2 and got[0][0] == 1 and got[1][0] == 2, (got, cx)
    assert abs(got[0][1] - 0.01) < 1e-15 and abs(got[1][1] - 1e-4) < 1e-15


@pytest.mark.parametrize("seed", [0, 5])
def test_non_fragile_pixels_have_exactly_the_oracle_outcome(seed):
    cam, scene, _, _ = pa.default_case(600, 96, 64, seed=seed)
    rng = np.random.default_rng(seed)
    pick = rng.choice(96 * 64, 300, replace=False)
    out = pa.oracle_run(scene, cam, BG)(capture=pick)
    pick = [int(f) for f in pick if not out.fragile.reshape(-1)[f]]
    outs, over = ro.admissible_outcomes(out, pick)
    assert over == [] and len(outs) == len(pick) > 250
    col, dep, nc, T = (out.color.detach().reshape(3, -1), out.invdepth.detach().reshape(-1),
                       out.n_contrib.reshape(-1), out.final_T.reshape(-1))
    for f in pick:
        assert len(outs[f]) == 1, f
        o = outs[f][0]
        assert o.n_contrib == nc[f] and o.decisions == ()
        assert np.abs(o.color - col[:, f].numpy()).max() < 1e-12 and abs(o.invdepth - float(dep[f])) < 1e-12
        assert abs(o.final_T - T[f]) < 1e-12


def _loss(out, gc, gd):
    return (out.color * gc.double()).sum() + (out.invdepth * gd.double()).sum()


def test_override_with_the_default_decisions_changes_nothing():
    s = ke.build(seed=2, n_alpha=60, n_chain=6)
    gc, gd = synth.upstream_grads(ke.H, ke.W, seed=1)
    a = pa.oracle_run(s["scene"], s["cam"], BG)
    oa = a(return_keep=True)
    _loss(oa, gc, gd).backward()
    keep = {}
    for t, k in oa.keep.items():
        keep.update(zip(pa.tile_pixels(t, ke.W, ke.H), k))
    b = pa.oracle_run(s["scene"], s["cam"], BG)
    ob = b(keep_override=keep)
    _loss(ob, gc, gd).backward()
    assert torch.equal(oa.color, ob.color) and torch.equal(oa.invdepth, ob.invdepth)
    assert np.array_equal(oa.n_contrib, ob.n_contrib) and np.array_equal(oa.final_T, ob.final_T)
    for k, g in a.grads().items():
        assert torch.equal(g, b.grads()[k]), k


def test_forced_outcome_gradients_equal_a_literal_walk():
    """Pixels forced to a non-float64 outcome: the gradients w.r.t. the colours and opacities of a loss on those pixels
    equal autograd through a literal front-to-back float64 loop that blends exactly the forced entries."""
    s = ke.build(seed=3, precomp=True, n_alpha=60, n_chain=6)
    out = pa.oracle_run(s["scene"], s["cam"], BG, colors_precomp=s["colors_precomp"])()
    outs, _ = ro.admissible_outcomes(out)
    pix = sorted(f for f, o in outs.items() if len(o) > 1)[:40]
    assert len(pix) == 40
    force = {f: outs[f][1].keep for f in pix}
    g = torch.Generator().manual_seed(4)
    gc = torch.zeros(3, ke.H, ke.W)
    gd = torch.zeros(1, ke.H, ke.W)
    for f in pix:
        y, x = divmod(f, ke.W)
        gc[:, y, x] = torch.randn(3, generator=g)
        gd[0, y, x] = float(torch.randn(1, generator=g))
    sc = s["scene"]                                     # float64 leaves (same values): gradients not rounded to float32
    sc64 = synth.Scene(*(t.double() for t in (sc.means3D, sc.scales, sc.rotations, sc.opacities, sc.shs)), sc.sh_degree)
    orc = pa.oracle_run(sc64, s["cam"], BG, colors_precomp=s["colors_precomp"].double())
    forced = orc(keep_override=force)
    _loss(forced, gc, gd).backward()
    for f in pix:                                       # the forced forward is the enumerated outcome
        y, x = divmod(f, ke.W)
        assert np.abs(forced.color.detach()[:, y, x].numpy() - outs[f][1].color).max() < 1e-12
        assert forced.n_contrib[y, x] == outs[f][1].n_contrib
    col = s["colors_precomp"].double().clone().requires_grad_(True)
    op = s["scene"].opacities.double().clone().requires_grad_(True)
    bg = BG.double()
    loss = 0.0
    for f in pix:
        y, x = divmod(f, ke.W)
        row, keep = out.rows[f], force[f]
        T, c, d = 1.0, torch.zeros(3, dtype=torch.float64), 0.0
        for i in np.flatnonzero(keep):
            gid = int(row.ids[i])
            raw = op[gid, 0] * math.exp(float(row.power[i]))
            a = raw + (raw.clamp(max=ro.ALPHA_MAX) - raw).detach()      # the oracle's straight-through cap
            c = c + col[gid] * a * T
            d = d + float(row.invz[i]) * a * T
            T = T * (1 - a)
        c = c + T * bg
        loss = loss + (c * gc[:, y, x].double()).sum() + d * float(gd[0, y, x])
    loss.backward()
    for name, lit in (("colors_precomp", col.grad), ("opacities", op.grad)):
        got = orc.grads()[name]
        assert (got - lit).abs().max() <= 1e-12 * max(1.0, float(lit.abs().max())), name
    assert float(op.grad.abs().max()) > 0


def _as_hip(out, grads=None):
    """A fake kernel result made of an oracle output."""
    return dict(color=out.color.detach().clone(), invdepth=out.invdepth.detach().clone(),
                views=dict(n_contrib=torch.from_numpy(out.n_contrib.copy()), final_T=torch.from_numpy(out.final_T.copy())),
                grads={} if grads is None else {k: v.clone() for k, v in grads.items()})


BAND_CASES = [("knife", dict()), ("knife_lod_opacity", dict(lod="opacity")), ("knife_lod_alpha", dict(lod="alpha")),
              ("default_0", 0), ("default_1", 1), ("default_2", 2)]


@pytest.mark.parametrize("name,case", BAND_CASES, ids=[c[0] for c in BAND_CASES])
def test_band_model_holds_for_the_kernels_precision_split(name, case):
    """``rasterize(dtype=float32, geom_dtype=float64)`` -- the kernels' precision split -- as a stand-in kernel: every
    knife-edge pixel reproduces an admissible float64 outcome, every other pixel takes the float64 decisions.  A failure
    here means the band (``ro.alpha_band`` / ``ro.t_noise``) is too narrow for float32."""
    if isinstance(case, dict):
        s = ke.build(seed=0, **case)
        scene, cam = s["scene"], s["cam"]
        kw = dict(interpolation_weights=s["interpolation_weights"], num_node_kids=s["num_node_kids"],
                  lod_mode=s["lod_mode"])
    else:
        cam, scene, _, _ = pa.default_case(1000, 128, 128, seed=case)
        kw = {}
    o64 = pa.oracle_run(scene, cam, BG, **kw)()
    o32 = pa.oracle_run(scene, cam, BG, dtype=torch.float32, geom_dtype=torch.float64, **kw)()
    m = pa.match_fragile(_as_hip(o32), o64)
    st = m["stats"]
    assert st["fragile_unmatched"] == 0 and st["fragile_unenumerated"] == 0, st
    steady = ~o64.fragile
    assert np.array_equal(o32.n_contrib[steady], o64.n_contrib[steady])
    t = torch.from_numpy(steady)
    assert pa.err_stats(o32.color.detach()[:, t], o64.color.detach()[:, t])["mixed"] <= 1.0
    if isinstance(case, dict):
        assert st["fragile"] >= 600 and st["forced"] >= 300, st     # the scenes do put pixels on the edges


# ---- negative controls: the check must reject what is wrong --------------------------------------------------------
@pytest.fixture(scope="module")
def knife():
    s = ke.build(seed=4, n_alpha=120, n_chain=8)
    gc, gd = synth.upstream_grads(ke.H, ke.W, seed=2)
    orc = pa.oracle_run(s["scene"], s["cam"], BG)
    out = orc()
    _loss(out, gc, gd).backward()
    outs, _ = ro.admissible_outcomes(out)
    return dict(s=s, gc=gc, gd=gd, out=out, grads=orc.grads(), outs=outs)


def _verify(k, hip):
    return pa.verify(hip, pa.oracle_run(k["s"]["scene"], k["s"]["cam"], BG), k["gc"], k["gd"])


def test_the_oracle_itself_passes(knife):
    pa.assert_verified("oracle as kernel", _verify(knife, _as_hip(knife["out"], knife["grads"])), fragile_frac=1.0)


@pytest.mark.parametrize("field", ["n_contrib", "final_T"])
def test_mixed_outcomes_are_rejected(knife, field):
    """One outcome's colour with another outcome's n_contrib / final T matches no outcome."""
    hip = _as_hip(knife["out"], knife["grads"])
    mixed = 0
    for f, o in knife["outs"].items():
        other = next((b for b in o[1:] if getattr(b, field) != getattr(o[0], field)), None)
        if other is None:
            continue
        hip["views"][field].view(-1)[f] = getattr(other, field)
        mixed += 1
    assert mixed >= 100
    st = _verify(knife, hip)["stats"]
    assert st["fragile_unmatched"] == mixed, st


def test_an_extra_blended_entry_outside_the_band_is_rejected(knife):
    """A pixel that is not on a knife edge blends one more entry, whose alpha is well below 1/255."""
    steady = np.flatnonzero(~knife["out"].fragile.reshape(-1))[::7][:400].tolist()
    rows = pa.oracle_run(knife["s"]["scene"], knife["s"]["cam"], BG)(capture=steady, return_keep=True)
    keep = {}
    for t, k in rows.keep.items():
        keep.update(zip(pa.tile_pixels(t, ke.W, ke.H), k))
    chosen = {}
    for f in steady:
        r = rows.rows[f]
        extra = np.flatnonzero(~keep[f] & (r.power <= 0) & (r.alpha > 0.3 * ro.ALPHA_MIN) & (r.alpha < 0.8 * ro.ALPHA_MIN))
        if len(extra):
            row = keep[f].copy()
            row[extra[0]] = True
            chosen[f] = row
    assert len(chosen) >= 3, len(chosen)
    orc = pa.oracle_run(knife["s"]["scene"], knife["s"]["cam"], BG)
    bad = orc(keep_override=chosen)
    _loss(bad, knife["gc"], knife["gd"]).backward()
    res = _verify(knife, _as_hip(bad, orc.grads()))
    with pytest.raises(AssertionError):
        pa.assert_verified("extra entry", res, fragile_frac=1.0)


def test_gradients_of_another_outcome_are_rejected(knife):
    """Forward of the float64 outcomes, gradients of the other outcome at every knife-edge pixel: what a K7 that decides
    differently from K6 would hand back."""
    force = {f: o[1].keep for f, o in knife["outs"].items() if len(o) > 1}
    orc = pa.oracle_run(knife["s"]["scene"], knife["s"]["cam"], BG)
    _loss(orc(keep_override=force), knife["gc"], knife["gd"]).backward()
    res = _verify(knife, _as_hip(knife["out"], orc.grads()))
    assert res["stats"]["fragile_unmatched"] == 0 and res["stats"]["n_contrib_mismatch"] == 0
    with pytest.raises(AssertionError, match="d_"):
        pa.assert_stats("other outcome's gradients", res["stats"])
