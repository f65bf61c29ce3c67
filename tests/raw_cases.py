"""Shared by tests/test_raw_gpu.py, tests/test_raw_edges_cpu.py and tests/test_raw_edges_gpu.py (a helper module, not a
test): the runners of the raw-parameter entrance (``GaussianRasterizer.forward_raw``) and of its float64 oracle
(``oracle.raster_oracle.rasterize`` behind ``ro.activate_raw``), and the named edge cases both edge suites use.

Every builder returns ``(raw, cam, bg, gc, gd, stored_degree, active_degree, act)``: ``raw`` the six tensors of
scene/gaussian_model.py as the optimiser holds them (xyz, f_dc, f_rest, opacity, scaling, rotation), ``stored_degree``
the SH degree ``f_rest`` has room for, ``active_degree`` the one the settings ask for, ``act`` the opacity activation.
All images are 53x37 or 64x48 and all P <= 600, so one oracle run takes seconds.  The seeds in ``SEEDS`` are fixed so
that every case keeps its share of knife-edge pixels under ``parity.FRAGILE_FRAC`` (tests/test_raw_edges_cpu.py
asserts it, with no GPU)."""
import numpy as np
import torch

import parity as pa
from hgs import synth
from oracle import raster_oracle as ro

BG = torch.tensor([0.1, 0.2, 0.3])
RAW_KEYS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
SMALL, WIDE = (53, 37), (64, 48)          # (W, H): off the 16-pixel tile grid, and on it


# ---- runners (moved here from tests/test_raw_gpu.py) ------------------------------------------------------------------
def _raw_from_scene(scene, seed, logit=True):
    g = torch.Generator().manual_seed(seed)
    op = scene.opacities.clamp(1e-4, 1 - 1e-4)
    return dict(
        xyz=scene.means3D.clone(),
        f_dc=scene.shs[:, :1].contiguous().clone(),
        f_rest=scene.shs[:, 1:].contiguous().clone(),
        opacity=(torch.log(op / (1 - op)) if logit else op * torch.where(torch.rand(op.shape, generator=g) < 0.5, -1.0, 1.0)),
        scaling=torch.log(scene.scales),
        rotation=scene.rotations * (0.5 + torch.rand(scene.P, 1, generator=g) * 2.0),   # un-normalised
    )


def _oracle_raw(raw, cam, bg, sh_degree, act):
    """The oracle of the raw entrance: float64 leaves, the activations of ``ro.activate_raw`` in front of the blend."""
    leaves = {k: v.clone().double().requires_grad_(True) for k, v in raw.items()}
    leaves["means2D"] = torch.zeros(raw["xyz"].shape[0], 3, dtype=torch.float64, requires_grad=True)

    def call(lv, **extra):
        s, r, o = ro.activate_raw(lv["scaling"], lv["rotation"], lv["opacity"], act)
        shs = torch.cat([lv["f_dc"], lv["f_rest"]], 1)
        return ro.rasterize(lv["xyz"], lv["means2D"], shs, None, o, s, r, None, image_height=cam.image_height,
                            image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg,
                            scale_modifier=1.0, viewmatrix=cam.world_view_transform,
                            projmatrix=cam.full_proj_transform, sh_degree=sh_degree, campos=cam.camera_center, **extra)
    return pa.OracleRun(leaves, call)


def _run_hip_raw(raw, cam, bg, gc, gd, sh_degree, act, device, debug=True, *, do_depth=True, context=None,
                 active_degree=None):
    """``active_degree``: the settings' SH degree when it is not the stored one (``sh_degree``).  ``context``: a
    RasterContext; a gradient that went into one of its buffers (``.grad`` stays None) is listed in "no_grad" and left
    out of "grads", and so is the gradient of an empty ``f_rest``."""
    import diff_gaussian_rasterization as dgr
    deg = sh_degree if active_degree is None else active_degree
    leaves = {k: v.clone().to(device).requires_grad_(True) for k, v in raw.items()}
    m2 = torch.zeros(raw["xyz"].shape[0], 3, device=device, requires_grad=True)
    rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(cam, bg, deg, do_depth=do_depth, debug=debug,
                                                                device=device))
    color, radii, invd = dgr.GaussianRasterizer(rs, context=context).forward_raw(
        leaves["xyz"], m2, leaves["f_dc"], leaves["f_rest"], leaves["opacity"], leaves["scaling"],
        leaves["rotation"], opacity_activation=act)
    call = color.grad_fn.call
    views = {k: v.cpu().clone() for k, v in dgr._C.raster_views(call).items()}
    loss = (color * gc.to(device)).sum()
    if do_depth:
        loss = loss + (invd * gd.to(device)).sum()
    loss.backward()
    torch.cuda.synchronize()
    leaves["means2D"] = m2
    grads = {k: v.grad.detach().cpu() for k, v in leaves.items() if v.grad is not None}
    return dict(color=color.detach().cpu(), radii=radii.cpu(), invdepth=invd.detach().cpu(), views=views, L=call.L,
                grads=grads, no_grad=[k for k, v in leaves.items() if v.grad is None])


def _compare(hip, res):
    idx = pa.check_indices(hip, res["oracle"])
    assert all(v == 0 for v in idx.values()), idx
    st = res["stats"]
    assert st["fragile_frac"] <= pa.FRAGILE_FRAC
    assert st["fragile_unmatched"] == 0 and st["fragile_unenumerated"] == 0, st
    assert st["n_contrib_mismatch"] == 0, st["n_contrib_mismatch"]
    for k, v in st.items():
        if isinstance(v, dict):
            assert v["maxrel"] <= pa.REL_TOL and v["l2"] <= pa.REL_TOL, (k, v)


# ---- the named cases ---------------------------------------------------------------------------------------------------
SPLIT_P3 = (1, 63, 64, 65, 255, 256, 257, 513)      # stored degree 3: f_rest rows of 45 floats
SPLIT_P12 = (1, 65, 257)                             # stored degrees 1 and 2: rows of 9 (cooperative) and 24 (per lane)
DEGREE_PAIRS = ((3, 0), (3, 1), (3, 2), (2, 1))      # (stored, active)
SIGMOID_RAW = (-90.0, -30.0, -17.0, -6.0, 0.0, 6.0, 17.0, 30.0, 90.0)
ABS_RAW = (0.0, -0.0, 1e-40, -1e-40, 0.5, -0.5, 1.0, -1.0)
NONE_RAW = (0.0, -0.0, -1e-3, -0.3, -2.0)            # rows <= 0 of the pass-through: never blended
SCALING_RAW = ((-12.0,) * 3, (-3.0,) * 3, (0.0,) * 3, (1.5,) * 3, (-9.0, 0.0, 1.0))
ROTATION_NORMS = (1e-6, 1e-3, 1.0, 50.0, 1e4)
P_ACT, P_ZERO_QUAT, ZERO_QUAT_ROW = 200, 65, 33

# seed of every case whose default (0) leaves more than FRAGILE_FRAC of the pixels on a knife edge (none does today)
SEEDS = {}


def _finish(name, scene, cam, size, stored, active, act, logit=None):
    W, H = size
    raw = _raw_from_scene(scene, seed=SEEDS.get(name, 0) + 1, logit=(act == "sigmoid") if logit is None else logit)
    gc, gd = synth.upstream_grads(H, W, seed=1)
    return raw, cam, BG, gc, gd, stored, active, act


def split_rows(P, stored):
    """A: split storage at P off the 256-row workgroup grid -- the 16-byte body / scalar tail split of coop_*_seg with
    ``count * nseg`` not a multiple of 4, a last workgroup of one row (257, 513)."""
    name = f"split_s{stored}_P{P}"
    cam = synth.make_camera(*SMALL)
    scene = synth.make_scene(P, cam, seed=SEEDS.get(name, 0), sh_degree=stored)
    return _finish(name, scene, cam, SMALL, stored, stored, "sigmoid")


def degree0():
    """B: ``f_rest`` of shape [P,0,3] -- the binding drops it, the activations run on the plain layout."""
    name = "degree0"
    cam = synth.make_camera(*SMALL)
    scene = synth.make_scene(65, cam, seed=SEEDS.get(name, 0), sh_degree=0)
    return _finish(name, scene, cam, SMALL, 0, 0, "sigmoid")


def lowered_degree(stored, active):
    """B: active degree below the stored one on split storage."""
    name = f"degree_s{stored}_a{active}"
    cam = synth.make_camera(*SMALL)
    scene = synth.make_scene(300, cam, seed=SEEDS.get(name, 0), sh_degree=stored)
    return _finish(name, scene, cam, SMALL, stored, active, "sigmoid")


def culled_rows(P):
    """C: which rows of the mostly-culled case are moved out of view, and how (bool masks over the rows)."""
    rows = torch.arange(P)
    wg0, wg2 = rows < 256, rows >= 512
    behind = (wg0 & (rows % 4 == 1)) | (wg2 & (rows % 3 == 0))
    beside = wg0 & ((rows % 4 == 2) | (rows % 4 == 3))
    return behind, beside


def mostly_culled(stored):
    """C: P = 600; rows 0..255 three quarters behind the camera or far beside the frustum (K1 then loads the visible
    rows' coefficients per lane: ``load_sh_split``), rows 256..511 all in view, rows 512..599 mixed; plus the
    clamped-colour rows of test_k8_fused_gpu._awkward_scene."""
    name = f"culled_s{stored}"
    cam = synth.make_camera(*WIDE)                   # at the origin, looking down +z: world = camera space
    scene = synth.make_scene(600, cam, seed=SEEDS.get(name, 0), sh_degree=stored)
    behind, beside = culled_rows(600)
    scene.means3D[behind, 2] = -scene.means3D[behind, 2]
    scene.means3D[beside, 0] = 40.0 * scene.means3D[beside, 2]
    scene.shs[1::5, 0] = -3.0                        # all three channels below zero
    scene.shs[2::5, 0, 0] = -3.0                     # red only
    scene.shs[4::5, 0, 1:] = -3.0                    # green and blue
    return _finish(name, scene, cam, WIDE, stored, stored, "sigmoid")


def accumulate_view(stored, view):
    """D: one of the two views whose gradients are accumulated into caller buffers (the same Gaussians, two cameras)."""
    name = f"accum_s{stored}"
    scene = synth.make_scene(257, synth.make_camera(*SMALL), seed=SEEDS.get(name, 0), sh_degree=stored)
    cam = synth.orbit_camera(*SMALL, view, 2, radius=0.3)
    return _finish(name, scene, cam, SMALL, stored, stored, "sigmoid")


def _special_rows(P):
    """F: every other row is a special one, so special and ordinary rows share wavefronts."""
    return torch.arange(1, P, 2)


def _act_scene(name, P=P_ACT):
    cam = synth.make_camera(*WIDE)
    return cam, synth.make_scene(P, cam, seed=SEEDS.get(name, 0))


def _cycle(values, n):
    t = torch.tensor(values, dtype=torch.float32)
    return t[torch.arange(n) % t.shape[0]]


def sigmoid_edges():
    """F: the sigmoid saturated both ways.  float32(sigmoid(17)) = 1 - 2^-24 and d(sigmoid) = 4e-8 there;
    float32(sigmoid(30)) = float32(sigmoid(90)) = 1 exactly; sigmoid(-90) = 8e-40 is a float32 denormal."""
    name = "act_sigmoid"
    cam, scene = _act_scene(name)
    out = _finish(name, scene, cam, WIDE, 3, 3, "sigmoid")
    sp = _special_rows(P_ACT)
    out[0]["opacity"][sp, 0] = _cycle(SIGMOID_RAW, sp.numel())
    return out


def abs_edges():
    """F: abs at +0, -0, denormals of both signs, and ordinary values of both signs."""
    name = "act_abs"
    cam, scene = _act_scene(name)
    out = _finish(name, scene, cam, WIDE, 3, 3, "abs")
    sp = _special_rows(P_ACT)
    out[0]["opacity"][sp, 0] = _cycle(ABS_RAW, sp.numel())
    return out


def none_edges():
    """F: opacities passed as they are (rows <= 0 are never blended); scale exp and rotation normalisation stay on."""
    name = "act_none"
    cam, scene = _act_scene(name)
    out = _finish(name, scene, cam, WIDE, 3, 3, "none", logit=True)
    out[0]["opacity"] = scene.opacities.clone()
    sp = _special_rows(P_ACT)[::2]                   # a quarter of the rows: the picture keeps its other Gaussians
    out[0]["opacity"][sp, 0] = _cycle(NONE_RAW, sp.numel())
    return out


def scaling_edges():
    """F: exp of very negative scales (the 0.3-pixel low-pass filter is all that is left of the footprint), of 0 and
    1.5 (screen-filling), and one row with all three at once."""
    name = "act_scaling"
    cam, scene = _act_scene(name)
    out = _finish(name, scene, cam, WIDE, 3, 3, "sigmoid")
    sp = _special_rows(P_ACT)[::2]
    out[0]["scaling"][sp] = _cycle(SCALING_RAW, sp.numel())
    return out


def rotation_edges():
    """F: raw quaternion norms from 1e-6 to 1e4, every fourth special row with a negative w."""
    name = "act_rotation"
    cam, scene = _act_scene(name)
    out = _finish(name, scene, cam, WIDE, 3, 3, "sigmoid")
    sp = _special_rows(P_ACT)
    q = scene.rotations[sp].clone()
    q[::4, 0] = -q[::4, 0].abs() - 0.1
    q = q / q.norm(dim=1, keepdim=True)
    out[0]["rotation"][sp] = q * _cycle(ROTATION_NORMS, sp.numel())[:, None]
    return out


def zero_quaternion():
    """F: one all-zero rotation row (behind ``fmax(|q|, 1e-12)``: the activated quaternion is zero, R the identity)."""
    name = "act_zero_quat"
    cam, scene = _act_scene(name, P_ZERO_QUAT)
    out = _finish(name, scene, cam, WIDE, 3, 3, "sigmoid")
    out[0]["rotation"][ZERO_QUAT_ROW] = 0.0
    return out


CASES = {}
for _P in SPLIT_P3:
    CASES[f"split_s3_P{_P}"] = (split_rows, (_P, 3))
for _s in (1, 2):
    for _P in SPLIT_P12:
        CASES[f"split_s{_s}_P{_P}"] = (split_rows, (_P, _s))
CASES["degree0"] = (degree0, ())
for _s, _a in DEGREE_PAIRS:
    CASES[f"degree_s{_s}_a{_a}"] = (lowered_degree, (_s, _a))
for _s in (3, 2):
    CASES[f"culled_s{_s}"] = (mostly_culled, (_s,))
    for _v in (0, 1):
        CASES[f"accum_s{_s}_v{_v}"] = (accumulate_view, (_s, _v))
CASES.update(act_sigmoid=(sigmoid_edges, ()), act_abs=(abs_edges, ()), act_none=(none_edges, ()),
             act_scaling=(scaling_edges, ()), act_rotation=(rotation_edges, ()), act_zero_quat=(zero_quaternion, ()))


def build(name):
    fn, args = CASES[name]
    return fn(*args)


def activated_scene(raw, sh_degree, act):
    """The case as the standard entrance takes it: torch's float32 activations of scene/gaussian_model.py:108-128
    (``sh_degree``: the active one)."""
    op = {"sigmoid": torch.sigmoid, "abs": torch.abs, "none": lambda t: t}[act](raw["opacity"])
    return synth.Scene(raw["xyz"].clone(), torch.exp(raw["scaling"]), torch.nn.functional.normalize(raw["rotation"]),
                       op, torch.cat([raw["f_dc"], raw["f_rest"]], 1).contiguous(), sh_degree)


def rows_touching_fragile(oracle_out):
    """[P] bool: the rows ``parity.rows_touching_fragile`` counts -- a fragile pixel inside the footprint rectangle."""
    fr, g = oracle_out.fragile, oracle_out.geom
    mask = np.zeros(g.visible.shape[0], dtype=bool)
    if not fr.any():
        return torch.from_numpy(mask)
    H, W = fr.shape
    ii = np.zeros((H + 1, W + 1), dtype=np.int64)
    ii[1:, 1:] = fr.astype(np.int64).cumsum(0).cumsum(1)
    vis = g.visible
    x0 = np.clip(np.floor(g.px[vis] - g.radii[vis]).astype(np.int64), 0, W)
    x1 = np.clip(np.ceil(g.px[vis] + g.radii[vis]).astype(np.int64) + 1, 0, W)
    y0 = np.clip(np.floor(g.py[vis] - g.radii[vis]).astype(np.int64), 0, H)
    y1 = np.clip(np.ceil(g.py[vis] + g.radii[vis]).astype(np.int64) + 1, 0, H)
    cnt = ii[y1, x1] - ii[y0, x1] - ii[y1, x0] + ii[y0, x0]
    mask[np.nonzero(vis)[0][cnt > 0]] = True
    return torch.from_numpy(mask)
