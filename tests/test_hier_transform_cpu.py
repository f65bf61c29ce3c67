"""The similarity transform of a hierarchy (hgs.hierarchy.transform_hierarchy, the numpy spec of csrc/hier_transform.hip)
without a GPU: the SH convention against oracle.raster_oracle.eval_sh_torch, the Gaussians' covariances, the identity,
composition and inverse, the boxes (nesting, signed permutations), the LOD cut under half-turns against
oracle/lod_oracle.py, a render of the float64 oracle from transformed rows and a transformed camera, the rejections of
the spec and of the C ABI's host-side checks, the command's argument parsing.  tests/test_hier_transform_gpu.py holds
the HIP call against this spec."""
import copy
import ctypes as C
import functools
import itertools
import re

import numpy as np
import pytest
import torch

from hgs import _lib, hierarchy, synth
from hgs import transform_hierarchy as cmd
from oracle import lod_oracle as lo
from oracle import raster_oracle as ro
from test_hier_trim_cpu import ARRAYS, HEADER, VIEWS, bits, scene2000

ROWS = ARRAYS[:5]
T_GENERAL = (3.0, -2.0, 9.0)
HALF_TURNS = (np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0]))


def random_rotations(n, seed):
    """n rotation matrices from normalised Gaussian quaternions (float64 [n,3,3])."""
    q = np.random.default_rng(seed).normal(size=(n, 4))
    return hierarchy._rot_from_quat(q / np.linalg.norm(q, axis=1, keepdims=True))


def signed_permutations():
    """The 24 proper signed permutation matrices (float64), the identity first."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for k in range(3):
                m[perm[k], k] = signs[k]
            if np.linalg.det(m) > 0:
                out.append(m)
    assert len(out) == 24 and np.array_equal(out[0], np.eye(3))
    return out


def general():
    return hierarchy.similarity(R=random_rotations(1, 11)[0], scale=1.7, translate=T_GENERAL)


def ulp32(x):
    """The float32 spacing at magnitude |x| (numpy float64 array in, float64 out)."""
    a = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


# ---- 1. the SH convention ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", (0, 1, 2, 3))
def test_rotated_coefficients_give_the_colour_of_the_rotated_direction(deg):
    rng = np.random.default_rng(deg)
    M = (deg + 1) ** 2
    worst = 0.0
    for R in list(random_rotations(20, 3)) + signed_permutations():
        sim = hierarchy.similarity(R=R)
        c = rng.normal(size=(40, M, 3))
        d = rng.normal(size=(40, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        z3, z4 = np.zeros((40, 3)), np.ones((40, 4))
        _, c2, _, _ = hierarchy.transform_rows(sim, z3, c, z3, z4, round32=False)
        assert c2.dtype == np.float64 and np.array_equal(c2[:, 0], c[:, 0])
        a = ro.eval_sh_torch(deg, torch.from_numpy(c2), torch.from_numpy(d @ R.T))
        b = ro.eval_sh_torch(deg, torch.from_numpy(c), torch.from_numpy(d))
        worst = max(worst, float((a - b).abs().max()))
        for D in (sim.D1, sim.D2, sim.D3):
            assert np.abs(D @ D.T - np.eye(D.shape[0])).max() <= 1e-13
    print(f"degree {deg}: colour invariance max |d| = {worst:.3g}")
    assert worst <= 1e-12


def test_band_one_is_the_closed_form():
    A = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])      # (x,y,z) -> (-y, z, -x)
    for R in list(random_rotations(20, 4)) + signed_permutations():
        D1 = hierarchy.similarity(R=R).D1
        assert np.abs(D1 - A @ R @ A.T).max() <= 1e-13
    for R in signed_permutations():                   # ... exactly so for the signed permutations, in every band
        sim = hierarchy.similarity(R=R)
        assert np.array_equal(sim.D1, A @ R @ A.T)
    ident = hierarchy.similarity()
    assert np.array_equal(ident.q_R, [1.0, 0.0, 0.0, 0.0]) and ident.log_s == 0.0
    assert all(np.array_equal(D, np.eye(D.shape[0])) for D in (ident.D1, ident.D2, ident.D3))


# ---- 2. the Gaussians ----------------------------------------------------------------------------------------------------
def covariances(log_scales, rots):
    q = np.asarray(rots, dtype=np.float64)
    Rm = hierarchy._rot_from_quat(q / np.linalg.norm(q, axis=1, keepdims=True))
    S2 = np.exp(np.asarray(log_scales, dtype=np.float64)) ** 2
    return np.einsum("nij,nj,nkj->nik", Rm, S2, Rm)


def test_covariances_follow_the_map():
    h, _ = scene2000()
    sim = general()
    t = hierarchy.transform_hierarchy(h, sim)
    assert all(getattr(t, k).dtype == getattr(h, k).dtype and getattr(t, k).shape == getattr(h, k).shape for k in ARRAYS)
    want = sim.s ** 2 * np.einsum("ij,njk,lk->nil", sim.R, covariances(h.log_scales.numpy(), h.rots.numpy()), sim.R)
    got = covariances(t.log_scales.numpy(), t.rots.numpy())
    rel = np.linalg.norm(got - want, axis=(1, 2)) / np.linalg.norm(want, axis=(1, 2))
    print(f"covariance: max relative Frobenius error {rel.max():.3g}")
    assert rel.max() <= 1e-6
    x = sim.apply(h.xyz.numpy().astype(np.float64))
    assert np.abs(t.xyz.numpy() - x).max() <= 0.5 * ulp32(x).max()
    assert torch.equal(bits(t.alpha), bits(h.alpha)) and torch.equal(t.nodes, h.nodes)
    # quaternion norms are kept, not renormalised
    n0, n1 = np.linalg.norm(h.rots.numpy().astype(np.float64), axis=1), np.linalg.norm(t.rots.numpy().astype(np.float64), axis=1)
    assert np.abs(n1 - n0).max() <= 2e-7 * n0.max()


# ---- 3. the identity, the alignment dots ---------------------------------------------------------------------------------
def test_the_identity_is_bit_exact_and_alignment_dots_survive():
    h, _ = scene2000()
    t = hierarchy.transform_hierarchy(h, hierarchy.similarity())
    for k in ARRAYS:
        assert torch.equal(bits(getattr(t, k)), bits(getattr(h, k))), k
    for sim in (hierarchy.similarity(quat=(1.0, 0.0, 0.0, 0.0)), hierarchy.similarity(R=np.eye(3), scale=1.0)):
        assert torch.equal(bits(hierarchy.transform_hierarchy(h, sim).shs), bits(h.shs))
    aligned = hierarchy.align_hierarchy(h)
    moved = hierarchy.transform_hierarchy(aligned, general())
    d0, d1 = hierarchy.alignment_dots(aligned), hierarchy.alignment_dots(moved)
    assert d0.size == h.num_nodes - 1 and np.abs(d1 - d0).max() <= 1e-6


# ---- 4. composition and inverse ----------------------------------------------------------------------------------------
def rows64(sim, h):
    """The row rule in float64 without the rounding to float32."""
    G = h.xyz.shape[0]
    return hierarchy.transform_rows(sim, h.xyz.numpy(), h.shs.numpy().reshape(G, -1, 3), h.log_scales.numpy(),
                                    h.rots.numpy(), round32=False)


def assert_within_4_ulp(name, got, want64, mid64, scale_mid):
    """|got - want64| <= 4 float32 ulp of the larger magnitude, per element.  What feeds an element is its whole vector
    (a rotation mixes the coordinates of a mean, the components of a quaternion, the coefficients of one band and
    channel), at the intermediate stage and at the final one: the rounding between the two steps is half an ulp of the
    intermediate vector's largest entry per entry, an orthogonal block turns that into at most sqrt(7)/2 ulp in any
    one entry, the second map's scale moves value and spacing together up to a factor 2 of the float32 grid, and the
    final rounding adds half an ulp: below 4.  ``mid64``: the intermediate values, ``scale_mid``: the factor that
    brings them into output units; both vectors reduced over ``axis`` = the mixed axis."""
    mag = np.maximum(np.abs(want64).max(axis=-1, keepdims=True), scale_mid * np.abs(mid64).max(axis=-1, keepdims=True))
    err = np.abs(got.astype(np.float64) - want64) / ulp32(np.broadcast_to(mag, want64.shape))
    print(f"{name}: worst error {err.max():.3g} ulp of the larger magnitude")
    assert err.max() <= 4.0, name


def band_view(c):
    """[G,M,3] -> per band a view [G,3,2l+1] (the mixed axis last)."""
    M = c.shape[1]
    return [np.swapaxes(c[:, l * l:(l + 1) ** 2, :], 1, 2) for l in range(4) if (l + 1) ** 2 <= M]


@pytest.mark.parametrize("case", ("a_then_b", "a_then_its_inverse"))
def test_compose_and_inverse_agree_with_two_applications(case):
    h, _ = scene2000()
    G = h.xyz.shape[0]
    a = general()
    b = a.inverse() if case == "a_then_its_inverse" else hierarchy.similarity(R=random_rotations(1, 12)[0], scale=0.6,
                                                                              translate=(-1.0, 4.0, 2.5))
    ba = b.compose(a)
    assert np.abs(ba.apply(h.xyz.numpy()) - b.apply(a.apply(h.xyz.numpy()))).max() <= 1e-12
    if case == "a_then_its_inverse":
        assert np.abs(ba.R - np.eye(3)).max() <= 1e-14 and abs(ba.s - 1.0) <= 1e-14 and np.abs(ba.t).max() <= 1e-14
    two = hierarchy.transform_hierarchy(hierarchy.transform_hierarchy(h, a), b)
    mid = rows64(a, h)
    want = rows64(ba, h)
    # the composed quaternion may be the negative of q_b (x) q_a: the same rotation
    sign = np.sign(np.dot(hierarchy._quat_mul(b.q_R, a.q_R), ba.q_R))
    assert abs(abs(np.dot(hierarchy._quat_mul(b.q_R, a.q_R), ba.q_R)) - 1.0) <= 1e-12
    assert_within_4_ulp("xyz", two.xyz.numpy(), want[0], mid[0], b.s)
    assert_within_4_ulp("rots", two.rots.numpy(), sign * want[3], mid[3], 1.0)
    assert_within_4_ulp("log_scales", two.log_scales.numpy()[..., None], want[2][..., None], mid[2][..., None], 1.0)
    for l, (g, w, m) in enumerate(zip(band_view(two.shs.numpy().reshape(G, -1, 3)), band_view(want[1]), band_view(mid[1]))):
        assert_within_4_ulp(f"shs band {l}", g, w, m, 1.0)
    # boxes do not compose: the box of a rotated box of a rotated box contains the box of the composed rotation
    one = hierarchy.transform_boxes(ba, h.boxes.numpy())
    tol = 4.0 * ulp32(np.abs(two.boxes.numpy()[:, :, :3]).max(axis=(1, 2)))[:, None]
    assert (two.boxes.numpy()[:, 0, :3] <= one[:, 0, :3] + tol).all() and (two.boxes.numpy()[:, 1, :3] >= one[:, 1, :3] - tol).all()


# ---- 5. the boxes ------------------------------------------------------------------------------------------------------
def test_nesting_survives_rounding_exactly():
    h, _ = scene2000()
    parent = h.nodes[1:, 1].numpy()
    b0 = h.boxes.numpy()
    assert (b0[parent, 0, :3] <= b0[1:, 0, :3]).all() and (b0[1:, 1, :3] <= b0[parent, 1, :3]).all()
    for k, R in enumerate(random_rotations(5, 21)):
        sim = hierarchy.similarity(R=R, scale=(0.37, 1.0, 1.7, 12.5, 3.0)[k], translate=(0.1 * k, -7.3, 100.0 * k))
        b = hierarchy.transform_boxes(sim, b0)
        assert (b[parent, 0, :3] <= b[1:, 0, :3]).all() and (b[1:, 1, :3] <= b[parent, 1, :3]).all(), k
        assert (b[:, 0, :3] <= b[:, 1, :3]).all()
        e = b[:, 1, :3] - b[:, 0, :3]
        assert np.array_equal(b[:, 0, 3], e.max(1)) and np.array_equal(b[:, 1, 3].view(np.uint32), b0[:, 1, 3].view(np.uint32))
        # the corners of the old box lie in the new one (up to the rounding of the new one), and it grew by <= sqrt 3
        lo_, hi_ = b0[:, 0, :3].astype(np.float64), b0[:, 1, :3].astype(np.float64)
        slack = ulp32(np.abs(b[:, :, :3]).max(axis=(1, 2)))[:, None]
        for corner in itertools.product((0, 1), repeat=3):
            p = sim.apply(np.where(np.array(corner)[None, :] == 1, hi_, lo_))
            assert (p >= b[:, 0, :3] - slack).all() and (p <= b[:, 1, :3] + slack).all()
        assert (b[:, 0, 3] <= np.float32(1.7320509) * np.float32(sim.s) * b0[:, 0, 3] * np.float32(1.00001) + slack[:, 0]).all()


@pytest.mark.parametrize("s", (0.5, 4.0))
def test_signed_permutations_permute_the_boxes_bit_for_bit(s):
    h, _ = scene2000()
    b0 = h.boxes.numpy()
    for R in signed_permutations():
        b = hierarchy.transform_boxes(hierarchy.similarity(R=R, scale=s), b0)
        want = b0.copy()
        for a in range(3):
            k = int(np.nonzero(R[a])[0][0])
            lo_, hi_ = (b0[:, 0, k], b0[:, 1, k]) if R[a, k] > 0 else (-b0[:, 1, k], -b0[:, 0, k])
            want[:, 0, a], want[:, 1, a] = np.float32(s) * lo_, np.float32(s) * hi_
        want[:, 0, 3] = (want[:, 1, :3] - want[:, 0, :3]).max(1)
        assert np.array_equal(b.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(b[:, 0, 3], np.float32(s) * b0[:, 0, 3])


# ---- 6. the cut under half-turns -----------------------------------------------------------------------------------------
def oracle_cut(nodes, boxes, tau, v):
    ri, pi, ni = lo.expand_to_size(nodes, boxes, tau, v)
    w, kids = lo.get_interpolation_weights(ni, tau, nodes, boxes, v)
    return ri, pi, ni, w, kids


@functools.lru_cache(maxsize=None)
def original_cuts():
    h, _ = scene2000()
    nd, bx = h.nodes.numpy(), h.boxes.numpy()
    return {(v, tau): oracle_cut(nd, bx, tau, v) for v in VIEWS for tau in (0.005, 0.02, 0.1)}


@pytest.mark.parametrize("s", (0.5, 1.0, 2.0))
@pytest.mark.parametrize("turn", range(3))
def test_the_cut_of_a_half_turned_hierarchy_is_the_originals(turn, s):
    h, _ = scene2000()
    sim = hierarchy.similarity(R=HALF_TURNS[turn], scale=s)
    t = hierarchy.transform_hierarchy(h, sim)
    nd, bx = t.nodes.numpy(), t.boxes.numpy()
    sizes = []
    for (v, tau), want in original_cuts().items():
        v2 = sim.apply(np.asarray(v))
        assert np.array_equal(v2, v2.astype(np.float32).astype(np.float64))          # the viewpoint moves exactly
        got = oracle_cut(nd, bx, tau, tuple(float(x) for x in v2))
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (v, tau, k)
        assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32)) and np.array_equal(got[4], want[4])
        sizes.append(len(got[0]))
    assert len(sizes) == 9 and min(sizes) > 0 and sizes[-1] == 981


# ---- 7. a render of the float64 oracle ---------------------------------------------------------------------------------
RENDER_CAM = synth.make_camera(96, 64)


@functools.lru_cache(maxsize=None)
def render_rows():
    """600 trained-like Gaussians as trained rows (xyz, shs, alpha, log_scales, rots), float32 numpy."""
    sc = synth.make_scene_trained_like(600, RENDER_CAM, seed=3)
    return (sc.means3D.numpy(), sc.shs.numpy(), sc.opacities.numpy(), torch.log(sc.scales).numpy(), sc.rotations.numpy())


def oracle_render(rows, cam):
    xyz, shs, alpha, ls, rots = (torch.from_numpy(np.ascontiguousarray(r)) for r in rows)
    out = ro.rasterize(xyz, torch.zeros(xyz.shape[0], 3), shs, None, alpha, torch.exp(ls),
                       torch.nn.functional.normalize(rots), None, image_height=cam.image_height,
                       image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3),
                       scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
                       sh_degree=3, campos=cam.camera_center, dtype=torch.float64)
    return out.color.detach()


@functools.lru_cache(maxsize=None)
def original_render():
    return oracle_render(render_rows(), RENDER_CAM)


@pytest.mark.parametrize("seed", (31, 32, 33))
def test_the_oracle_renders_the_moved_scene_from_the_moved_camera_alike(seed):
    """Measured: max |d| = 2.7e-6, 4.0e-6, 2.0e-6 for the three rotations against an image maximum of 0.78 (the float32
    rounding of the moved rows and of the moved camera's matrices); the bound, 2e-5, is about three times the worst of the three
    measurements taken when the check was set (1.2e-6 to 5.9e-6)."""
    xyz, shs, alpha, ls, rots = render_rows()
    sim = hierarchy.similarity(R=random_rotations(1, seed)[0], scale=1.0, translate=T_GENERAL)
    x2, c2, l2, q2 = hierarchy.transform_rows(sim, xyz, shs, ls, rots)
    assert all(v.dtype == np.float32 for v in (x2, c2, l2, q2))
    a = original_render()
    b = oracle_render((x2, c2, alpha, l2, q2), hierarchy.transform_camera(RENDER_CAM, sim))
    d = float((a - b).abs().max())
    print(f"render invariance, rotation {seed}: max |d| = {d:.3g}, image maximum {float(a.max()):.3g}")
    assert float(a.max()) > 0.5 and d <= 2e-5
    # moving the rows alone (the old camera) is another image: the check can fail
    assert float((a - oracle_render((x2, c2, alpha, l2, q2), RENDER_CAM)).abs().max()) > 1e-2


def test_transform_camera():
    sim = general()
    cam = synth.make_camera(64, 48, R=random_rotations(1, 5)[0], T=(0.3, -0.2, 1.5))
    moved = hierarchy.transform_camera(cam, sim)
    assert moved is not cam and moved.image_width == 64 and moved.world_view_transform.dtype == torch.float32
    p = np.random.default_rng(2).normal(size=(30, 3)) * 5
    ph = np.concatenate([p, np.ones((30, 1))], 1)
    ph2 = np.concatenate([sim.apply(p), np.ones((30, 1))], 1)
    for name in ("world_view_transform", "full_proj_transform"):
        a, b = ph @ getattr(cam, name).double().numpy(), ph2 @ getattr(moved, name).double().numpy()
        assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max(), name
    assert np.abs(moved.camera_center.double().numpy() - sim.apply(cam.camera_center.double().numpy())).max() <= 1e-6
    back = hierarchy.transform_camera(moved, sim.inverse())
    assert (back.world_view_transform - cam.world_view_transform).abs().max() <= 1e-5


# ---- 8. rejections -------------------------------------------------------------------------------------------------------
def test_the_spec_refuses_what_is_not_a_similarity():
    R = random_rotations(1, 6)[0]
    with pytest.raises(ValueError, match="orthonormal"):
        hierarchy.similarity(R=R + 1e-6)
    with pytest.raises(ValueError, match="orthonormal"):
        hierarchy.similarity(R=np.diag([1.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="mirror"):
        hierarchy.similarity(R=np.diag([1.0, 1.0, -1.0]))
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale"):
            hierarchy.similarity(R=R, scale=s)
    with pytest.raises(ValueError, match="translate"):
        hierarchy.similarity(R=R, translate=(0.0, float("nan"), 0.0))
    with pytest.raises(ValueError):
        hierarchy.similarity(quat=(0.0, 0.0, 0.0, 0.0))
    h, _ = scene2000()
    two = hierarchy.Hierarchy(h.xyz, h.shs[:, :2].contiguous(), h.alpha, h.log_scales, h.rots, h.nodes, h.boxes)
    with pytest.raises(ValueError, match="whole bands"):
        hierarchy.transform_hierarchy(two, general())
    bad = copy.copy(general())
    bad.D2 = hierarchy.similarity(R=random_rotations(1, 7)[0]).D2
    with pytest.raises(ValueError, match="D2 is not the SH block of R"):
        hierarchy.transform_hierarchy(h, bad)


def _view(N=5, G=None, M=16, base=4096, **at):
    a = {k: base for k in ARRAYS}
    a.update(at)
    return _lib.HierView(N if G is None else G, N, M, 0, *(a[k] for k in ARRAYS))


def _with(sim, **fields):
    out = copy.copy(sim)
    for k, v in fields.items():
        setattr(out, k, v)
    return out


def bad_parameter_blocks():
    """(name, Similarity that must be refused, a word of the message)."""
    g = general()
    other = hierarchy.similarity(R=random_rotations(1, 7)[0])
    skew = g.R.copy()
    skew[0, 1] += 1e-6
    nan_t = g.t.copy()
    nan_t[1] = float("nan")
    mirror = np.diag([1.0, 1.0, -1.0])
    return [("non-orthonormal R", _with(g, R=skew), b"orthonormal"),
            ("det -1", _with(hierarchy.similarity(), R=mirror), b"mirror"),
            ("s = 0", _with(g, s=0.0, log_s=0.0), b"s > 0"), ("s = -1", _with(g, s=-1.0, log_s=0.0), b"s > 0"),
            ("s = nan", _with(g, s=float("nan")), b"s > 0"), ("s = inf", _with(g, s=float("inf"), log_s=float("inf")), b"s > 0"),
            ("nan t", _with(g, t=nan_t), b"finite"), ("log_s", _with(g, log_s=g.log_s + 1e-9), b"log_s"),
            ("q of another rotation", _with(g, q_R=other.q_R), b"q does not reproduce R"),
            ("D2 of another rotation", _with(g, D2=other.D2), b"D2 is not the SH block of R"),
            ("D1 of another rotation", _with(g, D1=other.D1), b"D1 is not the SH block of R"),
            ("D3 not orthogonal", _with(g, D3=g.D3 * 1.001), b"D3 is not orthogonal")]


def test_the_c_checks_refuse_the_same_before_any_hip_call():
    """(Host only: every call here is refused before a HIP call; HGS_ERR_INVALID = 1, a HIP failure would be 2.)"""
    lib = _lib.lib()
    good = hierarchy.transform_args(general())
    call = lambda vi, vo, a: lib.hgs_hier_transform(C.byref(vi), C.byref(vo), C.byref(a), None, 0)
    for name, sim, word in bad_parameter_blocks():
        assert call(_view(), _view(), hierarchy.transform_args(sim)) == 1, name
        assert word in lib.hgs_last_error(), (name, lib.hgs_last_error())
        with pytest.raises(ValueError):
            hierarchy.check_similarity(sim)
    a = 4096
    sizes = [((_view(M=2), _view(M=2)), b"whole SH bands"), ((_view(M=3), _view(M=3)), b"whole SH bands"),
             ((_view(0), _view(0)), b"bad sizes"), ((_view(1 << 31), _view(1 << 31)), b"bad sizes"),
             ((_view(5, G=1 << 31), _view(5, G=1 << 31)), b"bad sizes"), ((_view(5, G=4), _view(5, G=4)), b"bad sizes"),
             ((_view(5), _view(5, G=6)), b"bad sizes"), ((_view(5), _view(4)), b"bad sizes"), ((_view(5), _view(5, M=4)), b"bad sizes"),
             ((_view(5, xyz=0), _view(5)), b"null"), ((_view(5), _view(5, shs=0)), b"null"),
             ((_view(5, rots=a + 8), _view(5)), b"16-byte"), ((_view(5), _view(5, boxes=a + 4)), b"16-byte"),
             ((_view(5, alpha=a + 2), _view(5)), b"4-byte"), ((_view(5), _view(5, shs=a + 16)), b"overlaps"),
             ((_view(5), _view(5, boxes=a + 5 * 32 - 16)), b"overlaps"), ((_view(5, xyz=a + 56), _view(5)), b"overlaps")]
    for (vi, vo), word in sizes:
        assert call(vi, vo, good) == 1, word
        assert word in lib.hgs_last_error(), (word, lib.hgs_last_error())
    assert lib.hgs_hier_transform(None, C.byref(_view()), C.byref(good), None, 0) == 1
    assert lib.hgs_hier_transform(C.byref(_view()), C.byref(_view()), None, None, 0) == 1
    hierarchy.check_similarity(general())


def test_the_abi_declares_and_binds_the_entry():
    plain = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bhgs_hier_transform\s*\(", plain)
    assert "hgs_hier_transform" in _lib.SIGNATURES and hasattr(_lib.lib(), "hgs_hier_transform")
    assert re.search(r"#define\s+HGS_ABI_VERSION\s+14\b", HEADER) and _lib.ABI_VERSION == 14
    body = re.search(r"typedef struct hgs_hier_transform_args \{(.*?)\} hgs_hier_transform_args;", HEADER, flags=re.S).group(1)
    fields = re.findall(r"double\s+(\w+)(?:\[(\d+)\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [(n, int(c or 1)) for n, c in fields] == [(n, C.sizeof(t) // 8) for n, t in _lib.HierTransformArgs._fields_]
    assert C.sizeof(_lib.HierTransformArgs) == 8 * 101
    a = hierarchy.transform_args(general())
    assert list(a.D3) == list(general().D3.reshape(-1)) and a.log_s == general().log_s


# ---- 9. the command ------------------------------------------------------------------------------------------------------
def test_the_command_parses_its_arguments(capsys):
    p = cmd.parse_args
    r = p(["a.hier", "b.hier", "--scale", "2", "--translate", "1", "-2", "3"])
    assert (r["in_path"], r["out_path"], r["scale"], r["translate"], r["quat"], r["R"], r["invert"], r["half"]) == \
        ("a.hier", "b.hier", 2.0, [1.0, -2.0, 3.0], None, None, False, False)
    r = p(["--quat", "0", "0", "0", "2", "a.hier", "--invert", "b.hier", "--half"])
    assert r["quat"] == [0.0, 0.0, 0.0, 2.0] and r["invert"] and r["half"] and r["scale"] == 1.0
    sim = cmd.build_similarity(r)
    assert np.abs(sim.R - np.diag([-1.0, -1.0, 1.0])).max() <= 1e-15
    r = p(["a.hier", "b.hier", "--axis-angle", "0", "0", "3", "90"])
    assert np.abs(cmd.build_similarity(r).R - np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])).max() <= 1e-15
    g = general()
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = g.s * g.R, g.t
    r = p(["a.hier", "b.hier", "--matrix"] + [repr(float(x)) for x in m.reshape(-1)])
    got = cmd.build_similarity(r)
    assert np.abs(got.R - g.R).max() <= 1e-12 and abs(got.s - g.s) <= 1e-12 and np.abs(got.t - g.t).max() == 0.0
    inv = cmd.build_similarity(dict(r, invert=True))
    assert np.abs(inv.apply(g.apply(np.array([[1.0, 2.0, 3.0]]))) - [1.0, 2.0, 3.0]).max() <= 1e-12
    bad = ([], ["a.hier"], ["a.hier", "b.hier"], ["a.hier", "b.hier", "--invert"], ["a.hier", "b.hier", "c.hier", "--scale", "2"],
           ["a.hier", "b.hier", "--scale"], ["a.hier", "b.hier", "--scale", "0"], ["a.hier", "b.hier", "--scale", "-1"],
           ["a.hier", "b.hier", "--scale", "nan"], ["a.hier", "b.hier", "--scale", "inf"], ["a.hier", "b.hier", "--scale", "big"],
           ["a.hier", "b.hier", "--quat", "1", "0", "0"], ["a.hier", "b.hier", "--quat", "0", "0", "0", "0"],
           ["a.hier", "b.hier", "--quat", "1", "0", "0", "0", "--axis-angle", "0", "0", "1", "90"],
           ["a.hier", "b.hier", "--axis-angle", "0", "0", "0", "90"], ["a.hier", "b.hier", "--translate", "1", "2", "nan"],
           ["a.hier", "b.hier", "--matrix", "1", "0", "0"], ["a.hier", "b.hier", "--frobnicate"],
           ["a.hier", "b.hier", "--scale", "2", "--matrix"] + ["1"] * 16)
    for argv in bad:
        assert p(argv) is None, argv
        assert cmd.main(argv) == 2, argv
    assert "usage: python -m hgs.transform_hierarchy" in capsys.readouterr().err
    # a --matrix that is no similarity is refused and named
    shear, mirror, proj = np.eye(4), np.eye(4), np.eye(4)
    shear[0, 1], mirror[2, 2], proj[3, 0] = 0.1, -1.0, 0.5
    for mat, word in ((shear, "shear"), (mirror, "mirror"), (proj, "projective"), (np.diag([1.0, 2.0, 1.0, 1.0]), "non-uniform")):
        argv = ["a.hier", "b.hier", "--matrix"] + [str(x) for x in mat.reshape(-1)]
        with pytest.raises(cmd.NotASimilarity, match=word):
            p(argv)
        assert cmd.main(argv) == 2
        assert word in capsys.readouterr().err
    assert cmd.main(["/nonexistent/in.hier", "out.hier", "--scale", "2"]) == 2
    assert "does not exist" in capsys.readouterr().err
