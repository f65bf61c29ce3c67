"""K1's half-row LOD route (csrc/preprocess.hip: preprocess_fwd_lod_half_kernel; hgs_raster_args.lod_half_rows) on
hand-built cuts, through the Python op.  The attribute arrays hold G = 300 rows of half BIT PATTERNS
(half_rows_cases.half_pattern_rows: normal values of both signs, subnormals, +-65504, -0.0); the reference is the same
call on float32 arrays that hold the exact widening of those bits (half_rows_cases.widen: a table from the format's
definition).  Widening is exact and everything behind it is the float32 route, so colour, inverse depth and radii must
agree bit for bit -- at every entry count around a wave and K1's 256-row workgroup, at SH widths that take the
cooperative gather (6 M % 16 == 0: M = 8 and 16) and the per-lane one, with and without skybox rows.  Then the refusals: every
other use of a float16 tensor raises, and the C ABI answers HGS_ERR_INVALID with the reason."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import half_rows_cases as hc
import parity as pa
from hgs import _lib, synth

pytestmark = pytest.mark.gpu

G = 300
W, H = 64, 48
POISON = np.arange(280, 290)              # rows that only ever serve as the parent of a weight-1 entry
PLAIN = np.arange(270, 280)               # rows of ordinary values (an opaque splat a few pixels wide): something is drawn at every n
ENTRIES = [1, 63, 64, 256, 257, 515]      # one lane, a wave's edge, K1's 256-row workgroup edge, two workgroups + a partial wave
WIDTHS = [1, 4, 8, 9, 16]                 # 6 M % 16 == 0 at M = 8 and 16: the cooperative SH gather; per lane at the others
DEGREE = {1: 0, 4: 1, 8: 1, 9: 2, 16: 3}
ERR_INVALID = 1


@functools.lru_cache(maxsize=None)
def _arrays(M, poison):
    """(half bits, means): uint16 arrays shs [G, M, 3], opacities [G, 1], scales [G, 3], rotations [G, 4] cut from the
    pattern rows; float32 means in front of the camera.  Some rows' rotation is the negated rotation of the row before
    (a parent in the opposite hemisphere whatever the pattern).  ``poison``: rows POISON hold NaN / infinity in every
    field, the mean included; else zeros.  Rows PLAIN are ordinary splats -- DC coefficient 1, opacity 0.9, scale 0.5,
    identity rotation -- so that the image is not the background even when the cut is one entry.  Computed once per
    (M, poison), never modified."""
    rows, _ = hc.half_pattern_rows(G, M)
    halves = rows[:, :112].view(np.uint16)
    bits = dict(shs=halves[:, :3 * M].reshape(G, M, 3).copy(), opacities=halves[:, 55:56].copy(),
                scales=halves[:, 52:55].copy(), rotations=halves[:, 48:52].copy())
    bits["rotations"][1::7] = bits["rotations"][0:-1:7][:len(bits["rotations"][1::7])] ^ 0x8000
    means = synth.make_scene(G, synth.make_camera(W, H), seed=3).means3D.numpy().astype(np.float32).copy()
    for k in bits:
        flat = bits[k].reshape(G, -1)
        flat[POISON] = np.where(np.arange(flat.shape[1])[None, :] % 2 == 0, 0x7E00, 0xFC00) if poison else 0
    means[POISON] = np.nan if poison else 0.0
    bits["shs"][PLAIN, 0] = 0x3C00                                 # 1.0
    bits["opacities"][PLAIN] = 0x3B33                              # 0.9
    bits["scales"][PLAIN] = 0x3800                                 # 0.5
    bits["rotations"][PLAIN] = np.array([0x3C00, 0, 0, 0], np.uint16)
    edge = np.concatenate([b[:280].reshape(-1) for b in bits.values()])
    assert (edge == 0x8000).any() and (edge == 0x7BFF).any() and (edge == 0xFBFF).any() and ((edge & 0x7FFF) < 0x0400).any()
    return bits, means


def _cut(n, seed):
    """n entries over rows [0, 280): weights exactly 1, exactly 0 and fractions; every fourth weight-1 entry names a
    POISON row as its parent; every sixteenth entry -- the first among them -- draws a PLAIN row."""
    rng = np.random.default_rng(seed)
    ri = rng.integers(0, 270, n).astype(np.int32)
    pi = rng.integers(0, 280, n).astype(np.int32)
    ri[::16] = rng.choice(PLAIN, len(ri[::16]))
    w = rng.choice(np.array([1.0, 1.0, 0.0, 0.25, 0.5, 0.999999], np.float32), n).astype(np.float32)
    w[0] = 1.0
    if n >= 63:
        w[1], w[2], w[3] = 0.0, 0.5, 1.0
        ri[4], pi[4], w[4] = 0, 1, 0.5                             # rows 0 / 1: the negated quaternion as the parent
    one = np.nonzero(w == 1.0)[0][::4]
    pi[one] = rng.choice(POISON, len(one))
    kids = rng.integers(1, 5, n).astype(np.int32)
    return ri, pi, w, kids


def _tensors(gpu, M, poison, half):
    bits, means = _arrays(M, poison)
    out = dict(means3D=torch.from_numpy(means).to(gpu))
    for k, b in bits.items():
        if half:
            out[k] = torch.from_numpy(b.view(np.int16)).to(gpu).view(torch.float16)
        else:
            out[k] = torch.from_numpy(hc.widen(b)).to(gpu)
    return out


def _render(gpu, arrays, cut, M, K, **over):
    import diff_gaussian_rasterization as dgr
    ri, pi, w, kids = (torch.from_numpy(x).to(gpu) for x in cut)
    cam = synth.make_camera(W, H)
    kw = pa.settings_kwargs(cam, torch.tensor([0.1, 0.2, 0.3]), DEGREE[M], do_depth=True, device=gpu,
                            interpolation_weights=w, num_node_kids=kids)
    kw.update(render_indices=ri, parent_indices=pi)
    rs = dgr.GaussianRasterizationSettings(**kw)
    a = dict(arrays, **over)
    with torch.no_grad():
        color, radii, invdepth = dgr.GaussianRasterizer(rs, context=dgr.RasterContext(skybox_points=K))(
            means3D=a["means3D"], means2D=torch.zeros(G, 3, device=gpu), shs=a["shs"], opacities=a["opacities"],
            scales=a["scales"], rotations=a["rotations"])
    assert radii.numel() == len(cut[0]) + K
    return color, invdepth, radii


def _same(x, y, what):
    for a, b, name in zip(x, y, ("colour", "inverse depth", "radii")):
        ia, ib = (t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t for t in (a, b))
        bad = torch.nonzero(ia != ib)
        assert bad.numel() == 0, f"{what}: {name} differs at {bad[:4].tolist()}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}"


@pytest.mark.parametrize("K", [0, 3], ids=["no_skybox", "skybox3"])
@pytest.mark.parametrize("M", WIDTHS)
@pytest.mark.parametrize("n", ENTRIES)
def test_half_rows_render_the_bits_of_the_widened_float_rows(gpu, n, M, K):
    cut = _cut(n, seed=10 * n + M)
    half = _render(gpu, _tensors(gpu, M, True, True), cut, M, K)
    flt = _render(gpu, _tensors(gpu, M, True, False), cut, M, K)
    _same(half, flt, f"n={n} M={M} K={K}")
    color, _, radii = half
    bg = torch.tensor([0.1, 0.2, 0.3], device=gpu).view(3, 1, 1)
    assert bool(((color - bg).abs() > 1e-3).any()) and bool((color > 0).any()), "nothing was drawn"
    assert int((radii > 0).sum()) >= 1, "no row is visible: the case shows nothing"
    if (6 * M) % 16 == 0 and n >= 256:
        # K1 takes the cooperative gather (coop_gather_sh_half) in a workgroup with at least half of its 256 rows visible
        assert int((radii[:256] > 0).sum()) >= 128, "the first workgroup took the per-lane route: the cooperative one did not run"


@pytest.mark.parametrize("M", WIDTHS)
def test_a_non_finite_parent_under_weight_one_does_not_reach_the_pixel(gpu, M):
    """The weight-1 rule on the half route: rows that only serve as parents of weight-1 entries hold NaN and infinities
    in one set of arrays and zeros in the other -- the images are the same bits."""
    n, K = 257, 3
    cut = _cut(n, seed=99 + M)
    assert np.isin(cut[1][cut[2] == 1.0], POISON).sum() >= 10 and not np.isin(cut[0], POISON).any()
    assert not np.isin(cut[1][cut[2] != 1.0], POISON).any()
    poisoned = _render(gpu, _tensors(gpu, M, True, True), cut, M, K)
    clean = _render(gpu, _tensors(gpu, M, False, True), cut, M, K)
    _same(poisoned, clean, f"M={M}")
    assert bool(torch.isfinite(poisoned[0]).all())


def test_per_pixel_remap(gpu):
    """LOD_REMAP = "alpha": the compositing kernels remap alpha; K1 leaves the opacity alone -- on both routes."""
    from diff_gaussian_rasterization import _C as dc
    n, M, K = 257, 16, 3
    cut = _cut(n, seed=5)
    old = dc.LOD_REMAP
    try:
        dc.LOD_REMAP = "alpha"
        half = _render(gpu, _tensors(gpu, M, True, True), cut, M, K)
        flt = _render(gpu, _tensors(gpu, M, True, False), cut, M, K)
    finally:
        dc.LOD_REMAP = old
    _same(half, flt, "per-pixel remap")
    per_gaussian = _render(gpu, _tensors(gpu, M, True, True), cut, M, K)
    assert not torch.equal(half[0], per_gaussian[0]), "the per-pixel remap changed nothing: the flag did not arrive"


# ===================================================================================================================
# refusals
# ===================================================================================================================
def test_every_other_use_of_a_half_tensor_raises(gpu):
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C as dc
    M, K = 4, 0
    cut = _cut(64, seed=1)
    h, f = _tensors(gpu, M, False, True), _tensors(gpu, M, False, False)
    msg = "ONE use: the in-op LOD interpolation"
    for k in ("shs", "opacities", "scales", "rotations"):                              # a mix of dtypes, either way round
        with pytest.raises(RuntimeError, match=msg):
            _render(gpu, h, cut, M, K, **{k: f[k]})
        with pytest.raises(RuntimeError, match=msg):
            _render(gpu, f, cut, M, K, **{k: h[k]})
    with pytest.raises(RuntimeError, match=msg):
        _render(gpu, h, cut, M, K, means3D=h["means3D"].half())
    # half without render_indices
    cam = synth.make_camera(W, H)
    rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(cam, torch.zeros(3), 1, device=gpu))
    call = dict(means3D=h["means3D"], means2D=torch.zeros(G, 3, device=gpu), shs=h["shs"], opacities=h["opacities"],
                scales=h["scales"], rotations=h["rotations"])
    with pytest.raises(RuntimeError, match=msg):
        dgr.GaussianRasterizer(rs)(**call)
    # half with an input that requires a gradient (the attributes, or the float32 mean)
    ri, pi, w, kids = (torch.from_numpy(x).to(gpu) for x in cut)
    kw = pa.settings_kwargs(cam, torch.zeros(3), 1, device=gpu, interpolation_weights=w, num_node_kids=kids)
    kw.update(render_indices=ri, parent_indices=pi)
    lod_rs = dgr.GaussianRasterizationSettings(**kw)
    for k in ("means3D", "shs"):
        with pytest.raises(RuntimeError, match="requires a gradient"):
            dgr.GaussianRasterizer(lod_rs)(**dict(call, **{k: call[k].clone().requires_grad_(True)}))
    # the raw-parameter path
    with pytest.raises(RuntimeError, match=msg):
        dgr.GaussianRasterizer(rs).forward_raw(h["means3D"], call["means2D"], h["shs"][:, :1], h["shs"][:, 1:],
                                               h["opacities"], h["scales"], h["rotations"])
    # the stand-alone gather stays float32 only
    with pytest.raises(RuntimeError, match="float16"):
        dc.lod_gather(ri, pi, w, h["means3D"], h["scales"], h["rotations"], h["shs"], h["opacities"])
    # ... and the supported call still runs afterwards
    color, _, _ = _render(gpu, h, cut, M, K)
    assert bool(torch.isfinite(color).all())


def _abi_call(gpu, M=4, n=64):
    """A valid half-row argument block (built by the op's own glue), and workspaces for it."""
    from diff_gaussian_rasterization import _C as dc
    cut = _cut(n, seed=2)
    t = _tensors(gpu, M, False, True)
    ri, pi, w, kids = (torch.from_numpy(x).to(gpu) for x in cut)
    cam = synth.make_camera(W, H)
    a, keep, P, _ = dc._build_args(torch.zeros(3, device=gpu), t["means3D"], None, t["opacities"], t["scales"], t["rotations"],
                                   1.0, None, cam.world_view_transform.to(gpu), cam.full_proj_transform.to(gpu),
                                   cam.tanfovx, cam.tanfovy, H, W, t["shs"], DEGREE[M], cam.camera_center.to(gpu), False, w,
                                   kids, True, lod=(ri, pi, 0))
    assert a.lod_half_rows == 1 and P == n
    pl = dc._plan(_lib.lib(), P, W, H, 4096)
    ws = {k: torch.zeros(v, dtype=torch.uint8, device=gpu) for k, v in pl.items()}
    out = dict(radii=torch.zeros(P, dtype=torch.int32, device=gpu), color=torch.zeros(3, H, W, device=gpu),
               invdepth=torch.zeros(1, H, W, device=gpu))
    return a, keep, ws, out, P


def _forward_calls(gpu, a, ws, out):
    lib, p, L = _lib.lib(), _lib.ptr, C.c_uint32(0)
    st, dev = C.c_void_p(torch.cuda.current_stream().cuda_stream), gpu.index or 0
    return {
        "hgs_raster_fwd": lambda: lib.hgs_raster_fwd(C.byref(a), p(ws["geom"]), p(ws["bin"]), p(ws["img"]), 4096, p(out["radii"]),
                                                     p(out["color"]), p(out["invdepth"]), C.byref(L), st, dev),
        "hgs_raster_fwd_stage1": lambda: lib.hgs_raster_fwd_stage1(C.byref(a), p(ws["geom"]), p(out["radii"]), C.byref(L), st, dev),
        "hgs_raster_fwd_stage2": lambda: lib.hgs_raster_fwd_stage2(C.byref(a), p(ws["geom"]), p(ws["bin"]), p(ws["img"]), 4096,
                                                                   p(out["color"]), p(out["invdepth"]), st, dev),
    }


def test_c_abi_refusals_name_their_reason(gpu):
    a, keep, ws, out, P = _abi_call(gpu)
    calls = _forward_calls(gpu, a, ws, out)
    err = lambda: (_lib.lib().hgs_last_error() or b"").decode()
    spare = torch.zeros(G * 6, device=gpu)
    saved = {f: getattr(a, f) for f in ("lod_render_indices", "lod_parent_indices", "prepare_backward", "shs_rest",
                                         "activations", "colors_precomp", "cov3D_precomp", "lod_half_rows")}
    cases = [(dict(lod_render_indices=None, lod_parent_indices=None), "needs lod_render_indices"),
             (dict(prepare_backward=1), "forward only"),
             (dict(shs_rest=spare.data_ptr()), "no shs_rest, activations, colors_precomp or cov3D_precomp"),
             (dict(activations=_lib.ACT_SCALE_EXP), "no shs_rest, activations, colors_precomp or cov3D_precomp"),
             (dict(colors_precomp=spare.data_ptr()), "no shs_rest, activations, colors_precomp or cov3D_precomp"),
             (dict(cov3D_precomp=spare.data_ptr()), "no shs_rest, activations, colors_precomp or cov3D_precomp"),
             (dict(lod_half_rows=2), "lod_half_rows = 2"), (dict(lod_half_rows=-1), "lod_half_rows = -1")]
    for change, reason in cases:
        for f, v in change.items():
            setattr(a, f, v)
        for name, fn in calls.items():
            assert fn() == ERR_INVALID, (name, change)
            assert reason in err(), (name, change, err())
        for f in change:
            setattr(a, f, saved[f])
    torch.cuda.synchronize()
    assert int(out["radii"].abs().sum()) == 0 and float(out["color"].abs().sum()) == 0.0, "a refused call wrote its outputs"
    # the backward: any value other than 0
    lib, p = _lib.lib(), _lib.ptr
    g = _lib.RasterGrads()
    dl = torch.zeros(3, H, W, device=gpu)
    for v in (1, 2):
        a.lod_half_rows = v
        rc = lib.hgs_raster_bwd(C.byref(a), p(ws["geom"]), p(ws["bin"]), p(ws["img"]), p(ws["bwd"]), 4096, p(out["color"]),
                                p(out["invdepth"]), p(dl), None, C.byref(g), C.c_void_p(torch.cuda.current_stream().cuda_stream),
                                gpu.index or 0)
        assert rc == ERR_INVALID and "forward only" in err() and "hgs_raster_bwd" in err(), (v, err())
    a.lod_half_rows = 1
    # and the block itself is a good one: the single-call forward runs on it
    assert calls["hgs_raster_fwd"]() == 0, err()
    torch.cuda.synchronize()
    assert bool((out["color"] != 0).any()) and bool((out["radii"] > 0).any())
    del keep
