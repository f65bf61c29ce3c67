"""Every C-ABI workspace and output stays inside the bytes its size query (or the header's row count) grants, and no
result depends on what a workspace or write-only output held before the call.

The drop-in binding carves all workspaces of a frame out of one arena, so an overrun of one lands in the next and goes
unnoticed.  Here every workspace, scratch buffer and output gets an allocation of its own between two non-zero guards
(tests/ws_guard.py), at sizes off the 64-row wave grid and images off the 16-pixel tile grid.  Each case runs the same
call chain twice -- free buffers filled with 0x00, then with 0xFF -- and requires (a) intact guards and (b) bitwise equal
results, and (c) compares the results with the plain reference of the existing tests at their tolerances.  Buffers the
header says the caller initialises (accumulation targets, the zero-filled d_* of hgs_lod_gather_bwd) are initialised."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity as pa
import ws_guard as wg
from hgs import _lib, hierarchy, synth
from oracle import lod_oracle

pytestmark = pytest.mark.gpu

W, H = 67, 45
FILLS = (0x00, 0xFF)
BG = torch.tensor([0.1, 0.2, 0.3])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    _lib.check(rc, what)


class Bufs:
    """The guarded allocations of one run of a chain."""

    def __init__(self, dev, fill):
        self.dev, self.fill, self.all = dev, fill, []

    def new(self, name, nbytes, fill=None):
        g = wg.guarded(nbytes, self.dev, self.fill if fill is None else fill, name)
        self.all.append(g)
        return g

    def filled(self, name, dtype, shape, fill=None):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return self.new(name, n, fill).view(dtype, *shape)

    def copy_of(self, name, t):
        """An input in a guarded allocation (kernels must not write it, nor around it)."""
        t = t.contiguous()
        g = self.new(name, t.numel() * t.element_size())
        g.body.copy_(t.reshape(-1).view(torch.uint8).to(self.dev))
        return g.view(t.dtype, *t.shape)

    def check(self):
        wg.check(*self.all)


def _assert_same(r0, r1, path=""):
    if isinstance(r0, dict):
        assert r0.keys() == r1.keys(), path
        for k in r0:
            _assert_same(r0[k], r1[k], f"{path}.{k}")
    elif torch.is_tensor(r0):
        a, b = r0.contiguous().view(torch.uint8), r1.contiguous().view(torch.uint8)
        if not torch.equal(a, b):
            raise AssertionError(f"{path}: results differ between 0x00- and 0xFF-filled workspaces "
                                 f"({int((a != b).sum())} bytes)")
    elif isinstance(r0, (list, tuple)):
        assert len(r0) == len(r1), path
        for i, (a, b) in enumerate(zip(r0, r1)):
            _assert_same(a, b, f"{path}[{i}]")
    else:
        assert r0 == r1, (path, r0, r1)


def _both_fills(run):
    """run(fill) -> results (guards checked inside); the two fills give bitwise equal results."""
    r0, r1 = (run(f) for f in FILLS)
    _assert_same(r0, r1)
    return r0


# ================================================================================================================
# 1. rasterizer chain through raw ctypes
# ================================================================================================================
def _ws_sizes(lib, P, L):
    g, b, i, w = (C.c_size_t() for _ in range(4))
    _ok(lib.hgs_raster_ws_sizes(P, W, H, L, C.byref(g), C.byref(b), C.byref(i), C.byref(w)), "hgs_raster_ws_sizes")
    return g.value, b.value, i.value, w.value


def _cov3d(scene):
    """Upper triangle of R S S^T R^T in float64, rounded once (the 3D covariance of scales / rotations)."""
    q = scene.rotations.double()
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    Mx = R * scene.scales.double()[:, None, :]
    S = Mx @ Mx.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float()


def _case(P, seed, cam=None):
    cam = cam or synth.make_camera(W, H, 60.0)
    scene = synth.make_scene(P, cam, seed=seed)
    gc, gd = synth.upstream_grads(H, W, seed=seed + 1)
    return cam, scene, gc, gd


def _inputs(route, scene, dev):
    """Device tensors of one route: dict of the _build_args keywords."""
    d = lambda t: None if t is None else t.contiguous().to(dev)
    inp = dict(means3D=d(scene.means3D), opacity=d(scene.opacities), sh=d(scene.shs), colors=None, sh_rest=None,
               scales=d(scene.scales), rotations=d(scene.rotations), cov3D_precomp=None)
    if route == "shs_rest":
        inp["sh"], inp["sh_rest"] = d(scene.shs[:, :1]), d(scene.shs[:, 1:])
    elif route == "colors":
        inp["sh"], inp["colors"] = None, d(_colors(scene))
    elif route == "cov3D":
        inp["scales"] = inp["rotations"] = None
        inp["cov3D_precomp"] = d(_cov3d(scene))
    return inp


def _colors(scene):
    g = torch.Generator().manual_seed(scene.P)
    return torch.rand(scene.P, 3, generator=g)


def _build(cam, inp, degree, debug, dev, lod=None, weights=None, kids=None):
    from diff_gaussian_rasterization import _C
    return _C._build_args(BG.to(dev), inp["means3D"], inp["colors"], inp["opacity"], inp["scales"], inp["rotations"],
                          1.0, inp["cov3D_precomp"], cam.world_view_transform.to(dev),
                          cam.full_proj_transform.to(dev), cam.tanfovx, cam.tanfovy, H, W, inp["sh"], degree,
                          cam.camera_center.to(dev), debug, weights, kids, True, inp["sh_rest"], 0, lod)


def _views(lib, P, L, geom, binb, img, debug):
    """Integer state of the forward, read out of the guarded workspaces (tile_ids_sorted: the column itself after a debug
    forward, else rebuilt from the ranges as the binding does -- only debug forwards write the column)."""
    v = _lib.RasterViews()
    _ok(lib.hgs_raster_views_get(P, W, H, L, geom.addr, binb.addr, img.addr, C.byref(v)), "hgs_raster_views_get")
    T = ((W + 15) // 16) * ((H + 15) // 16)

    def at(g, addr, dtype, n):
        off = addr - g.addr
        esz = torch.empty((), dtype=dtype).element_size()
        return g.body[off:off + n * esz].view(dtype).cpu().clone()

    out = dict(tiles_touched=at(geom, v.tiles_touched, torch.int32, P), offsets=at(geom, v.offsets, torch.int32, P),
               depths=at(geom, v.depths, torch.float32, P), rects=at(geom, v.rects, torch.int32, 2 * P).view(P, 2),
               point_list=at(binb, v.point_list, torch.int32, L),
               ranges=at(binb, v.ranges, torch.int32, 2 * T).view(T, 2),
               final_T=at(img, v.final_T, torch.float32, H * W).view(H, W),
               n_contrib=at(img, v.n_contrib, torch.int32, H * W).view(H, W))
    if debug:
        out["tile_ids_sorted"] = at(binb, v.tile_ids_sorted, torch.int32, L)
    else:
        rg = out["ranges"].long()
        out["tile_ids_sorted"] = torch.repeat_interleave(torch.arange(T, dtype=torch.int32), (rg[:, 1] - rg[:, 0]).clamp(min=0))
    return out


def _grad_bufs(bufs, P, M, inp):
    """Guarded gradient outputs of hgs_raster_bwd (accumulate_grads = 0: all of them write-only)."""
    g = _lib.RasterGrads()
    out = {}

    def mk(key, field, shape):
        t = bufs.filled("dL_d" + key, torch.float32, shape)
        out[key] = t
        setattr(g, field, t.data_ptr())

    mk("means3D", "dL_dmeans3D", (P, 3))
    mk("means2D", "dL_dmeans2D", (P, 3))
    mk("opacities", "dL_dopacity", (P, 1))
    if inp["sh"] is not None:
        mk("shs", "dL_dshs", (P, inp["sh"].shape[1], 3))
    if inp["sh_rest"] is not None:
        mk("shs_rest", "dL_dshs_rest", (P, M - 1, 3))
    if inp["colors"] is not None:
        mk("colors_precomp", "dL_dcolors", (P, 3))
    if inp["scales"] is not None:
        mk("scales", "dL_dscales", (P, 3))
        mk("rotations", "dL_drotations", (P, 4))
    if inp["cov3D_precomp"] is not None:
        mk("cov3D_precomp", "dL_dcov3D", (P, 6))
    return g, out


def raster_chain(cam, inp, degree, gc, gd, dev, fill, *, prepare_backward=1, debug=0, mode="two_stage", L_hint=None,
                 lod=None, weights=None, kids=None, defer_sh=False):
    """Forward (two-stage, or hgs_raster_fwd with L_cap = L_hint / L_hint - 1) and backward, every workspace and output
    in its own guarded allocation.  Returns (results on the CPU, the live chain state for a deferred SH backward)."""
    lib = _lib.lib()
    a, keep, P, M = _build(cam, inp, degree, debug, dev, lod, weights, kids)
    a.prepare_backward = prepare_backward
    a.defer_sh_bwd = int(defer_sh)
    bufs = Bufs(dev, fill)
    n_geom, _, n_img, _ = _ws_sizes(lib, P, 0)
    geom, img = bufs.new("geom_ws", n_geom), bufs.new("img_ws", n_img)
    radii = bufs.filled("radii", torch.int32, (P,))
    color = bufs.filled("out_color", torch.float32, (3, H, W))
    invd = bufs.filled("out_invdepth", torch.float32, (1, H, W))
    L = C.c_uint32(0)
    p = _lib.ptr
    if mode == "two_stage":
        _ok(lib.hgs_raster_fwd_stage1(C.byref(a), geom.addr, p(radii), C.byref(L), _stream(), dev.index or 0), "stage1")
        L_ws = L.value
        binb = bufs.new("bin_ws", _ws_sizes(lib, P, L_ws)[1])
        _ok(lib.hgs_raster_fwd_stage2(C.byref(a), geom.addr, binb.addr, img.addr, L_ws, p(color), p(invd), _stream(),
                                      dev.index or 0), "stage2")
    else:
        L_cap = L_hint if mode == "fused_exact" else L_hint - 1
        binb = bufs.new("bin_ws(L_cap)", _ws_sizes(lib, P, L_cap)[1])
        rc = lib.hgs_raster_fwd(C.byref(a), geom.addr, binb.addr, img.addr, L_cap, p(radii), p(color), p(invd),
                                C.byref(L), _stream(), dev.index or 0)
        assert L.value == L_hint
        if mode == "fused_exact":
            _ok(rc, "hgs_raster_fwd")
            L_ws = L_cap
        else:
            assert rc == _lib.ERR_CAPACITY, rc
            bufs.check()                                  # the missed call stayed inside its L_cap-sized bin_ws
            L_ws = L.value
            binb = bufs.new("bin_ws", _ws_sizes(lib, P, L_ws)[1])
            _ok(lib.hgs_raster_fwd_stage2(C.byref(a), geom.addr, binb.addr, img.addr, L_ws, p(color), p(invd),
                                          _stream(), dev.index or 0), "stage2 after a capacity miss")
    bwd = bufs.new("bwd_ws", _ws_sizes(lib, P, L_ws)[3])
    g, grads = _grad_bufs(bufs, P, M, inp)
    dLc, dLd = gc.contiguous().to(dev), gd.contiguous().to(dev)
    _ok(lib.hgs_raster_bwd(C.byref(a), geom.addr, binb.addr, img.addr, bwd.addr, L_ws, p(color), p(invd), p(dLc),
                           p(dLd), C.byref(g), _stream(), dev.index or 0), "hgs_raster_bwd")
    bufs.check()
    res = dict(color=color.cpu().clone(), invdepth=invd.cpu().clone(), radii=radii.cpu().clone(), L=L.value,
               grads={k: v.cpu().clone() for k, v in grads.items()},
               views=_views(lib, P, L.value, geom, binb, img, debug))
    state = dict(a=a, keep=keep, bufs=bufs, geom=geom, bwd=bwd, grads=grads, L_ws=L_ws, P=P, M=M)
    return res, state


def _reference(cam, scene, route, **kw):
    extra = {}
    if route == "colors":
        extra["colors_precomp"] = _colors(scene)
    elif route == "cov3D":
        extra["cov3D_precomp"] = _cov3d(scene)
    return pa.oracle_run(scene, cam, BG, **extra, **kw)


def _check_against_reference(name, hip, orc, gc, gd):
    res = pa.verify(hip, orc, gc, gd)
    res["indices"] = pa.check_indices(hip, res["oracle"])
    pa.assert_verified(name, res)
    return res["oracle"]


SIZES = [1, 63, 65, 200, 255, 257, 10_440, 16_769]
RASTER_CASES = [("h48", P, 1, 0) for P in SIZES] + [("h48", P, 0, 0) for P in (63, 200, 10_440)] + \
    [("h48", P, 1, 1) for P in (200, 257)] + \
    [(r, P, 1, d) for r in ("shs_rest", "colors", "cov3D") for P, d in ((63, 0), (200, 1), (16_769, 0))]


@pytest.mark.parametrize("route,P,pb,debug", RASTER_CASES)
def test_raster_chain_stays_in_bounds(gpu, route, P, pb, debug):
    cam, scene, gc, gd = _case(P, seed=P % 89)
    orc = _reference(cam, scene, route)
    inp = _inputs(route, scene, gpu)
    run = lambda fill: raster_chain(cam, inp, scene.sh_degree, gc, gd, gpu, fill, prepare_backward=pb,
                                    debug=debug)[0]
    hip = _both_fills(run)
    if route == "shs_rest":            # the reference differentiates the concatenated [P, 16, 3] coefficients
        hip["grads"]["shs"] = torch.cat([hip["grads"]["shs"], hip["grads"].pop("shs_rest")], 1)
    oo = _check_against_reference(f"{route} P={P}", hip, orc, gc, gd)
    assert hip["L"] == oo.binning.num_rendered


@pytest.mark.parametrize("P", [200, 10_440])
@pytest.mark.parametrize("mode", ["fused_exact", "fused_miss"])
def test_single_call_forward_stays_in_bounds(gpu, P, mode):
    cam, scene, gc, gd = _case(P, seed=3)
    orc = _reference(cam, scene, "h48")
    inp = _inputs("h48", scene, gpu)
    L = int(orc(tiles=[]).binning.num_rendered)              # (geometry and binning only)
    assert L >= 2
    run = lambda fill: raster_chain(cam, inp, scene.sh_degree, gc, gd, gpu, fill, mode=mode, L_hint=L)[0]
    _check_against_reference(f"{mode} P={P}", _both_fills(run), orc, gc, gd)


def _lod_cut(P, seed):
    """A numpy hierarchy over P leaves and a blending cut through it (lod_oracle), with the gathered rows the in-op
    interpolation computes, in float32 as the header defines them."""
    cam = synth.make_camera(W, H, 60.0)
    sc = synth.make_scene(P, cam, seed=seed)
    h = hierarchy.build_hierarchy(sc)
    tau = 2 * 4.5 * cam.tanfovx / (0.5 * W)
    ri, pi, ni = lod_oracle.expand_to_size(h.nodes.numpy(), h.boxes.numpy(), tau, cam.camera_center.numpy())
    w, ns = lod_oracle.get_interpolation_weights(ni, tau, h.nodes.numpy(), h.boxes.numpy(), cam.camera_center.numpy())
    rows = dict(means3D=h.xyz, scales=torch.exp(h.log_scales), rotations=torch.nn.functional.normalize(h.rots),
                opacities=h.alpha.abs(), shs=h.shs)
    ri_t, pi_t, wt = torch.from_numpy(ri.astype(np.int64)), torch.from_numpy(pi.astype(np.int64)), torch.from_numpy(w)
    wc = wt[:, None]
    g = {}
    for k, v in rows.items():
        node, par = v[ri_t], v[pi_t]
        if k == "rotations":
            par = torch.where(((node * par).sum(1, keepdim=True) < 0), -par, par)
        ww = wc if v.dim() == 2 else wc[:, :, None]
        g[k] = ww * node + (1 - ww) * par
    gathered = synth.Scene(g["means3D"].contiguous(), g["scales"].contiguous(), g["rotations"].contiguous(),
                           g["opacities"].contiguous(), g["shs"].contiguous(), 3)
    return cam, rows, gathered, ri, pi, w, ns


def test_in_op_lod_chain_stays_in_bounds(gpu):
    cam, rows, gathered, ri, pi, w, ns = _lod_cut(600, seed=5)
    n = len(ri)
    assert 64 < n and n % 64 != 0 and bool(((w > 0) & (w < 1)).any()), (n, "the cut must blend and sit off the grid")
    gc, gd = synth.upstream_grads(H, W, seed=11)
    wt, kt = torch.from_numpy(w), torch.from_numpy(ns.astype(np.int32))
    orc = pa.oracle_run(gathered, cam, BG, interpolation_weights=wt, num_node_kids=kt)
    d = lambda t: t.contiguous().to(gpu)
    inp = dict(means3D=d(rows["means3D"]), opacity=d(rows["opacities"]), sh=d(rows["shs"]), colors=None, sh_rest=None,
               scales=d(rows["scales"]), rotations=d(rows["rotations"]), cov3D_precomp=None)
    lod = (d(torch.from_numpy(ri.astype(np.int32))), d(torch.from_numpy(pi.astype(np.int32))), 0)
    run = lambda fill: raster_chain(cam, inp, 3, gc, gd, gpu, fill, lod=lod, weights=d(wt), kids=d(kt))[0]
    _check_against_reference(f"in-op LOD n={n}", _both_fills(run), orc, gc, gd)


def _view_cams(n):
    return [synth.make_camera(W, H, 60.0, T=[0.04 * i, -0.03 * i, 0.02 * i]) for i in range(n)]


@pytest.mark.parametrize("P", [200, 10_440])
@pytest.mark.parametrize("n_views", [1, _lib.MAX_DEFERRED_VIEWS])
def test_deferred_sh_backward_stays_in_bounds(gpu, P, n_views):
    """hgs_raster_bwd with defer_sh_bwd = 1 per view, then hgs_raster_sh_bwd_batched over the views: against the sum of
    the views' reference gradients."""
    cams = _view_cams(n_views)
    scene = synth.make_scene(P, cams[0], seed=P % 31)
    gc, gd = synth.upstream_grads(H, W, seed=7)
    inp = _inputs("h48", scene, gpu)
    lib = _lib.lib()
    views = []                       # the views' forward results (for the reference: the outcomes they took)

    def run(fill):
        chains = [raster_chain(c, inp, 3, gc, gd, gpu, fill, defer_sh=True) for c in cams]
        views[:] = [r for r, _ in chains]
        states = [st for _, st in chains]
        bufs = Bufs(gpu, fill)
        d_sh = bufs.filled("dL_dshs", torch.float32, (P, 16, 3))                 # written (accumulate = 0)
        d_m3 = bufs.filled("dL_dmeans3D", torch.float32, (P, 3), fill=0x00)      # += target: the views' sum goes in
        d_m3.copy_(sum(s["grads"]["means3D"].double() for s in states).float())
        arr = (_lib.ShBwdView * n_views)()
        for v, s, c in zip(arr, states, cams):
            v.geom_ws, v.bwd_ws, v.campos, v.L = s["geom"].addr, s["bwd"].addr, s["keep"][3].data_ptr(), s["L_ws"]
        _ok(lib.hgs_raster_sh_bwd_batched(arr, n_views, P, 16, 3, inp["means3D"].data_ptr(), inp["sh"].data_ptr(),
                                          d_sh.data_ptr(), d_m3.data_ptr(), 0, _stream(), gpu.index or 0),
            "hgs_raster_sh_bwd_batched")
        for s in states:
            s["bufs"].check()
        bufs.check()
        return dict(shs=d_sh.cpu().clone(), means3D=d_m3.cpu().clone())

    hip = _both_fills(run)
    refs = [pa.verify(v, _reference(c, scene, "h48"), gc, gd) for v, c in zip(views, cams)]
    for r in refs:
        assert r["stats"]["fragile_unmatched"] == 0 and r["stats"]["fragile_unenumerated"] == 0, r["stats"]
    for k in ("shs", "means3D"):
        ref = sum(r["grads"][k] for r in refs)
        st = pa.err_stats(hip[k], ref)
        assert st["maxrel"] <= pa.REL_TOL and st["l2"] <= pa.REL_TOL, (k, st)


@pytest.mark.parametrize("P", [200, 16_769])
@pytest.mark.parametrize("n_views", [1, _lib.MAX_DEFERRED_VIEWS])
def test_batched_sh_colors_stay_in_bounds(gpu, P, n_views):
    cams = _view_cams(n_views)
    scene = synth.make_scene(P, cams[0], seed=P % 37)
    lib = _lib.lib()
    m3, shs = scene.means3D.to(gpu), scene.shs.contiguous().to(gpu)
    g = torch.Generator().manual_seed(P)
    d_rgbs = [torch.randn(P, 3, generator=g) for _ in cams]

    def run(fill):
        bufs = Bufs(gpu, fill)
        views = (_lib.ShColorView * n_views)()
        keep = []
        for v, c, dr in zip(views, cams, d_rgbs):
            cp, rgb = c.camera_center.contiguous().to(gpu), bufs.filled("rgb", torch.float32, (P, 3))
            cl, d = bufs.filled("clamp", torch.uint8, (P,)), bufs.copy_of("d_rgb", dr)
            keep.append((cp, rgb, cl, d))
            v.campos, v.rgb, v.clamp, v.d_rgb = cp.data_ptr(), rgb.data_ptr(), cl.data_ptr(), d.data_ptr()
        _ok(lib.hgs_sh_colors_batched(views, n_views, P, 16, 3, m3.data_ptr(), shs.data_ptr(), _stream(),
                                      gpu.index or 0), "hgs_sh_colors_batched")
        d_sh = bufs.filled("dL_dshs", torch.float32, (P, 16, 3))
        d_m3 = bufs.filled("dL_dmeans3D", torch.float32, (P, 3), fill=0x00)     # += target, zeroed by the caller
        _ok(lib.hgs_sh_colors_batched_bwd(views, n_views, P, 16, 3, m3.data_ptr(), shs.data_ptr(), d_sh.data_ptr(),
                                          d_m3.data_ptr(), 0, _stream(), gpu.index or 0), "hgs_sh_colors_batched_bwd")
        bufs.check()
        return dict(rgb=[k[1].cpu().clone() for k in keep], clamp=[k[2].cpu().clone() for k in keep],
                    shs=d_sh.cpu().clone(), means3D=d_m3.cpu().clone())

    r0, r1 = (run(f) for f in FILLS)
    for k in ("shs", "means3D"):
        _assert_same(r0[k], r1[k], k)
    for i in range(n_views):
        _assert_same(r0["rgb"][i], r1["rgb"][i], f"rgb[{i}]")
        _assert_same(r0["clamp"][i], r1["clamp"][i], f"clamp[{i}]")
    # reference: float64 autograd through the same expression, the clamp masking the upstream gradient
    leaf_sh = scene.shs.double().clone().requires_grad_(True)
    leaf_m3 = scene.means3D.double().clone().requires_grad_(True)
    loss = 0
    from oracle import raster_oracle as ro
    for i, (c, dr) in enumerate(zip(cams, d_rgbs)):
        dirs = leaf_m3 - c.camera_center.double()
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        raw = ro.eval_sh_torch(3, leaf_sh, dirs) + 0.5
        ref_rgb = raw.clamp(min=0).detach()
        st = pa.err_stats(r0["rgb"][i], ref_rgb)
        assert st["maxrel"] <= pa.REL_TOL and st["l2"] <= pa.REL_TOL, ("rgb", i, st)
        bits = r0["clamp"][i].long()
        clamped = torch.stack([(bits >> ch) & 1 for ch in range(3)], 1).bool()
        fragile = raw.detach().abs() < 1e-6
        assert bool(((clamped == (raw.detach() < 0)) | fragile).all()), ("clamp bits", i)
        loss = loss + (raw * dr.double() * (~clamped)).sum()
    loss.backward()
    for k, ref in (("shs", leaf_sh.grad), ("means3D", leaf_m3.grad)):
        st = pa.err_stats(r0[k], ref)
        assert st["maxrel"] <= pa.REL_TOL and st["l2"] <= pa.REL_TOL, (k, st)


# ================================================================================================================
# 2. sort
# ================================================================================================================
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4_097, 300_001])
@pytest.mark.parametrize("end_bit", [8, 32, 45, 64])
def test_sort_pairs_stays_in_bounds(gpu, n, end_bit):
    lib = _lib.lib()
    rng = np.random.default_rng(n * 67 + end_bit)
    hi = np.uint64((1 << end_bit) - 1) if end_bit < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    keys &= hi
    keys[rng.random(n) < 0.3] = keys[0]                    # runs of equal keys: stability matters
    vals = rng.permutation(n).astype(np.uint32)
    order = np.argsort(keys, kind="stable")
    ref_k, ref_v = keys[order], vals[order]

    def run(fill):
        bufs = Bufs(gpu, fill)
        k_in = bufs.copy_of("keys_in", torch.from_numpy(keys.view(np.int64)))
        v_in = bufs.copy_of("vals_in", torch.from_numpy(vals.view(np.int32)))
        k_out = bufs.filled("keys_out", torch.int64, (n,))
        v_out = bufs.filled("vals_out", torch.int32, (n,))
        tmp = bufs.new("tmp", lib.hgs_sort_tmp_bytes(n))
        _ok(lib.hgs_sort_pairs(k_in.data_ptr(), v_in.data_ptr(), k_out.data_ptr(), v_out.data_ptr(), tmp.addr, n,
                               end_bit, _stream(), gpu.index or 0), "hgs_sort_pairs")
        bufs.check()
        assert torch.equal(k_in.cpu(), torch.from_numpy(keys.view(np.int64))), "keys_in was modified"
        return dict(k=k_out.cpu().clone(), v=v_out.cpu().clone())

    r = _both_fills(run)
    assert np.array_equal(r["k"].numpy().view(np.uint64), ref_k)
    assert np.array_equal(r["v"].numpy().view(np.uint32), ref_v)


# ================================================================================================================
# 3. hierarchy build and LOD
# ================================================================================================================
@pytest.mark.parametrize("P", [1, 2, 3, 63, 65, 257, 4_099])
def test_hier_build_stays_in_bounds(gpu, P):
    from test_hier_build_gpu import compare_to_spec
    lib = _lib.lib()
    cam = synth.make_camera(W, H, 60.0)
    sc = synth.make_scene(P, cam, seed=P % 13)
    N = 2 * P - 1

    def run(fill):
        bufs = Bufs(gpu, fill)
        xyz, scales = bufs.copy_of("xyz", sc.means3D), bufs.copy_of("scales", sc.scales)
        rots, op = bufs.copy_of("rots", sc.rotations), bufs.copy_of("opacity", sc.opacities.reshape(P))
        shs = bufs.copy_of("shs", sc.shs)
        out = dict(xyz=bufs.filled("out_xyz", torch.float32, (N, 3)),
                   shs=bufs.filled("out_shs", torch.float32, (N, 16, 3)),
                   alpha=bufs.filled("out_alpha", torch.float32, (N, 1)),
                   log_scales=bufs.filled("out_log_scales", torch.float32, (N, 3)),
                   rots=bufs.filled("out_rots", torch.float32, (N, 4)),
                   nodes=bufs.filled("out_nodes", torch.int32, (N, 7)),
                   boxes=bufs.filled("out_boxes", torch.float32, (N, 2, 4)))
        tmp = bufs.new("tmp", lib.hgs_hier_build_tmp_bytes(P))
        p = lambda k: out[k].data_ptr()
        _ok(lib.hgs_hier_build(xyz.data_ptr(), scales.data_ptr(), rots.data_ptr(), op.data_ptr(), shs.data_ptr(), P,
                               16, p("xyz"), p("shs"), p("alpha"), p("log_scales"), p("rots"), p("nodes"), p("boxes"),
                               tmp.addr, _stream(), gpu.index or 0), "hgs_hier_build")
        bufs.check()
        return {k: v.cpu().clone() for k, v in out.items()}

    r = _both_fills(run)
    compare_to_spec(hierarchy.Hierarchy(**r), hierarchy.build_hierarchy(sc))


def _vec3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


@pytest.mark.parametrize("P", [65, 257, 4_099])
def test_lod_cut_weights_and_gather_stay_in_bounds(gpu, P):
    lib = _lib.lib()
    cam = synth.make_camera(W, H, 60.0)
    sc = synth.make_scene(P, cam, seed=P % 17)
    h = hierarchy.build_hierarchy(sc)
    N = h.num_nodes
    vp = cam.camera_center.numpy()
    tau = 2 * 4.5 * cam.tanfovx / (0.5 * W)
    ri, pi, ni = lod_oracle.expand_to_size(h.nodes.numpy(), h.boxes.numpy(), tau, vp)
    w, ns = lod_oracle.get_interpolation_weights(ni, tau, h.nodes.numpy(), h.boxes.numpy(), vp)
    n = len(ri)
    assert 1 < n < N
    rows = dict(means3D=h.xyz, scales=torch.exp(h.log_scales), rotations=torch.nn.functional.normalize(h.rots),
                opacities=h.alpha.abs(), shs=h.shs)
    inner = dict(means3D=(3,), scales=(3,), rotations=(4,), opacities=(1,), shs=(16, 3))
    g = torch.Generator().manual_seed(P)
    g_rows = {k: torch.randn((n,) + s, generator=g) for k, s in inner.items()}

    def run(fill):
        bufs = Bufs(gpu, fill)
        nodes, boxes = bufs.copy_of("nodes", h.nodes), bufs.copy_of("boxes", h.boxes)
        res = {}
        for fn_name in ("hgs_expand_to_size", "hgs_expand_to_size_nested"):
            outs = [bufs.filled(f"{fn_name}.{k}", torch.int32, (n,)) for k in ("render", "parent", "nodes_for")]
            tmp = bufs.new(f"{fn_name}.tmp", lib.hgs_expand_tmp_bytes(N))
            cnt = C.c_int32(0)
            _ok(getattr(lib, fn_name)(nodes.data_ptr(), boxes.data_ptr(), N, tau, _vec3(vp), _vec3((0, 0, 0)),
                                      *(o.data_ptr() for o in outs), n, tmp.addr, C.byref(cnt), _stream(),
                                      gpu.index or 0), fn_name)
            assert cnt.value == n, (fn_name, cnt.value, n)
            res[fn_name] = [o.cpu().clone() for o in outs]
        flag = bufs.new("nested.tmp", 4)
        nested = C.c_int32(-1)
        _ok(lib.hgs_hier_boxes_nested(nodes.data_ptr(), boxes.data_ptr(), N, flag.addr, C.byref(nested), _stream(),
                                      gpu.index or 0), "hgs_hier_boxes_nested")
        res["nested"] = nested.value
        ni_d = bufs.copy_of("node_indices", torch.from_numpy(ni.astype(np.int32)))
        wt = bufs.filled("interpolation_weights", torch.float32, (n,))
        nsib = bufs.filled("num_siblings", torch.int32, (n,))
        _ok(lib.hgs_interp_weights(ni_d.data_ptr(), n, tau, nodes.data_ptr(), boxes.data_ptr(), N, _vec3(vp),
                                   _vec3((0, 0, 0)), wt.data_ptr(), nsib.data_ptr(), _stream(), gpu.index or 0),
            "hgs_interp_weights")
        res["w"], res["ns"] = wt.cpu().clone(), nsib.cpu().clone()
        # gather / scatter over the cut
        ri_d = bufs.copy_of("render_indices", torch.from_numpy(ri.astype(np.int32)))
        pi_d = bufs.copy_of("parent_indices", torch.from_numpy(pi.astype(np.int32)))
        w_d = bufs.copy_of("weights", torch.from_numpy(w))
        src = {k: bufs.copy_of(k, v) for k, v in rows.items()}
        o = {k: bufs.filled("o_" + k, torch.float32, (n,) + s) for k, s in inner.items()}
        _ok(lib.hgs_lod_gather(ri_d.data_ptr(), pi_d.data_ptr(), w_d.data_ptr(), n, 16,
                               *(src[k].data_ptr() for k in ("means3D", "scales", "rotations", "shs", "opacities")),
                               *(o[k].data_ptr() for k in ("means3D", "scales", "rotations", "shs", "opacities")),
                               _stream(), gpu.index or 0), "hgs_lod_gather")
        gi = {k: bufs.copy_of("g_" + k, v) for k, v in g_rows.items()}
        d = {k: bufs.filled("d_" + k, torch.float32, (N,) + s, fill=0x00) for k, s in inner.items()}   # zeroed: caller
        flag2 = bufs.new("gather_bwd.flag", 4)
        _ok(lib.hgs_lod_gather_bwd(ri_d.data_ptr(), pi_d.data_ptr(), w_d.data_ptr(), n, 16, src["rotations"].data_ptr(),
                                   *(gi[k].data_ptr() for k in ("means3D", "scales", "rotations", "shs", "opacities")),
                                   *(d[k].data_ptr() for k in ("means3D", "scales", "rotations", "shs", "opacities")),
                                   flag2.addr, _stream(), gpu.index or 0), "hgs_lod_gather_bwd")
        bufs.check()
        res["o"] = {k: v.cpu().clone() for k, v in o.items()}
        res["d"] = {k: v.cpu().clone() for k, v in d.items()}
        return res

    r = _both_fills(run)
    assert r["nested"] == 1
    for fn_name in ("hgs_expand_to_size", "hgs_expand_to_size_nested"):
        for got, ref in zip(r[fn_name], (ri, pi, ni)):
            assert np.array_equal(got.numpy(), ref.astype(np.int32)), fn_name
    assert np.array_equal(r["w"].numpy().view(np.uint32), w.astype(np.float32).view(np.uint32))
    assert np.array_equal(r["ns"].numpy(), ns.astype(np.int32))
    # gather: the float64 expression, and its adjoint for the scatter
    ri_t, pi_t = torch.from_numpy(ri.astype(np.int64)), torch.from_numpy(pi.astype(np.int64))
    wd = torch.from_numpy(w).double()
    for k, v in rows.items():
        v = v.double().reshape(N, -1)
        node, par = v[ri_t], v[pi_t]
        sign = torch.ones(n, 1, dtype=torch.float64)
        if k == "rotations":
            sign = torch.where((node * par).sum(1, keepdim=True) < 0, -1.0, 1.0).double()
        ref = wd[:, None] * node + (1 - wd[:, None]) * sign * par
        st = pa.err_stats(r["o"][k].reshape(n, -1), ref)
        assert st["maxrel"] <= pa.REL_TOL and st["l2"] <= pa.REL_TOL, ("gather", k, st)
        gk = g_rows[k].double().reshape(n, -1)
        dref = torch.zeros(N, gk.shape[1], dtype=torch.float64)
        dref.index_add_(0, ri_t, wd[:, None] * gk)
        dref.index_add_(0, pi_t, (1 - wd[:, None]) * sign * gk)
        st = pa.err_stats(r["d"][k].reshape(N, -1), dref)
        assert st["maxrel"] <= pa.REL_TOL and st["l2"] <= pa.REL_TOL, ("gather_bwd", k, st)


# ================================================================================================================
# 4. distCUDA2
# ================================================================================================================
@pytest.mark.parametrize("P", [1, 2, 3, 4, 63, 65, 1_025])
def test_dist2_knn3_stays_in_bounds(gpu, P):
    """Against a float64 brute force.  With fewer than 4 points the kernel's convention applies (csrc/knn.hip): the sum
    over the P - 1 neighbours there are, divided by 3."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(P)
    pts = torch.randn(P, 3, generator=g) * torch.tensor([3.0, 1.0, 0.2])
    pts[: P // 10] = pts[: P // 10].round()                          # clusters + exact duplicates

    def run(fill):
        bufs = Bufs(gpu, fill)
        xyz = bufs.copy_of("xyz", pts)
        out = bufs.filled("out_mean_d2", torch.float32, (P,))
        tmp = bufs.new("tmp", lib.hgs_knn_tmp_bytes(P))
        _ok(lib.hgs_dist2_knn3(xyz.data_ptr(), P, out.data_ptr(), tmp.addr, _stream(), gpu.index or 0),
            "hgs_dist2_knn3")
        bufs.check()
        return out.cpu().clone()

    got = _both_fills(run)
    d2 = torch.cdist(pts.double(), pts.double()) ** 2
    d2.fill_diagonal_(float("inf"))
    k = min(3, P - 1)
    ref = d2.topk(k, dim=1, largest=False).values.sum(1) / 3 if k > 0 else torch.zeros(P, dtype=torch.float64)
    assert torch.allclose(got.double(), ref, rtol=1e-4, atol=1e-6), (P, got[:4], ref[:4])


# ================================================================================================================
# 5. fused SSIM loss
# ================================================================================================================
SSIM_SIZES = [(1, 3, 45, 67), (3, 1, 17, 33), (2, 4, 5, 1)]


@pytest.mark.parametrize("dims", SSIM_SIZES)
@pytest.mark.parametrize("per_image", [0, 1])
def test_ssim_stays_in_bounds(gpu, dims, per_image):
    """hgs_ssim_fwd with maps, hgs_ssim_fwd with maps = NULL (the same value bits), hgs_ssim_bwd with a non-unit
    upstream gradient; against the float64 spec within test_ssim_gpu's float32 yardstick rule."""
    from test_ssim_gpu import errors, pair, yardstick
    import ssim_spec
    lib = _lib.lib()
    N, Ch, Hs, Ws = dims
    x1, x2 = pair(dims, seed=N * 1000 + Hs)
    go = torch.tensor([0.7, -1.3, 2.5][:N]) if per_image else torch.tensor([-0.2])

    def run(fill):
        bufs = Bufs(gpu, fill)
        i1, i2 = bufs.copy_of("img1", x1), bufs.copy_of("img2", x2)
        out_image = bufs.filled("out_image", torch.float32, (N,))
        out_mean = bufs.filled("out_mean", torch.float32, (1,))
        maps = bufs.filled("maps", torch.float32, (3, N, Ch, Hs, Ws))
        tmp = bufs.new("tmp", lib.hgs_ssim_tmp_bytes(N, Ch, Hs, Ws))
        _ok(lib.hgs_ssim_fwd(i1.data_ptr(), i2.data_ptr(), N, Ch, Hs, Ws, out_image.data_ptr(), out_mean.data_ptr(),
                             maps.data_ptr(), tmp.addr, _stream(), gpu.index or 0), "hgs_ssim_fwd")
        g = bufs.copy_of("grad_out", go)
        grad = bufs.filled("grad_img1", torch.float32, (N, Ch, Hs, Ws))
        _ok(lib.hgs_ssim_bwd(i1.data_ptr(), i2.data_ptr(), maps.data_ptr(), g.data_ptr(), per_image, N, Ch, Hs, Ws,
                             grad.data_ptr(), _stream(), gpu.index or 0), "hgs_ssim_bwd")
        out_image0 = bufs.filled("out_image(no maps)", torch.float32, (N,))
        out_mean0 = bufs.filled("out_mean(no maps)", torch.float32, (1,))
        tmp0 = bufs.new("tmp(no maps)", lib.hgs_ssim_tmp_bytes(N, Ch, Hs, Ws))
        _ok(lib.hgs_ssim_fwd(i1.data_ptr(), i2.data_ptr(), N, Ch, Hs, Ws, out_image0.data_ptr(), out_mean0.data_ptr(),
                             None, tmp0.addr, _stream(), gpu.index or 0), "hgs_ssim_fwd (maps = NULL)")
        bufs.check()
        assert torch.equal(x1, i1.cpu()) and torch.equal(x2, i2.cpu()), "an input was modified"
        return dict(out_image=out_image.cpu().clone(), out_mean=out_mean.cpu().clone(), maps=maps.cpu().clone(),
                    grad=grad.cpu().clone(), out_image0=out_image0.cpu().clone(), out_mean0=out_mean0.cpu().clone())

    r = _both_fills(run)
    _assert_same(r["out_image0"], r["out_image"], "out_image with maps = NULL")
    _assert_same(r["out_mean0"], r["out_mean"], "out_mean with maps = NULL")
    size_average = not per_image
    grad_out = go if per_image else go[0]
    vs, gs = ssim_spec.ssim_and_grad(x1.double(), x2.double(), size_average=size_average, grad_out=grad_out.double())
    ye = errors(*yardstick(x1, x2, size_average, grad_out), vs, gs)
    he = errors(r["out_image"] if per_image else r["out_mean"][0], r["grad"], vs, gs)
    assert he[0] <= max(2e-6, 3 * ye[0]) and he[1] <= 1.5 * ye[1] and he[2] <= 3 * ye[2], (he, ye)
    other = r["out_mean"][0] if per_image else r["out_image"]          # the output the upstream gradient is not of
    vo = ssim_spec.ssim(x1.double(), x2.double(), size_average=not size_average)
    yo = (yardstick(x1, x2, not size_average)[0].double() - vo).abs().max().item()
    assert (other.double() - vo).abs().max().item() <= max(2e-6, 3 * yo)


# ================================================================================================================
# 6. hierarchy merge
# ================================================================================================================
@pytest.mark.parametrize("Ps,tails", [([1], [0]), ([63, 65], [0, 0]), ([1, 257, 4_099], [0, 9, 0])])
def test_hier_merge_stays_in_bounds(gpu, Ps, tails):
    """hgs_hier_merge_place per chunk (its rows in guarded copies, a skybox tail G > N on one), then
    hgs_hier_merge_root: every merged array in its own guarded, 0x00- or 0xFF-filled allocation, so a byte the merger
    does not write shows as a difference between the fills; against the spec on the trimmed chunks."""
    from test_hier_merge_gpu import _chunk, _cpu, _trim, _with_tail, compare_to_spec
    lib = _lib.lib()
    chunks = [_chunk(P, seed=P % 11 + i, dev=gpu, shift=(3.0 * i, -1.0 * i)) for i, P in enumerate(Ps)]
    sources = [_cpu(_with_tail(c, t, seed=t) if t else c) for c, t in zip(chunks, tails)]
    assert any(s.xyz.shape[0] > s.num_nodes for s in sources) == any(tails)
    k = len(Ps)
    bases, N = hierarchy.merge_layout([s.num_nodes for s in sources])
    M = 16

    def hv(G, n, h):
        return _lib.HierView(G, n, M, 0, *(h[f].data_ptr() for f in ("xyz", "shs", "alpha", "log_scales", "rots",
                                                                     "nodes", "boxes")))

    def run(fill):
        bufs = Bufs(gpu, fill)
        out = dict(xyz=bufs.filled("merged.xyz", torch.float32, (N, 3)),
                   shs=bufs.filled("merged.shs", torch.float32, (N, M, 3)),
                   alpha=bufs.filled("merged.alpha", torch.float32, (N, 1)),
                   log_scales=bufs.filled("merged.log_scales", torch.float32, (N, 3)),
                   rots=bufs.filled("merged.rots", torch.float32, (N, 4)),
                   nodes=bufs.filled("merged.nodes", torch.int32, (N, 7)),
                   boxes=bufs.filled("merged.boxes", torch.float32, (N, 2, 4)))
        tmp = bufs.new("tmp", _lib.HIER_MERGE_TMP_BYTES)
        merged = hv(N, N, out)
        for c, s in enumerate(sources):
            h = {f: bufs.copy_of(f"chunk{c}.{f}", getattr(s, f)) for f in ("xyz", "shs", "alpha", "log_scales",
                                                                           "rots", "nodes", "boxes")}
            rep = _lib.HierMergeReport()
            _ok(lib.hgs_hier_merge_place(C.byref(hv(s.xyz.shape[0], s.num_nodes, h)), c, k, bases[c],
                                         C.byref(merged), tmp.addr, C.byref(rep), _stream(), gpu.index or 0),
                f"hgs_hier_merge_place({c})")
            assert list(rep.first_bad) == [-1, -1, -1] and rep.children_sum == s.num_nodes - 1
            for f, t in h.items():
                assert torch.equal(t.cpu(), getattr(s, f)), f"chunk {c}'s {f} was modified"
        _ok(lib.hgs_hier_merge_root(C.byref(merged), k, _stream(), gpu.index or 0), "hgs_hier_merge_root")
        bufs.check()
        return {f: t.cpu().clone() for f, t in out.items()}

    r = _both_fills(run)
    compare_to_spec(hierarchy.Hierarchy(**r), hierarchy.merge_hierarchies([_trim(s) for s in sources]))


# ================================================================================================================
# 7. budgeted residency
# ================================================================================================================
def _resid_cut(rows, n, rng):
    """A cut of n entries whose distinct needed rows are exactly ``rows``."""
    ri = rng.permutation(np.concatenate([rows, rng.choice(rows, n - len(rows))])).astype(np.int32)
    return ri, rng.choice(rows, n).astype(np.int32), rng.choice(np.array([1.0, 0.5], np.float32), n)


@pytest.mark.parametrize("M", [1, 9, 16])
@pytest.mark.parametrize("G,B,n", [(1, 1, 1), (65, 63, 64), (257, 255, 300), (1003, 257, 1000)])
def test_residency_chain_stays_in_bounds(gpu, G, B, n, M):
    """hgs_resid_mark -> _evict -> _fetch -> _remap, every device buffer of the four calls between guards: a first frame
    that fills the budget with rows 0 .. B-1, then one that needs rows G-B .. G-1 -- the last host row into the last
    free slot, after an eviction wherever the two sets differ.  The caller initialises slot_of, id_of_slot and free_list
    (include/hgs.h); stamp, counters, the slot arrays, miss_ids, ro and po hold the fill.  Which slot a row gets depends
    on the order of the miss list and of the free stack, which the header leaves open: results are compared by row id
    (tests/residency_model.py: by_id), between the fills and with the plain slot cache."""
    import residency_model as rm
    from test_residency_kernels_gpu import DeviceCache, HostRows
    rng = np.random.default_rng(G + M)
    cuts = [_resid_cut(np.arange(B), n, rng), _resid_cut(np.arange(G - B, G), n, rng)]
    host_np = rm.pattern_rows(G, M)
    host = HostRows(host_np)

    def run(fill):
        bufs = Bufs(gpu, fill)
        dc = DeviceCache(gpu, G, B, M, host, cap=n, alloc=lambda name, dtype, count: bufs.filled(name, dtype, (count,)))
        res = []
        for frame, (ri, pi, w) in enumerate(cuts, start=1):
            dc.set_cut(ri, pi, w, prefill=False)
            rc, count = dc.mark(frame)
            _ok(rc, "hgs_resid_mark")
            _ok(dc.evict(frame, count), "hgs_resid_evict")
            _ok(dc.fetch(count, frame), "hgs_resid_fetch")
            _ok(dc.remap(), "hgs_resid_remap")
            bufs.check()
            assert dc.free_top == 0                                # the budget is full to its last slot
            s = dc.state()
            rm.check_invariants(s["slot_of"], s["id_of_slot"], s["free_list"], s["free_top"], B)
            for t, a in ((dc.ri, ri), (dc.pi, pi), (dc.w, w)):
                assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32)), "an input was modified"
            res.append(dict(count=count, **{k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v
                                            for k, v in rm.by_id(s, dc.out(dc.ro), dc.out(dc.po)).items()}))
        return res

    try:
        got = _both_fills(run)
    finally:
        torch.cuda.synchronize()
        host.free()
    model = rm.SlotCache(G, B, M, host_np)
    for frame, ((ri, pi, w), r) in enumerate(zip(cuts, got), start=1):
        rc, ro, po, m = model.make_resident(ri, pi, w, frame)
        assert rc == rm.OK and r["count"] == m == (B if frame == 1 else min(B, G - B))
        want = rm.by_id(rm.state_of(model), ro, po)
        for k, v in want.items():
            assert np.array_equal(np.asarray(r[k]), v), (frame, k)
        assert np.array_equal(want["ro_ids"], ri) and np.array_equal(want["resident"], np.unique(ri))
