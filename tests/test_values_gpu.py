"""hgs_raster_values on the GPU: against the float64 spec (tests/values_spec.py), against K6's own image bit for bit,
against f-22 and f-24 on the same forward, under NaN poison, slot maps, channel groups and guard words, on the in-op
LOD route, and the Python layers built on it.

Against the spec, on non-fragile pixels and per channel,
    |device - spec| <= MIXED_REL * Aabs + MIXED_ABS * max over the pixels of Aabs
with ``Aabs`` the same sum over the absolute values (the values are signed: they cancel in the sum, their rounding does
not) and the constants of tests/parity.py; the fragile share must stay under parity.FRAGILE_FRAC -- a condition."""
import ctypes as C
import functools
import json
import math

import numpy as np
import pytest
import torch

import contribution_cases as cc
import parity as pa
import pixels_spec as ps
import values_spec as vs
import ws_guard as wg
from hgs import _lib, synth

pytestmark = pytest.mark.gpu

BG = (0.25, -0.5, 0.75, 0.125)


def _forward(gpu, cam, scene, bg=None, do_depth=False):
    """(color, invdepth, call) of the plain rows' no-grad forward on the product path."""
    import diff_gaussian_rasterization as dgr
    from hgs.importance import _view_forward
    rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(cam, torch.zeros(3) if bg is None else bg, scene.sh_degree,
                                                                do_depth=do_depth, device=gpu))
    s = scene.to(gpu)
    with torch.no_grad():
        res, _ = _view_forward(rs, s.means3D, s.opacities, s.shs, None, s.scales, s.rotations, None, None, 0)
    return res[1], res[6], res[-1]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _values(P, C, seed=0):
    """Seeded signed values [P, C], float32 (host)."""
    return torch.from_numpy(np.random.default_rng(100 + seed).uniform(-2.0, 2.0, size=(P, C)).astype(np.float32))


def _paint(call, values, **kw):
    from diff_gaussian_rasterization import _C
    got = _C.raster_values(call, values, **kw)
    torch.cuda.synchronize()
    return got


# ---- against the spec ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.CASES) + ["centred_row"])
def test_painted_values_match_the_spec(gpu, name):
    cam, scene, view, _ = ps.case(name)
    frag = view.out.fragile.reshape(-1)
    assert frag.mean() <= pa.FRAGILE_FRAC, f"fragile share {frag.mean():.2e}"
    ok = ~frag
    _, _, call = _forward(gpu, cam, scene)
    H, W = cam.image_height, cam.image_width
    for Cn in (1, 3, 4):
        v = _values(scene.P, Cn, seed=Cn)
        for bg in (None, BG[:Cn]):
            out, wsum = _paint(call, v.to(gpu), background=bg, want_wsum=True)
            assert out.shape == (Cn, H, W) and out.dtype == torch.float32 and wsum.shape == (H, W)
            ref, ref_w, aabs = vs.fold_values(view, v.numpy(), background=bg)
            dev = out.cpu().numpy().astype(np.float64).reshape(Cn, -1).T
            ratios = []
            for c in range(Cn):
                bound = pa.MIXED_REL * aabs[:, c] + pa.MIXED_ABS * aabs[:, c].max()
                err = np.abs(dev[:, c] - ref[:, c])
                ratios.append(float((err[ok] / bound[ok]).max()))
            print(f"{name} C={Cn} bg={bg is not None}: largest err / bound per channel {[round(x, 3) for x in ratios]}")
            assert max(ratios) <= 1.0, (name, Cn, ratios)
            dw = np.abs(wsum.cpu().numpy().astype(np.float64).reshape(-1) - ref_w)
            assert bool((dw[ok] <= pa.MIXED_REL * ref_w[ok] + pa.MIXED_ABS * ref_w.max()).all())


# ---- against K6 itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.CASES) + ["centred_row"])
def test_the_forwards_own_colours_paint_the_forwards_image_bit_for_bit(gpu, name):
    """Every pixel, the fragile ones included: the colour and inverse-depth words of K1's records, read in place (a
    column slice of the [P, 16] records: row stride 16), give the bits of out_color and out_invdepth."""
    from diff_gaussian_rasterization import _C
    cam, scene, _, _ = ps.case(name)
    for bg3 in (torch.zeros(3), torch.tensor(BG[:3])):
        color, invdepth, call = _forward(gpu, cam, scene, bg=bg3, do_depth=True)
        words = _C.raster_views(call)["records"][:, 6:10]            # (r, g) of the second float4, (b, 1/z) of the third
        assert words.stride() == (16, 1)
        bg4 = None if not bool(bg3.any()) else tuple(bg3.tolist()) + (0.0,)      # K6 adds no background to the depth
        out = _paint(call, words, background=bg4)
        assert torch.equal(_bits(out[:3]), _bits(color)), name
        assert torch.equal(_bits(out[3]), _bits(invdepth[0])), name
        assert bool((color != bg3.to(gpu)[:, None, None]).any())


# ---- against f-22 and f-24 on the same forward ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_tiles_b", "long_lists", "big_rows"])
def test_painting_agrees_with_the_scores_and_the_readout_of_the_same_forward(gpu, name):
    from diff_gaussian_rasterization import _C
    from hgs.importance import Scores
    cam, scene, _, _ = ps.case(name)
    P = scene.P
    _, _, call = _forward(gpu, cam, scene)
    sc = Scores.zeros(P, gpu)
    _C.raster_contributions(call, sc.wmax, sc.wsum, sc.count)
    count = _C.raster_pixels(call, want=("count",))["count"]
    rows = sc.count.argsort(descending=True)[:4]                    # four rows that are blended somewhere
    assert int(sc.count[rows].min()) > 0
    onehot = torch.zeros(P, 4, device=gpu)
    onehot[rows, torch.arange(4, device=gpu)] = 1.0
    bg = torch.tensor(BG[:1], device=gpu)
    ones, wsum = _paint(call, torch.ones(P, device=gpu), want_wsum=True)
    with_bg = _paint(call, _values(P, 1).to(gpu), background=bg)
    hot = _paint(call, onehot)
    none = count == 0
    assert bool((_bits(with_bg[0])[none] == _bits(bg)[0]).all()) and not bool(_bits(wsum)[none].any())
    assert torch.equal(_bits(ones[0]), _bits(wsum))                 # a channel of ones IS the weight sum
    assert bool((wsum[~none] > 0).all())
    assert torch.equal((hot != 0).reshape(4, -1).sum(dim=1), sc.count[rows])
    total = hot.double().reshape(4, -1).sum(dim=1)
    bound = pa.MIXED_REL * sc.wsum[rows] + pa.MIXED_ABS * sc.wsum.max()
    assert bool(((total - sc.wsum[rows]).abs() <= bound).all()), (total, sc.wsum[rows])


# ---- NaN poison ----------------------------------------------------------------------------------------------------------
def test_values_of_rows_that_are_blended_nowhere_reach_no_pixel(gpu):
    """``long_lists``: 4 000 rows on 64 x 64 pixels, most pixels saturated -- rows that stand in a tile's list and are
    blended at no pixel are what the case is made of."""
    from diff_gaussian_rasterization import _C
    from hgs.importance import Scores
    cam, scene, _, _ = ps.case("long_lists")
    P = scene.P
    _, _, call = _forward(gpu, cam, scene)
    sc = Scores.zeros(P, gpu)
    _C.raster_contributions(call, sc.wmax, sc.wsum, sc.count)
    unseen = sc.count == 0
    listed = _C.raster_views(call)["tiles_touched"] > 0
    assert int((unseen & listed).sum()) > 0, "rows that are in a list and blended nowhere are what the case is about"
    v = _values(P, 3).to(gpu)
    clean = _paint(call, v, background=BG[:3])
    for poison in (float("nan"), float("inf")):
        bad = v.clone()
        bad[unseen] = poison
        assert torch.equal(_bits(_paint(call, bad, background=BG[:3])), _bits(clean)), poison
    # and a NaN in a row that IS blended shows at exactly the pixels the row is blended at
    row = int(sc.count.argmax())
    bad = v.clone()
    bad[row, 1] = float("nan")
    got = _paint(call, bad, background=BG[:3])
    assert int(torch.isnan(got[1]).sum()) == int(sc.count[row]) and not bool(torch.isnan(got[[0, 2]]).any())


# ---- slot maps -----------------------------------------------------------------------------------------------------------
def test_slot_maps_permute_the_table_and_ignored_rows_add_nothing(gpu):
    cam, scene, _, _ = ps.case("edge_tiles_a")
    P, S = scene.P, scene.P + 37
    _, _, call = _forward(gpu, cam, scene)
    v = torch.cat((_values(P, 2), torch.ones(P, 1)), dim=1).to(gpu)          # the last channel: ones
    base, base_w = _paint(call, v, background=BG[:3], want_wsum=True)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(S)[:P].astype(np.int32)).to(gpu)
    table = torch.full((S, 3), float("nan"), device=gpu)                     # slots no row names are never read
    table[perm.long()] = v
    got, got_w = _paint(call, table, slot_of_row=perm, background=BG[:3], want_wsum=True)
    assert torch.equal(_bits(got), _bits(base)) and torch.equal(_bits(got_w), _bits(base_w))
    r = torch.arange(P, device=gpu)
    for dropped, slot in ((r % 2 == 0, torch.where(r % 2 == 0, -1, perm.long()).to(torch.int32)),
                          (r % 3 != 0, torch.where(r % 3 != 0, S + 5, perm.long()).to(torch.int32)),
                          (r % 5 == 1, torch.where(r % 5 == 1, S, perm.long()).to(torch.int32))):
        zeroed = v.clone()
        zeroed[dropped] = 0.0
        want = _paint(call, zeroed, background=BG[:3])
        poisoned = table.clone()
        poisoned[perm.long()[dropped]] = float("nan")                        # an ignored row's values are never read
        got, got_w = _paint(call, poisoned, slot_of_row=slot, background=BG[:3], want_wsum=True)
        assert torch.equal(_bits(got), _bits(want))
        # wsum drops exactly those rows: it is the ones channel of the zeroed call, less than the full sum somewhere
        full_ones = _paint(call, zeroed[:, 2].contiguous())
        assert torch.equal(_bits(got_w), _bits(full_ones[0]))
        assert bool((got_w <= base_w).all()) and bool((got_w < base_w).any())


# ---- channel groups ------------------------------------------------------------------------------------------------------
def test_seven_channels_of_a_wider_table_are_seven_single_channel_calls(gpu):
    cam, scene, _, _ = ps.case("edge_tiles_b")
    P = scene.P
    _, _, call = _forward(gpu, cam, scene)
    table = _values(P, 9, seed=9).to(gpu)
    bg = torch.tensor([0.5, -1.0, 2.0, 0.0, 0.25, -0.125, 3.0], device=gpu)
    v = table[:, :7]
    assert v.stride() == (9, 1) and v.data_ptr() == table.data_ptr()         # read in place, no copy
    out, wsum = _paint(call, v, background=bg, want_wsum=True)
    assert out.shape == (7, cam.image_height, cam.image_width)
    for c in range(7):
        one, w1 = _paint(call, table[:, c], background=bg[c:c + 1], want_wsum=True)
        assert torch.equal(_bits(one[0]), _bits(out[c])), c
        assert torch.equal(_bits(w1), _bits(wsum))
    # a later group starts inside the table: channels 2..8 of the same rows
    out2 = _paint(call, table[:, 2:])
    assert torch.equal(_bits(out2[4]), _bits(_paint(call, table[:, 6])[0]))


# ---- guards ------------------------------------------------------------------------------------------------------------
def _through_the_abi(gpu, call, fill, values, Cn, bg=None, args=None, slot=None, n_slots=None, L=None, want_wsum=True):
    """``out`` [Cn, H*W] and ``wsum`` [H*W] between guard words, pre-filled with ``fill``, written by one call."""
    HW = call.H * call.W
    out, ws = wg.guarded(Cn * HW * 4, gpu, fill, "out"), wg.guarded(HW * 4, gpu, fill, "wsum")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = _lib.lib().hgs_raster_values(C.byref(call.args if args is None else args), call.p_geom, call.p_bin, call.p_img,
                                      call.L_ws if L is None else L, p(values), values.stride(0), Cn, p(slot),
                                      values.shape[0] if n_slots is None else n_slots, p(bg), C.c_void_p(out.addr),
                                      C.c_void_p(ws.addr) if want_wsum else None,
                                      C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream), gpu.index or 0)
    _lib.check(rc, "hgs_raster_values")
    wg.check(out, ws)
    return out.view(torch.int32).clone().view(Cn, HW), ws.view(torch.int32).clone()


@pytest.mark.parametrize("name", ["1x1", "5x3", "edge_tiles_a"])
@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_planes_stay_inside_their_buffers_and_repeat_their_bits(gpu, name, fill):
    """H * W off the 64 and 256 grids: the planes exactly sized between guard words; every pixel is written whatever
    the planes held before, two runs and the glue's own buffers give equal bits."""
    cam, scene, _, _ = ps.case(name)
    _, _, call = _forward(gpu, cam, scene)
    HW = call.H * call.W
    for Cn in (1, 3, 4):
        v = _values(scene.P, Cn, seed=Cn).to(gpu)
        bg = torch.tensor(BG[:Cn], device=gpu)
        a, aw = _through_the_abi(gpu, call, fill, v, Cn, bg)
        b, bw = _through_the_abi(gpu, call, fill, v, Cn, bg)
        out, wsum = _paint(call, v, background=bg, want_wsum=True)
        assert torch.equal(a, b) and torch.equal(aw, bw)
        assert torch.equal(a, _bits(out).reshape(Cn, HW)) and torch.equal(aw, _bits(wsum).reshape(-1))
        # without wsum the other plane keeps its fill; without a background the bits are those of a zero background
        c, cw = _through_the_abi(gpu, call, fill, v, Cn, None, want_wsum=False)
        assert bool((cw == (0 if fill == 0 else -1)).all())
        z, _ = _through_the_abi(gpu, call, fill, v, Cn, torch.zeros(Cn, device=gpu))
        assert torch.equal(c, z)


def test_nothing_rendered_paints_the_background(gpu):
    cam, scene, _, _ = pa.default_case(100, 40, 30, 3)
    scene.means3D[:, 2] = -scene.means3D[:, 2]                 # behind the camera
    _, _, call = _forward(gpu, cam, scene)
    assert call.L == 0
    v = torch.full((scene.P, 3), float("nan"), device=gpu)     # never read
    bg = torch.tensor(BG[:3], device=gpu)
    out, wsum = _paint(call, v, background=bg, want_wsum=True)
    assert torch.equal(_bits(out), _bits(bg[:, None, None].expand_as(out))) and not bool(_bits(wsum).any())
    assert not bool(_bits(_paint(call, v)).any())
    for fill in (0x00, 0xFF):
        a, aw = _through_the_abi(gpu, call, fill, v, 3, bg)
        assert torch.equal(a, _bits(bg)[:, None].expand_as(a)) and not bool(aw.any())
    # L == 0 and P == 0 through the ABI on a frame that does show rows: no workspace is read
    cam, scene, _, _ = ps.case("5x3")
    _, _, call = _forward(gpu, cam, scene)
    v = torch.full((scene.P, 3), float("nan"), device=gpu)
    a0 = _lib.RasterArgs.from_buffer_copy(call.args)
    a0.P = 0
    for kw in (dict(L=0), dict(args=a0)):
        a, aw = _through_the_abi(gpu, call, 0xFF, v, 3, bg, **kw)
        assert torch.equal(a, _bits(bg)[:, None].expand_as(a)) and not bool(aw.any())


# ---- the in-op LOD route -----------------------------------------------------------------------------------------------
def test_in_op_lod_route_equals_the_gathered_rows_and_the_per_pixel_remap_is_refused(gpu):
    """The cut of hier2000() at 3 px with 7 skybox rows behind it: the in-op LOD forward (default slot map: the cut's
    render_indices, values per NODE) against the plain forward of the same rows gathered by hand under an explicit map."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    from hgs.importance import activated, tau_of, view_cut
    from hgs.painting import paint_view
    K = 7
    hd, cam = cc.on_device(cc.hier2000(), gpu), cc.camera()
    N = hd.num_nodes
    ri, pi, w, kids = view_cut(hd, cam, tau_of(3.0, cam.tanfovx, cam.image_width), frustum=False)
    n = int(ri.numel())
    assert 0 < n < N
    sky = synth.make_scene(K, cam, seed=77, s_px=(6.0, 20.0), z_range=(25.0, 40.0)).to(gpu)
    rows = activated(hd)
    full = {k: torch.cat((rows[k], getattr(sky, k))).contiguous() for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    gm, gs, gr, gsh, gop = _C.lod_gather(ri, pi, w, full["means3D"], full["scales"], full["rotations"], full["shs"],
                                         full["opacities"])
    tail = lambda a, b: torch.cat((a, b[N:])).contiguous()
    gathered = dict(means3D=tail(gm, full["means3D"]), shs=tail(gsh, full["shs"]), opacities=tail(gop, full["opacities"]),
                    scales=tail(gs, full["scales"]), rotations=tail(gr, full["rotations"]))
    wa = torch.cat((w, torch.ones(K, device=gpu)))
    ka = torch.cat((kids, torch.ones(K, dtype=torch.int32, device=gpu)))
    e_i = torch.empty(0, dtype=torch.int32, device=gpu)

    def settings(r, p, ww, kk):
        kw = pa.settings_kwargs(cam, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=ww, num_node_kids=kk)
        kw["render_indices"], kw["parent_indices"] = r, p
        return dgr.GaussianRasterizationSettings(**kw)

    v = _values(N, 2, seed=5).to(gpu)                          # one row per NODE
    slot = torch.cat((ri, torch.full((K,), -1, dtype=torch.int32, device=gpu)))
    a, aw, call_a = paint_view(settings(ri.contiguous(), pi.contiguous(), w.contiguous(), kids.contiguous()), v, **full,
                               background=BG[:2], want_wsum=True, skybox_points=K)
    b, bw, call_b = paint_view(settings(e_i, e_i, wa, ka), v, **gathered, slot_of_row=slot, background=BG[:2], want_wsum=True)
    # the same rows without a map: the table gathered by hand, the skybox rows' values zero
    byrow = torch.cat((v[ri.long()], torch.zeros(K, 2, device=gpu)))
    c, cw, _ = paint_view(settings(e_i, e_i, wa, ka), byrow, **gathered, background=BG[:2], want_wsum=True)
    torch.cuda.synchronize()
    assert call_b.P == n + K
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(aw), _bits(bw))
    assert torch.equal(_bits(a), _bits(c))
    assert bool((aw <= cw).all()) and bool((aw < cw).any()), "the skybox must be on screen for the case to mean anything"
    # lod_per_pixel = 1 is refused before any HIP call, the planes untouched
    args = _lib.RasterArgs.from_buffer_copy(call_a.args)
    args.lod_per_pixel = 1
    with pytest.raises(_lib.HgsError, match="lod_per_pixel"):
        _through_the_abi(gpu, call_a, 0xFF, v, 2, None, args=args, slot=slot)


# ---- the Python layers ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hier():
    return cc.on_device(cc.hier2000(), torch.device("cuda:0"))


def test_normalized_levels_lie_between_the_levels_a_pixel_shows(gpu):
    from hgs.painting import node_levels, paint_hierarchy_view
    from hgs.picking import read_hierarchy_view
    # the camera of the hierarchy's scene turned 0.6 rad about the vertical: the scene fills one side of the picture
    # and leaves the other empty, with pixels of one and two rows along its edge
    yaw = 0.6
    h = _hier()
    cam = synth.make_camera(cc.W, cc.H, R=[[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]])
    lv = node_levels(h.nodes)
    few = 0
    for tau_px in (0.0, 6.0):
        r = read_hierarchy_view(h, cam, tau_px=tau_px, want=("count", "front", "back"))
        img = paint_hierarchy_view(h, cam, lv, tau_px=tau_px, normalize=True, fill=-7.0)
        torch.cuda.synchronize()
        assert img.shape == (1, cam.image_height, cam.image_width) and img.dtype == torch.float32
        some = r.count > 0
        assert int(some.sum()) > 300 and int((~some).sum()) > 0
        assert bool((img[0][~some] == -7.0).all())
        # a weighted mean lies between the smallest and the largest level among the ids the readout names, front to
        # back, on the pixels that show a row.  Rounding: the two float32 sums of n <= count.max() terms each carry at
        # most n 2^-24 of their size, the quotient twice that of the largest level
        shown = torch.cat((r.front[some], r.back[some])).long()
        lo, hi = float(lv[shown].min()), float(lv[shown].max())
        tol = 2.0 * int(r.count.max()) * 2.0 ** -24 * hi + 1e-6
        got = img[0][some]
        print(f"tau_px {tau_px}: levels {lo} .. {hi}, painted {float(got.min())} .. {float(got.max())}, tol {tol:.2e}")
        assert bool((got >= lo - tol).all()) and bool((got <= hi + tol).all())
        # per pixel where front and back are all its rows: one row shows its own level, two rows a level between theirs
        one, two = r.count == 1, r.count == 2
        few += int(one.sum()) + int(two.sum())
        want = lv[r.front[one].long()]
        assert bool(((img[0][one] - want).abs() <= tol).all())
        a, b = lv[r.front[two].long()], lv[r.back[two].long()]
        g = img[0][two]
        assert bool((g >= torch.minimum(a, b) - tol).all()) and bool((g <= torch.maximum(a, b) + tol).all())
    assert few > 0
    # without normalize: the plain blend, NaN as the default fill, a background behind it
    plain = paint_hierarchy_view(h, cam, lv, tau_px=6.0, background=2.0)
    mean = paint_hierarchy_view(h, cam, lv, tau_px=6.0, normalize=True)
    r = read_hierarchy_view(h, cam, tau_px=6.0, want=("count", "alpha"))
    assert bool(torch.isnan(mean[0][r.count == 0]).all()) and not bool(torch.isnan(mean[0][r.count > 0]).any())
    assert bool((plain[0][r.count == 0] == 2.0).all())
    two_ch = paint_hierarchy_view(h, cam, torch.stack((lv, -lv), dim=1), tau_px=6.0)
    assert two_ch.shape[0] == 2 and torch.equal(two_ch[1], -two_ch[0]) and bool((two_ch[0] > 0).any())
    with pytest.raises(ValueError):
        paint_hierarchy_view(h, cam, lv[:-1])


def test_command_writes_the_image_of_the_python_call(gpu, tmp_path, capsys):
    from gaussian_hierarchy._C import write_hierarchy
    from hgs import paint_hierarchy as ph
    from hgs.painting import error_per_weight, node_extents, paint_hierarchy_view
    from hgs.score_hierarchy import read_cameras
    host = cc.hier2000()
    N = host.num_nodes
    path, cams = tmp_path / "in.hier", tmp_path / "cameras.json"
    write_hierarchy(str(path), *[getattr(host, k) for k in cc.FIELDS])
    cams.write_text(json.dumps([cc.camera_entry(c) for c in cc.orbit(2)]))
    cam = read_cameras(str(cams))[1]
    h = _hier()
    base = [str(path), "--cameras", str(cams), "--camera", "1"]
    # a built-in, normalized
    out = tmp_path / "o" / "extent.npy"
    rc = ph.main(base + ["--builtin", "extent", "--tau-px", "3", "--normalize", "--out", str(out)])
    said = capsys.readouterr().out
    assert rc == 0 and said.startswith(f"paint_hierarchy: N = {N} nodes, camera 1 (64 x 48) at 3 px") and "normalized" in said
    want = paint_hierarchy_view(h, cam, node_extents(h.boxes), tau_px=3.0, normalize=True)
    got = np.load(out)
    assert got.dtype == np.float32 and got.shape == (1, 48, 64)
    assert np.array_equal(got.view(np.int32), want.cpu().numpy().view(np.int32))
    # a value file with two channels and a background
    v = _values(N, 2, seed=3)
    vals = tmp_path / "v.npy"
    np.save(vals, v.numpy())
    out = tmp_path / "values.npy"
    rc = ph.main(base + ["--values", str(vals), "--background", "0.5", "-1", "--no-frustum", "--out", str(out)])
    assert rc == 0 and "2 channels" in capsys.readouterr().out
    want = paint_hierarchy_view(h, cam, v, frustum=False, background=(0.5, -1.0))
    assert np.array_equal(np.load(out).view(np.int32), want.cpu().numpy().view(np.int32))
    # the file python -m hgs.lod_error writes
    rng = np.random.default_rng(8)
    err = dict(err=rng.uniform(0.0, 1.0, N), wsum=rng.uniform(0.5, 2.0, N), entries=np.ones(N, dtype=np.int64), views=np.int64(1))
    npz, out = tmp_path / "e.npz", tmp_path / "err.npy"
    np.savez(npz, **err)
    rc = ph.main(base + ["--lod-error", str(npz), "--tau-px", "3", "--out", str(out)])
    assert rc == 0 and "err / wsum" in capsys.readouterr().out
    want = paint_hierarchy_view(h, cam, error_per_weight(err), tau_px=3.0)
    assert np.array_equal(np.load(out).view(np.int32), want.cpu().numpy().view(np.int32))
    # values of another length: named, exit 1, nothing written
    np.save(vals, v.numpy()[:-1])
    out = tmp_path / "short.npy"
    rc = ph.main(base + ["--values", str(vals), "--out", str(out)])
    assert rc == 1 and "nothing written" in capsys.readouterr().err and not out.exists()
