"""The per-pixel readout without a GPU: the float64 spec (tests/pixels_spec.py) against the oracle itself, the torch
statements of hgs.picking on hand-built tensors, the refusals of hgs_raster_pixels and of its Python glue, the export,
and the command's parser and exits."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import pixels_spec as ps
from hgs import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hierarchical-3d-gaussians_amd")


# ---- the spec against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_tile", "edge_tiles_a", "opaque_stack", "5x3"])
def test_spec_agrees_with_the_oracles_own_image(name):
    cam, scene, view, spec = ps.case(name)
    fT = np.asarray(view.out.final_T, dtype=np.float64).reshape(-1)
    assert np.abs(spec.alpha - (1.0 - fT)).max() <= 1e-12
    total = 0
    sw, tb, ta = spec.of_row(spec.back)                    # what the spec says about each pixel's last row
    for flat, ids, w, keep in view.pix:
        assert np.array_equal(spec.n[flat], keep.sum(axis=1))
        total += int(keep.sum())
        for p in range(flat.size):
            kept = ids[keep[p]]
            f = flat[p]
            assert spec.front[f] == (kept[0] if kept.size else ps.NONE)
            assert spec.back[f] == (kept[-1] if kept.size else ps.NONE)
            if kept.size:
                ww = w[p][keep[p]]
                assert spec.heaviest[f] == kept[int(np.argmax(ww))] and spec.wmax[f] == ww.max()
                T = 1.0 - np.cumsum(ww)
                below = np.flatnonzero(T < 0.5)
                assert spec.median[f] == (kept[below[0]] if below.size else ps.NONE)
                assert sw[f] == ww[-1] and ta[f] == T[-1] and abs(tb[f] - (T[-2] if kept.size > 1 else 1.0)) <= 1e-15
            else:
                assert np.isnan(sw[f])
    assert int(spec.n.sum()) == total and total > 0
    assert bool(((spec.n == 0) == (spec.front == ps.NONE)).all()) and bool((spec.wmax[spec.n == 0] == 0).all())
    assert bool((spec.second <= spec.wmax).all())
    if name == "opaque_stack":
        assert int((spec.median != ps.NONE).sum()) > 50          # the median within the first rows of the stack


def test_map_ids_names_slots_and_ignored_rows():
    ids = np.array([-1, 0, 1, 2, 3])
    assert ps.map_ids(ids).tolist() == [-1, 0, 1, 2, 3]
    assert ps.map_ids(ids, [7, -1, 9, 3], n_slots=9).tolist() == [-1, 7, -2, -2, 3]
    assert ps.map_ids(ids, [7, -1, 9, 3]).tolist() == [-1, 7, -2, 9, 3]


# ---- hgs.picking on hand-built tensors ---------------------------------------------------------------------------------
def _tree7():
    """root 0 -> (1, 2); 1 -> (3, 4); 2 -> (5, 6): depth, parent, start, count_leafs, count_merged, start_children, count_children"""
    return torch.tensor([[0, -1, 0, 4, 0, 1, 2], [1, 0, 0, 2, 0, 3, 2], [1, 0, 0, 2, 0, 5, 2], [2, 1, 0, 1, 0, 0, 0],
                         [2, 1, 0, 1, 0, 0, 0], [2, 2, 0, 1, 0, 0, 0], [2, 2, 0, 1, 0, 0, 0]], dtype=torch.int32)


def _readout():
    from hgs.picking import PixelReadout
    front = torch.tensor([[3, 3, -1, 5], [4, -2, -1, 5], [1, 1, 6, 6]], dtype=torch.int32)
    median = torch.tensor([[3, -1, -1, 5], [4, -2, -1, 6], [-1, 1, 6, 2]], dtype=torch.int32)
    depth = torch.where(median == -1, torch.zeros(3, 4), torch.full((3, 4), 2.0))
    return PixelReadout(front=front, median=median, median_depth=depth, H=3, W=4)


def test_pick_takes_the_sorted_unique_named_ids_of_a_region():
    from hgs.picking import pick
    r = _readout()
    assert pick(r, (0, 0, 4, 3)).tolist() == [1, 3, 4, 5, 6] and pick(r, (0, 0, 4, 3)).dtype == torch.int64
    assert pick(r, (1, 1, 3, 2)).tolist() == []                          # -2 and -1 alone: never picked
    assert pick(r, (3, 0, 4, 3)).tolist() == [5, 6]                      # the right border column
    assert pick(r, (2, 2, 9, 9)).tolist() == [6]                         # clipped to the image
    assert pick(r, (-5, -5, 1, 1), "front").tolist() == [3]
    assert pick(r, (3, 1, 4, 3), ("front", "median")).tolist() == [2, 5, 6]
    mask = np.zeros((3, 4), dtype=np.uint8)
    mask[2, :2] = 7
    assert pick(r, mask).tolist() == [1] and pick(r, torch.from_numpy(mask).bool(), ("median",)).tolist() == [1]
    for bad in (dict(which=()), dict(which=("alpha",)), dict(which=("back",)), dict(region=np.zeros((3, 5), dtype=bool)),
                dict(region=np.zeros((3, 4), dtype=np.float32))):
        kw = dict(region=(0, 0, 1, 1), which=("front",))
        kw.update(bad)
        with pytest.raises(ValueError):
            pick(r, kw["region"], kw["which"])


def test_leaves_below_marks_exactly_the_leaves_of_the_subtrees():
    from hgs.picking import leaves_below
    nodes = _tree7()
    assert leaves_below(nodes, [1]).tolist() == [0, 0, 0, 1, 1, 0, 0]    # an interior id: exactly its leaves
    assert leaves_below(nodes, [5]).tolist() == [0, 0, 0, 0, 0, 1, 0]    # a leaf marks itself
    assert leaves_below(nodes, [0]).tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert leaves_below(nodes, torch.tensor([2, 3, 3])).tolist() == [0, 0, 0, 1, 0, 1, 1]
    m = leaves_below(nodes, [])
    assert m.dtype == torch.uint8 and m.tolist() == [0] * 7
    # any numbering: levelled by the depth column, not by the index
    perm = torch.tensor([6, 2, 4, 0, 5, 1, 3])                           # new index of old node i
    shuffled = torch.zeros_like(nodes)
    shuffled[perm] = nodes
    shuffled[:, 1] = torch.where(shuffled[:, 1] >= 0, perm[shuffled[:, 1].clamp(min=0).long()].to(torch.int32), shuffled[:, 1])
    got = leaves_below(shuffled, perm[[1]])
    assert got[perm].tolist() == [0, 0, 0, 1, 1, 0, 0]
    for bad in ([7], [-1]):
        with pytest.raises(ValueError):
            leaves_below(nodes, bad)
    with pytest.raises(ValueError):
        leaves_below(nodes[:, :6], [0])


def test_node_depth_image_and_world_points():
    from hgs import synth
    from hgs.picking import PixelReadout, node_depth_image, world_points
    r = _readout()
    d = node_depth_image(r.front, _tree7())
    assert d.dtype == torch.int32 and d.tolist() == [[2, 2, -1, 2], [2, -1, -1, 2], [1, 1, 2, 2]]
    with pytest.raises(ValueError):
        node_depth_image(torch.tensor([7]), _tree7())
    # a point in front of an orbit camera comes back from its pixel and its view-space depth
    W, H = 64, 48
    cam = synth.orbit_camera(W, H, 1, 3)
    x, y, z = 37, 11, 4.25
    ndc = lambda p, n: (2.0 * p + 1.0) / n - 1.0
    view = torch.tensor([ndc(x, W) * cam.tanfovx * z, ndc(y, H) * cam.tanfovy * z, z, 1.0], dtype=torch.float64)
    world = (view @ torch.linalg.inv(cam.world_view_transform.double()))[:3]
    median = torch.full((H, W), -1, dtype=torch.int32)
    depth = torch.zeros(H, W)
    median[y, x], depth[y, x] = 5, z
    median[0, 0], depth[0, 0] = -2, 1.0                                  # an unnamed row still has a depth
    pts = world_points(PixelReadout(median=median, median_depth=depth, H=H, W=W), cam)
    assert pts.shape == (H, W, 3) and pts.dtype == torch.float32
    assert torch.allclose(pts[y, x].double(), world, rtol=1e-5, atol=1e-5)
    assert bool(torch.isfinite(pts[0, 0]).all())
    rest = torch.ones(H, W, dtype=torch.bool)
    rest[y, x] = rest[0, 0] = False
    assert bool(torch.isnan(pts[rest]).all())
    back = torch.cat((pts[y, x].double(), torch.ones(1, dtype=torch.float64))) @ cam.world_view_transform.double()
    assert abs(float(back[2]) - z) <= 1e-5 * z
    with pytest.raises(ValueError):
        world_points(PixelReadout(median=median, H=H, W=W), cam)


def test_readout_numpy_and_nothing():
    from hgs.picking import PLANES, nothing
    r = nothing(3, 5)
    n = r.numpy()
    assert set(n) == set(PLANES) | {"H", "W"} and int(n["H"]) == 3 and int(n["W"]) == 5
    for name in ("front", "back", "heaviest", "median"):
        assert n[name].dtype == np.int32 and (n[name] == -1).all()
    assert n["count"].dtype == np.int32 and not n["count"].any()
    for name in ("alpha", "wmax", "median_depth"):
        assert n[name].dtype == np.float32 and not n[name].view(np.uint32).any()
    assert set(nothing(2, 2, want=("front",)).numpy()) == {"front", "H", "W"}


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_export_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgs.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bhgs_raster_pixels\s*\(", src) and re.search(r"\bhgs_raster_pixels\b", nm)
    assert "hgs_raster_pixels" in _lib.SIGNATURES and hasattr(_lib.lib(), "hgs_raster_pixels")
    # the struct's fields, in the header's order, are the names the glue uses
    body = re.search(r"typedef struct \{([^}]*)\} hgs_raster_pixel_planes;", src).group(1)
    assert tuple(re.findall(r"\*\s*(\w+)\s*;", body)) == _lib.PIXEL_PLANES
    assert [n for n, _ in _lib.RasterPixelPlanes._fields_] == list(_lib.PIXEL_PLANES)
    assert C.sizeof(_lib.RasterPixelPlanes) == 8 * C.sizeof(C.c_void_p)
    assert _lib.lib().hgs_abi_version() == 14


FAKE = 0x10000       # never dereferenced: every refusal happens before any HIP call


def _args(P=10, W=32, H=32):
    a = _lib.RasterArgs()
    a.P, a.M, a.sh_degree, a.width, a.height = P, 0, 0, W, H
    a.tanfovx = a.tanfovy = a.scale_modifier = 1.0
    a.bg = a.viewmatrix = a.projmatrix = a.campos = FAKE
    a.means3D = a.opacities = a.colors_precomp = a.cov3D_precomp = FAKE
    return a


def _call(a, L=100, planes="front", n_slots=10, slot=None, geom=FAKE, binb=FAKE, img=FAKE):
    lib = _lib.lib()
    out = None if planes is None else C.byref(_lib.RasterPixelPlanes(**{n: FAKE for n in ([planes] if planes else [])}))
    rc = lib.hgs_raster_pixels(C.byref(a) if a is not None else None, geom, binb, img, L, slot, n_slots, out, None, 0)
    return rc, lib.hgs_last_error().decode()


def test_every_refusal_is_invalid_with_its_message_and_needs_no_gpu():
    INVALID = 1
    for kw, word in ((dict(planes=None), "null planes"), (dict(planes=""), "null planes"),
                     (dict(slot=FAKE, n_slots=0), "n_slots = 0"), (dict(slot=FAKE, n_slots=-3), "n_slots = -3"),
                     (dict(geom=None), "null workspace"), (dict(binb=None), "null workspace"),
                     (dict(img=None), "null workspace")):
        rc, msg = _call(_args(), **kw)
        assert rc == INVALID and word in msg and "hgs_raster_pixels" in msg, (kw, rc, msg)
    assert _call(None)[0] == INVALID and "null args" in _call(None)[1]
    a = _args()
    a.lod_per_pixel = 1
    rc, msg = _call(a)
    assert rc == INVALID and "lod_per_pixel" in msg and "not built" in msg
    for field, val, word in (("P", -1, "bad sizes"), ("width", 0, "bad sizes"), ("height", -4, "bad sizes"),
                             ("width", 16369, "not supported"), ("lod_half_rows", 2, "lod_half_rows")):
        a = _args()
        setattr(a, field, val)
        rc, msg = _call(a)
        assert rc == INVALID and word in msg, (field, rc, msg)
    a = _args()
    a.bg = None
    assert _call(a)[0] == INVALID


# ---- the Python glue ---------------------------------------------------------------------------------------------------
def test_raster_pixels_refuses_bad_arguments_before_the_library(monkeypatch):
    from diff_gaussian_rasterization import _C
    touched = []
    monkeypatch.setattr(_lib, "lib", lambda: touched.append(1))
    call = types.SimpleNamespace(device=torch.device("cuda:0"), P=5, W=8, H=4, L=10, L_ws=10)
    slot = torch.zeros(5, dtype=torch.int32)
    for kw, word in ((dict(want=()), "at least one plane"), (dict(want=("front", "depth")), "unknown plane 'depth'"),
                     (dict(want="colour"), "unknown plane"), (dict(n_slots=4), "n_slots bounds slot_of_row"),
                     (dict(slot_of_row=slot), "slot_of_row must be an int32 tensor on cuda:0"),
                     (dict(slot_of_row=np.zeros(5, dtype=np.int32)), "slot_of_row must be an int32 tensor"),
                     (dict(slot_of_row=[0] * 5), "slot_of_row must be an int32 tensor")):
        with pytest.raises(RuntimeError, match=word):
            _C.raster_pixels(call, **kw)
    assert not touched
    assert _C.PIXEL_PLANES == _lib.PIXEL_PLANES


# ---- the command -------------------------------------------------------------------------------------------------------
def _run(*argv):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    return subprocess.run([sys.executable, "-m", "hgs.pick_hierarchy", *argv], capture_output=True, text=True, env=env)


def test_parse_args_good_and_bad_lines():
    from hgs import pick_hierarchy as ph
    base = ["a.hier", "--cameras", "c.json", "--camera", "2"]
    rect = base + ["--rect", "1", "2", "30", "40"]
    assert ph.parse_args(rect) == dict(
        in_path="a.hier", cameras="c.json", camera=2, rect=(1, 2, 30, 40), pixel=None, pixel_mask=None, which=("front",),
        tau_px=0.0, frustum=True, resolution_scale=1.0, ids_out=None, mask_out=None, readout_out=None)
    full = ph.parse_args(["--pixel", "5", "0", "--which", "median", "--tau-px", "3", "a.hier", "--no-frustum", "--cameras",
                          "c.json", "--which", "heaviest", "--camera", "0", "--resolution-scale", "2", "--ids-out", "i.npy",
                          "--mask-out", "m.npy", "--readout-out", "r.npz"])
    assert (full["pixel"], full["which"], full["tau_px"], full["frustum"], full["resolution_scale"], full["camera"]) == \
        ((5, 0), ("median", "heaviest"), 3.0, False, 2.0, 0)
    assert (full["ids_out"], full["mask_out"], full["readout_out"], full["rect"]) == ("i.npy", "m.npy", "r.npz", None)
    assert ph.parse_args(base + ["--pixel-mask", "m.npy"])["pixel_mask"] == "m.npy"
    assert ph.parse_args(base + ["--rect", "-4", "-4", "3", "3"])["rect"] == (-4, -4, 3, 3)
    bad = [[], base, ["--cameras", "c.json", "--camera", "0", "--pixel", "1", "1"], rect + ["b.hier"], rect + ["--bogus"],
           rect + ["--pixel", "1", "1"], rect + ["--pixel-mask", "m.npy"], rect + ["--rect", "0", "0", "1", "1"],
           base + ["--rect", "1", "2", "3"], base + ["--rect", "5", "2", "5", "9"], base + ["--rect", "5", "9", "6", "2"],
           base + ["--rect", "a", "2", "6", "9"], base + ["--rect", "0.5", "2", "6", "9"], base + ["--pixel", "-1", "0"],
           base + ["--pixel", "3"], base[:3] + ["--pixel", "1", "1"], base[:3] + ["--camera", "-1", "--pixel", "1", "1"],
           base[:3] + ["--camera", "x", "--pixel", "1", "1"], ["a.hier", "--camera", "0", "--pixel", "1", "1"],
           rect + ["--which", "alpha"], rect + ["--which", "front", "--which", "front"], rect + ["--which"],
           rect + ["--tau-px", "-1"], rect + ["--tau-px", "nan"], rect + ["--tau-px", "x"], rect + ["--resolution-scale", "0"],
           rect + ["--resolution-scale", "inf"], rect + ["--camera", "1"], rect + ["--ids-out", "a", "--ids-out", "b"]]
    for argv in bad:
        assert ph.parse_args(argv) is None, argv


def test_command_exits_two_on_usage_and_one_on_a_bad_region_and_writes_nothing(tmp_path):
    import contribution_cases as cc
    from hgs import synth
    ids = tmp_path / "ids.npy"
    for argv in ([], ["a.hier"], ["a.hier", "--cameras", "c.json", "--camera", "0"],
                 ["a.hier", "--cameras", "c.json", "--camera", "0", "--pixel", "1", "1", "--bogus"]):
        r = _run(*argv)
        assert r.returncode == 2 and r.stderr.strip().startswith("usage: python -m hgs.pick_hierarchy"), (argv, r.stderr)
    r = _run(str(tmp_path / "none.hier"), "--cameras", str(tmp_path / "c.json"), "--camera", "0", "--pixel", "1", "1")
    assert r.returncode == 2 and "does not exist" in r.stderr
    # files that exist: the region is checked against the camera before the hierarchy is read, so its faults need no GPU
    hier, cams, mask = tmp_path / "in.hier", tmp_path / "c.json", tmp_path / "m.npy"
    hier.write_bytes(b"")
    cams.write_text(json.dumps([cc.camera_entry(synth.orbit_camera(cc.W, cc.H, k, 2)) for k in range(2)]))
    line = [str(hier), "--cameras", str(cams), "--ids-out", str(ids)]
    r = _run(*line, "--camera", "2", "--pixel", "1", "1")
    assert r.returncode == 2 and "holds 2 cameras" in r.stderr
    r = _run(*line, "--camera", "1", "--pixel", str(cc.W), "0")
    assert r.returncode == 1 and "outside" in r.stderr and "nothing written" in r.stderr, r.stderr
    r = _run(*line, "--camera", "1", "--rect", str(cc.W), "0", str(cc.W + 5), "4")
    assert r.returncode == 1 and "does not meet" in r.stderr
    r = _run(*line, "--camera", "0", "--pixel-mask", str(mask))
    assert r.returncode == 2 and "does not exist" in r.stderr
    for wrong in (np.zeros((cc.H, cc.W + 1), dtype=np.uint8), np.zeros((cc.H, cc.W), dtype=np.float32)):
        np.save(mask, wrong)
        r = _run(*line, "--camera", "0", "--pixel-mask", str(mask))
        assert r.returncode == 1 and "m.npy" in r.stderr and f"[{cc.H}, {cc.W}]" in r.stderr, r.stderr
    mask.write_bytes(b"not an array")
    r = _run(*line, "--camera", "0", "--pixel-mask", str(mask))
    assert r.returncode == 1 and "m.npy" in r.stderr
    cams.write_text("[]")
    r = _run(*line, "--camera", "0", "--pixel", "1", "1")
    assert r.returncode == 2 and "non-empty list" in r.stderr
    assert not ids.exists()


# ---- kernel resources --------------------------------------------------------------------------------------------------
def test_new_kernel_has_no_scratch_and_the_neighbours_keep_their_rows():
    """From the compiler's own report (scripts/kernel_resources.py, no GPU): the readout kernel spills nothing, and it,
    the kernels of contrib.hip and attribute.hip -- the three files share the walk of csrc/tile_walk.h since f-25 and
    were rewritten onto it -- and K6 and K7 in render.hip show exactly the registers, LDS and scratch they showed
    before the walk was folded into one text (profiles/f23_attribute_kernels.md, profiles/f25_tile_walk.md)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    csrc = os.path.join(PKG, "csrc")
    rows = {r["kernel"]: r for r in kernel_resources.collect(
        [os.path.join(csrc, f) for f in ("pixels.hip", "contrib.hip", "attribute.hip", "render.hip")])}
    new = rows["pixels_tile_kernel"]
    assert new["file"] == "pixels.hip" and new["scratch"] == 0 and new["spills"] == 0 and new["wg"] == 64
    assert [k for k, r in rows.items() if r["file"] == "pixels.hip"] == ["pixels_tile_kernel"]      # one launch
    before = {                                                      # kernel: (VGPRs, LDS bytes, scratch bytes)
        "pixels_tile_kernel": (82, 2600, 0),                        # no LDS accumulators; K6's own occupancy class
        "contrib_tile_kernel": (46, 6760, 0), "contrib_sum_kernel": (34, 0, 0),
        "attribute_tile_kernel<1>": (49, 6760, 0), "attribute_tile_kernel<2>": (56, 6760, 0),
        "attribute_tile_kernel<3>": (64, 6760, 0), "attribute_sum_kernel<1>": (32, 0, 0),
        "attribute_sum_kernel<2>": (38, 0, 0), "attribute_sum_kernel<3>": (44, 0, 0),
        "render_fwd_quad_kernel<false, false>": (79, 5264, 0), "render_fwd_quad_kernel<false, true>": (80, 6304, 0),
        "render_fwd_quad_kernel<true, false>": (80, 5264, 0), "render_fwd_quad_kernel<true, true>": (80, 6304, 0),
        "render_bwd_quad_kernel<false, false>": (123, 9360, 0), "render_bwd_quad_kernel<false, true>": (123, 10240, 0),
        "render_bwd_quad_kernel<true, false>": (128, 9360, 0), "render_bwd_quad_kernel<true, true>": (128, 10240, 0)}
    for k, want in before.items():
        r = rows[k]
        assert (r["vgpr"] + r["agpr"], r["lds"], r["scratch"]) == want, (k, r["vgpr"] + r["agpr"], r["lds"], r["scratch"])
