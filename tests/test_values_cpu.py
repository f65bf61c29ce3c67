"""The value painting without a GPU: the float64 spec (tests/values_spec.py) against the oracle's own image, the makers
of per-node values on hand-built tensors, the refusals of hgs_raster_values and of its Python glue, the export, the
command's parser and exits, and the compiler's report on the new kernel."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import contribution_spec as cs
import pixels_spec as ps
import values_spec as vs
from hgs import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hierarchical-3d-gaussians_amd")


# ---- the spec against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_tile", "5x3", "edge_tiles_a"])
def test_spec_with_the_oracles_colours_is_the_oracles_image(name):
    """v = the colours the oracle blends, bg = its background: the fold of the captured weights IS its image."""
    cam, scene = ps.CASES[name]()
    rng = np.random.default_rng(11)
    colours = torch.from_numpy(rng.uniform(-1.0, 2.0, size=(scene.P, 3)))
    bg = torch.tensor([0.1, 0.7, 0.3], dtype=torch.float64)
    view = cs.oracle_view(scene, cam, bg=bg, colors_precomp=colours)
    out, wsum, aabs = vs.fold_values(view, colours.numpy(), background=bg.numpy())
    image = view.out.color.detach().numpy().reshape(3, -1).T
    assert np.abs(out - image).max() <= 1e-12
    fT = np.asarray(view.out.final_T, dtype=np.float64).reshape(-1)
    assert np.abs(wsum - (1.0 - fT)).max() <= 1e-12                 # every row named: the weights add up to 1 - T
    assert bool((aabs >= np.abs(out) - 1e-15).all()) and float(wsum.max()) > 0.5
    # a slot map: the permuted table read through it is the same image; ignored rows leave the sum and stay in T
    S = scene.P + 5
    perm = rng.permutation(S)[:scene.P]
    table = np.zeros((S, 3))
    table[perm] = colours.numpy()
    again, wsum2, _ = vs.fold_values(view, table, slot_of_row=perm, background=bg.numpy())
    assert np.array_equal(again, out) and np.array_equal(wsum2, wsum)
    drop = np.arange(scene.P) % 3 == 0
    zeroed = colours.numpy().copy()
    zeroed[drop] = 0.0
    want, _, _ = vs.fold_values(view, zeroed, background=bg.numpy())
    for bad in (-1, S + 2):
        got, w3, _ = vs.fold_values(view, table, slot_of_row=np.where(drop, bad, perm), n_slots=S, background=bg.numpy())
        assert np.array_equal(got, want) and bool((w3 <= wsum).all()) and bool((w3 < wsum).any())
    one, _, _ = vs.fold_values(view, colours.numpy()[:, 1])
    assert one.shape == (view.W * view.H, 1) and np.abs(one[:, 0] - (out[:, 1] - fT * 0.7)).max() <= 1e-12


# ---- the makers of per-node values -------------------------------------------------------------------------------------
def _tree7():
    """root 0 -> (1, 2); 1 -> (3, 4); 2 -> (5, 6): depth, parent, start, count_leafs, count_merged, start_children, count_children"""
    return torch.tensor([[0, -1, 0, 4, 0, 1, 2], [1, 0, 0, 2, 0, 3, 2], [1, 0, 0, 2, 0, 5, 2], [2, 1, 0, 1, 0, 0, 0],
                         [2, 1, 0, 1, 0, 0, 0], [2, 2, 0, 1, 0, 0, 0], [2, 2, 0, 1, 0, 0, 0]], dtype=torch.int32)


def test_makers_of_per_node_values():
    from hgs.importance import Attribution
    from hgs.painting import error_per_weight, node_extents, node_levels, node_opacities
    lv = node_levels(_tree7())
    assert lv.dtype == torch.float32 and lv.tolist() == [0, 1, 1, 2, 2, 2, 2]
    boxes = torch.zeros(7, 2, 4)
    boxes[:, 0, 3] = torch.arange(7, dtype=torch.float32) * 0.5
    assert node_extents(boxes).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    h = types.SimpleNamespace(alpha=torch.tensor([[0.5], [-0.25], [1.0], [0.0], [0.1], [0.2], [0.3], [0.9], [0.9]]),
                              num_nodes=7)
    op = node_opacities(h)
    assert op.shape == (7,) and op.tolist()[:3] == [0.5, 0.25, 1.0]                # |alpha| of the N node rows
    att = Attribution(acc=torch.tensor([[2.0], [0.0], [3.0]], dtype=torch.float64),
                      wsum=torch.tensor([4.0, 0.0, 1.5], dtype=torch.float64), entries=torch.ones(3, dtype=torch.int64), views=1)
    e = error_per_weight(att)
    assert e.dtype == torch.float32 and e[0] == 0.5 and math.isnan(float(e[1])) and e[2] == 2.0
    z = error_per_weight(dict(err=np.array([2.0, 0.0, 3.0]), wsum=np.array([4.0, 0.0, 1.5])))     # the .npz of lod_error
    assert torch.equal(torch.nan_to_num(z, nan=-1.0), torch.nan_to_num(e, nan=-1.0))
    for bad in (lambda: node_levels(torch.zeros(3, 6)), lambda: node_extents(torch.zeros(3, 8)),
                lambda: error_per_weight(dict(err=np.zeros(3), wsum=np.zeros(4)))):
        with pytest.raises(ValueError):
            bad()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_export_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgs.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bhgs_raster_values\s*\(", src) and re.search(r"\bhgs_raster_values\b", nm)
    assert "hgs_raster_values" in _lib.SIGNATURES and hasattr(_lib.lib(), "hgs_raster_values")
    restype, argtypes = _lib.SIGNATURES["hgs_raster_values"]
    decl = re.search(r"int hgs_raster_values\((.*?)\);", src, flags=re.S).group(1)
    assert restype is C.c_int and len(argtypes) == len(decl.split(",")) == 15
    assert _lib.lib().hgs_abi_version() == 14                       # additive: the version stays


FAKE = 0x10000       # never dereferenced: every refusal happens before any HIP call


def _args(P=10, W=32, H=32):
    a = _lib.RasterArgs()
    a.P, a.M, a.sh_degree, a.width, a.height = P, 0, 0, W, H
    a.tanfovx = a.tanfovy = a.scale_modifier = 1.0
    a.bg = a.viewmatrix = a.projmatrix = a.campos = FAKE
    a.means3D = a.opacities = a.colors_precomp = a.cov3D_precomp = FAKE
    return a


def _call(a, L=100, values=FAKE, stride=4, channels=3, slot=None, n_slots=10, bg=None, out=FAKE, wsum=None, geom=FAKE,
          binb=FAKE, img=FAKE):
    lib = _lib.lib()
    rc = lib.hgs_raster_values(C.byref(a) if a is not None else None, geom, binb, img, L, values, stride, channels, slot,
                               n_slots, bg, out, wsum, None, 0)
    return rc, lib.hgs_last_error().decode()


def test_every_refusal_is_invalid_with_its_message_and_needs_no_gpu():
    INVALID = 1
    for kw, word in ((dict(channels=0), "channels = 0"), (dict(channels=5), "channels = 5"),
                     (dict(channels=-1), "channels = -1"), (dict(stride=2), "value_stride = 2 < channels = 3"),
                     (dict(stride=0, channels=1), "value_stride = 0"), (dict(values=None), "null values"),
                     (dict(out=None), "null output"), (dict(n_slots=0), "n_slots = 0"),
                     (dict(slot=FAKE, n_slots=-3), "n_slots = -3"), (dict(n_slots=9), "n_slots = 9 < P = 10"),
                     (dict(geom=None), "null workspace"), (dict(binb=None), "null workspace"),
                     (dict(img=None), "null workspace")):
        rc, msg = _call(_args(), **kw)
        assert rc == INVALID and word in msg and "hgs_raster_values" in msg, (kw, rc, msg)
    assert _call(None)[0] == INVALID and "null args" in _call(None)[1]
    a = _args()
    a.lod_per_pixel = 1
    rc, msg = _call(a)
    assert rc == INVALID and "lod_per_pixel" in msg and "not built" in msg and "hgs_raster_values" in msg
    for field, val, word in (("P", -1, "bad sizes"), ("width", 0, "bad sizes"), ("lod_half_rows", 2, "lod_half_rows")):
        a = _args()
        setattr(a, field, val)
        rc, msg = _call(a)
        assert rc == INVALID and word in msg, (field, rc, msg)


# ---- the Python glue ---------------------------------------------------------------------------------------------------
def test_raster_values_refuses_bad_arguments_before_the_library(monkeypatch):
    from diff_gaussian_rasterization import _C
    touched = []
    monkeypatch.setattr(_lib, "lib", lambda: touched.append(1))
    dev = torch.device("cuda:0")
    call = types.SimpleNamespace(device=dev, P=5, W=8, H=4, L=10, L_ws=10)
    for kw, word in ((dict(values=torch.zeros(5, 3)), "values must be a tensor on the forward's device"),
                     (dict(values=np.zeros((5, 3), dtype=np.float32)), "values must be a tensor"),
                     (dict(values=None), "values must be a tensor")):
        with pytest.raises(RuntimeError, match=word):
            _C.raster_values(call, **kw)
    assert not touched
    assert _C.VALUE_CHANNELS == 4
    # what follows the device check is checked on a stand-in whose tensors claim the forward's device
    cpu = types.SimpleNamespace(device=torch.device("cpu"), P=5, W=8, H=4, L=10, L_ws=10)

    class OnForwardDevice(torch.Tensor):
        is_cuda = True

    t = lambda x: x.as_subclass(OnForwardDevice)
    slot = torch.zeros(5, dtype=torch.int32)
    for kw, word in ((dict(values=t(torch.zeros(5, 3, dtype=torch.float64))), "float32 tensor"),
                     (dict(values=t(torch.zeros(5, 3, 2))), r"\[S, C\]"),
                     (dict(values=t(torch.zeros(0, 3))), "at least one slot"),
                     (dict(values=t(torch.zeros(3, 5).t())), "contiguous rows"),
                     (dict(values=t(torch.zeros(4, 3))), "4 slots for 5 op rows"),
                     (dict(values=t(torch.zeros(4))), "4 slots for 5 op rows"),
                     (dict(values=t(torch.zeros(9, 2)), slot_of_row=slot.long()), "slot_of_row must be an int32 tensor"),
                     (dict(values=t(torch.zeros(9, 2)), slot_of_row=slot[:4]), "one entry per op row"),
                     (dict(values=t(torch.zeros(9, 2)), slot_of_row=[0] * 5), "slot_of_row must be an int32 tensor"),
                     (dict(values=t(torch.zeros(5, 2)), background=[0.0, 1.0, 2.0]), "one value per channel"),
                     (dict(values=t(torch.zeros(5, 2)), background=torch.zeros(2, dtype=torch.float64)), "float32 tensor on")):
        with pytest.raises(RuntimeError, match=word):
            _C.raster_values(cpu, **kw)
    assert not touched


# ---- the command -------------------------------------------------------------------------------------------------------
def _run(*argv):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    return subprocess.run([sys.executable, "-m", "hgs.paint_hierarchy", *argv], capture_output=True, text=True, env=env)


def test_parse_args_good_and_bad_lines():
    from hgs import paint_hierarchy as ph
    base = ["a.hier", "--cameras", "c.json", "--camera", "2", "--out", "i.npy"]
    lvl = base + ["--builtin", "level"]
    assert ph.parse_args(lvl) == dict(
        in_path="a.hier", cameras="c.json", camera=2, values=None, builtin="level", lod_error=None, tau_px=0.0,
        frustum=True, resolution_scale=1.0, normalize=False, background=None, out_path="i.npy")
    full = ph.parse_args(["--values", "v.npy", "--tau-px", "3", "a.hier", "--no-frustum", "--background", "0.5", "-1", "2",
                          "--cameras", "c.json", "--normalize", "--camera", "0", "--resolution-scale", "2", "--out", "o.npy"])
    assert (full["values"], full["builtin"], full["lod_error"], full["tau_px"], full["frustum"]) == ("v.npy", None, None, 3.0, False)
    assert (full["background"], full["normalize"], full["resolution_scale"], full["camera"], full["out_path"]) == \
        ((0.5, -1.0, 2.0), True, 2.0, 0, "o.npy")
    assert ph.parse_args(base + ["--lod-error", "e.npz"])["lod_error"] == "e.npz"
    assert ph.parse_args(lvl + ["--background", "1"])["background"] == (1.0,)
    for b in ph.BUILTINS:
        assert ph.parse_args(base + ["--builtin", b])["builtin"] == b
    bad = [[], base, lvl[1:], lvl + ["b.hier"], lvl + ["--bogus"], lvl + ["--values", "v.npy"],
           lvl + ["--lod-error", "e.npz"], base + ["--values", "v.npy", "--lod-error", "e.npz"], lvl + ["--builtin", "extent"],
           base + ["--builtin", "depth"], base + ["--builtin"], base[:5] + ["--builtin", "level"],
           base[:3] + base[5:] + ["--builtin", "level"], ["a.hier"] + base[3:] + ["--builtin", "level"],
           lvl + ["--camera", "1"], base[:3] + ["--camera", "-1", "--out", "i.npy", "--builtin", "level"],
           base[:3] + ["--camera", "x", "--out", "i.npy", "--builtin", "level"], lvl + ["--tau-px", "-1"],
           lvl + ["--tau-px", "nan"], lvl + ["--tau-px", "x"], lvl + ["--resolution-scale", "0"],
           lvl + ["--resolution-scale", "inf"], lvl + ["--normalize", "--normalize"], lvl + ["--no-frustum", "--no-frustum"],
           lvl + ["--background"], lvl + ["--background", "--normalize"], lvl + ["--background", "x"],
           lvl + ["--background", "nan"], lvl + ["--background", "1", "--background", "2"], lvl + ["--out", "j.npy"]]
    for argv in bad:
        assert ph.parse_args(argv) is None, argv


def test_command_exits_two_on_usage_and_one_on_bad_values_and_writes_nothing(tmp_path):
    import contribution_cases as cc
    from hgs import synth
    out = tmp_path / "image.npy"
    for argv in ([], ["a.hier"], ["a.hier", "--cameras", "c.json", "--camera", "0", "--out", str(out)],
                 ["a.hier", "--cameras", "c.json", "--camera", "0", "--out", str(out), "--builtin", "level", "--bogus"]):
        r = _run(*argv)
        assert r.returncode == 2 and r.stderr.strip().startswith("usage: python -m hgs.paint_hierarchy"), (argv, r.stderr)
    r = _run(str(tmp_path / "none.hier"), "--cameras", str(tmp_path / "c.json"), "--camera", "0", "--builtin", "level",
             "--out", str(out))
    assert r.returncode == 2 and "does not exist" in r.stderr
    # files that exist: the values are read before the hierarchy, so their faults need no GPU
    hier, cams, vals, err = tmp_path / "in.hier", tmp_path / "c.json", tmp_path / "v.npy", tmp_path / "e.npz"
    hier.write_bytes(b"")
    cams.write_text(json.dumps([cc.camera_entry(synth.orbit_camera(cc.W, cc.H, k, 2)) for k in range(2)]))
    line = [str(hier), "--cameras", str(cams), "--out", str(out)]
    r = _run(*line, "--camera", "2", "--builtin", "level")
    assert r.returncode == 2 and "holds 2 cameras" in r.stderr
    r = _run(*line, "--camera", "0", "--values", str(vals))
    assert r.returncode == 2 and "does not exist" in r.stderr
    for wrong in (np.zeros((4, 2, 2), dtype=np.float32), np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.float32)):
        np.save(vals, wrong)
        r = _run(*line, "--camera", "0", "--values", str(vals))
        assert r.returncode == 1 and "v.npy" in r.stderr and "[N] or [N, C]" in r.stderr and "nothing written" in r.stderr
    vals.write_bytes(b"not an array")
    r = _run(*line, "--camera", "0", "--values", str(vals))
    assert r.returncode == 1 and "v.npy" in r.stderr
    np.savez(err, err=np.zeros(4), entries=np.zeros(4))
    r = _run(*line, "--camera", "1", "--lod-error", str(err))
    assert r.returncode == 1 and "e.npz" in r.stderr and "no err and wsum" in r.stderr
    cams.write_text("[]")
    r = _run(*line, "--camera", "0", "--builtin", "level")
    assert r.returncode == 2 and "non-empty list" in r.stderr
    assert not out.exists()


# ---- kernel resources --------------------------------------------------------------------------------------------------
def test_new_kernel_has_no_scratch_and_the_walks_neighbours_keep_their_rows():
    """From the compiler's own report (scripts/kernel_resources.py, no GPU): every instance of the painting kernel spills
    nothing and keeps the three LDS arrays of its file, and the other includers of csrc/tile_walk.h show exactly the
    registers, LDS and scratch they showed before this file joined them (profiles/f26_values_kernels.md)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    csrc = os.path.join(PKG, "csrc")
    rows = {r["kernel"]: r for r in kernel_resources.collect(
        [os.path.join(csrc, f) for f in ("values.hip", "pixels.hip", "contrib.hip", "attribute.hip")])}
    mine = {k: r for k, r in rows.items() if r["file"] == "values.hip"}
    assert sorted(mine) == sorted(f"values_tile_kernel<{c}, {w}>" for c in (1, 2, 3, 4) for w in ("false", "true"))
    lds = (64 + 1) * (2 * 16 + 4 * 2 + 16)             # records, lists, values
    for k, r in mine.items():
        assert r["scratch"] == 0 and r["spills"] == 0 and r["wg"] == 64 and r["lds"] == lds, (k, r)
        assert r["vgpr"] + r["agpr"] <= 80, (k, r["vgpr"] + r["agpr"])        # K6's occupancy class or better
        c, w = int(k[len("values_tile_kernel<")]), k.endswith("true>")
        assert r["mix"]["global_store"] == 4 * (c + w), (k, r["mix"])         # plain stores of the lane's four pixels, no more
        assert r["mix"]["valu_dpp"] == 0, (k, r["mix"])                       # no cross-lane reduction
    before = {                                                      # kernel: (VGPRs, LDS bytes, scratch bytes)
        "pixels_tile_kernel": (82, 2600, 0),
        "contrib_tile_kernel": (46, 6760, 0), "contrib_sum_kernel": (34, 0, 0),
        "attribute_tile_kernel<1>": (49, 6760, 0), "attribute_tile_kernel<2>": (56, 6760, 0),
        "attribute_tile_kernel<3>": (64, 6760, 0), "attribute_sum_kernel<1>": (32, 0, 0),
        "attribute_sum_kernel<2>": (38, 0, 0), "attribute_sum_kernel<3>": (44, 0, 0)}
    for k, want in before.items():
        r = rows[k]
        assert (r["vgpr"] + r["agpr"], r["lds"], r["scratch"]) == want, (k, r["vgpr"] + r["agpr"], r["lds"], r["scratch"])
