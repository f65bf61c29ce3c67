"""The image attribution without a GPU: the float64 spec (tests/attribution_spec.py) against the oracle's own autograd,
the two exports, every refusal of hgs_raster_attribute, its size query, the Python glue's refusals, Attribution's merge
and mean, and the command's parser and exits."""
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

import attribution_spec as asp
import contribution_spec as cs
import parity as pa
from hgs import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hierarchical-3d-gaussians_amd")
NAMES = ("hgs_raster_attribute_tmp_bytes", "hgs_raster_attribute")
CASES = ((64, 16, 16, 3), (300, 70, 45, 0))


def _image(C_, H, W, seed):
    return np.random.default_rng(seed).standard_normal((C_, H, W)).astype(np.float32)


@pytest.fixture(scope="module")
def views():
    out = {}
    for P, W, H, seed in CASES:
        cam, scene, _, _ = pa.default_case(P, W, H, seed)
        g = torch.Generator().manual_seed(seed + 11)
        out[(P, W, H, seed)] = asp.oracle_view(scene, cam, colors_precomp=torch.rand(P, 3, generator=g, dtype=torch.float64))
    return out


@pytest.mark.parametrize("case", CASES)
def test_spec_is_the_oracles_colour_gradient_seeded_with_the_image(views, case):
    """d(sum_c sum_p f_c(p) color_c(p)) / d colors_precomp = A, all pixels and under a mask; Aabs bounds it and a
    channel of ones is wsum, which is contribution_spec's."""
    v = views[case]
    f = _image(3, v.H, v.W, case[3] + 5)
    for mask in (None, np.arange(v.W * v.H) % 3 != 1):
        A, Aabs, wsum = asp.fold_image(v, f, pixel_mask=mask)
        ref = asp.autograd_attribution(v, f, pixel_mask=mask)
        assert A.shape == ref.shape == (v.P, 3)
        assert np.abs(A - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        assert np.all(np.abs(A) <= Aabs * (1 + 1e-12)) and Aabs.max() > 0
        ones, ones_abs, _ = asp.fold_image(v, np.ones((1, v.H, v.W)), pixel_mask=mask)
        assert np.array_equal(ones, ones_abs) and np.abs(ones[:, 0] - wsum).max() <= 1e-13 * wsum.max()
        assert np.abs(wsum - cs.fold(v, pixel_mask=mask)[1]).max() <= 1e-12 * wsum.max()


def test_spec_selects_the_image_and_follows_the_slot_map(views):
    v = views[CASES[1]]
    f = _image(2, v.H, v.W, 3)
    mask = np.arange(v.W * v.H) % 5 != 2
    base = asp.fold_image(v, f, pixel_mask=mask)
    poisoned = f.reshape(2, -1).copy()
    poisoned[0, ~mask], poisoned[1, ~mask] = np.nan, np.inf
    for a, b in zip(base, asp.fold_image(v, poisoned.reshape(f.shape), pixel_mask=mask)):
        assert np.array_equal(a, b)
    P = v.P
    perm = np.random.default_rng(0).permutation(P + 9)[:P]
    got = asp.fold_image(v, f, pixel_mask=mask, slot_of_row=perm, n_slots=P + 9)
    for a, b in zip(base, got):
        rest = np.ones(P + 9, dtype=bool)
        rest[perm] = False
        assert np.array_equal(a, b[perm]) and not b[rest].any()
    slot = np.where(np.arange(P) % 2 == 0, -1, P + 50)
    assert all(not a.any() for a in asp.fold_image(v, f, slot_of_row=slot, n_slots=P))
    one = asp.fold_image(v, f[0], pixel_mask=mask)               # [H, W]: one channel
    assert one[0].shape == (P, 1) and np.abs(one[0][:, 0] - base[0][:, 0]).max() <= 1e-13 * np.abs(base[0]).max()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_exports_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgs.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert re.search(rf"\b{name}\b", nm), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.lib().hgs_abi_version() == 14


def test_tmp_bytes_is_monotone_covers_the_records_and_has_the_contribution_scratchs_size():
    lib = _lib.lib()
    grid = [0, 1, 2, 15, 16, 17, 63, 64, 65, 1000, 4097, 1 << 20, 2_667_604, (1 << 28) + 3]
    sizes = [lib.hgs_raster_attribute_tmp_bytes(L) for L in grid]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert all(s >= 16 * max(L, 1) for s, L in zip(sizes, grid))       # one 16-byte record per instance
    assert all(s <= 16 * max(L, 1) + 1024 for s, L in zip(sizes, grid))
    assert sizes == [lib.hgs_raster_contrib_tmp_bytes(L) for L in grid]


FAKE = 0x10000       # never dereferenced: every refusal happens before any HIP call


def _args(P=10, W=32, H=32):
    a = _lib.RasterArgs()
    a.P, a.M, a.sh_degree, a.width, a.height = P, 0, 0, W, H
    a.tanfovx = a.tanfovy = a.scale_modifier = 1.0
    a.bg = a.viewmatrix = a.projmatrix = a.campos = FAKE
    a.means3D = a.opacities = a.colors_precomp = a.cov3D_precomp = FAKE
    return a


def _call(a, L=100, image=FAKE, channels=1, n_slots=10, out=FAKE, wsum=FAKE, slot=None, geom=FAKE, binb=FAKE, img=FAKE,
          tmp=FAKE):
    lib = _lib.lib()
    rc = lib.hgs_raster_attribute(C.byref(a) if a is not None else None, geom, binb, img, L, image, channels, None, slot,
                                  n_slots, out, wsum, tmp, None, 0)
    return rc, lib.hgs_last_error().decode()


def test_every_refusal_is_invalid_with_its_message_and_needs_no_gpu():
    INVALID = 1
    for kw, word in ((dict(out=None), "null output"), (dict(image=None), "null image"),
                     (dict(channels=0), "channels = 0"), (dict(channels=4), "channels = 4"),
                     (dict(channels=-1), "channels = -1"),
                     (dict(n_slots=0), "n_slots = 0"), (dict(n_slots=-3), "n_slots = -3"),
                     (dict(n_slots=9), "n_slots = 9 < P = 10"), (dict(geom=None), "null workspace"),
                     (dict(binb=None), "null workspace"), (dict(img=None), "null workspace"),
                     (dict(tmp=None), "null workspace")):
        rc, msg = _call(_args(), **kw)
        assert rc == INVALID and word in msg and "hgs_raster_attribute" in msg, (kw, rc, msg)
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
    # wsum is optional; a slot map lifts the n_slots >= P requirement; half rows are allowed; nothing to do is OK and
    # touches nothing, GPU or not
    assert _call(_args(P=0), n_slots=1)[0] == 0
    assert _call(_args(), L=0, n_slots=3, slot=FAKE, wsum=None, channels=3)[0] == 0
    a = _args()
    a.lod_half_rows, a.lod_render_indices, a.colors_precomp, a.cov3D_precomp = 1, FAKE, None, None
    a.shs = a.scales = a.rotations = a.lod_parent_indices = a.interpolation_weights = a.num_node_kids = FAKE
    a.M, a.sh_degree, a.lod_n, a.lod_rows = 16, 3, 10, 50
    rc, msg = _call(a, L=0)
    assert rc == 0, msg


# ---- the Python glue ---------------------------------------------------------------------------------------------------
def test_raster_attribute_refuses_bad_tensors_before_the_library():
    """The image's device is the first thing checked, so a host image, an array and None are refused with no GPU at
    hand; the refusals behind it need device tensors and are in tests/test_attribution_gpu.py."""
    from diff_gaussian_rasterization import _C
    call = types.SimpleNamespace(device=torch.device("cuda:0"), P=5, W=8, H=4, L=10, L_ws=10)
    img, out = torch.zeros(1, 4, 8), torch.zeros(5, 1, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="image must be a tensor on the forward's device"):
        _C.raster_attribute(call, img, out)
    with pytest.raises(RuntimeError, match="image must be a tensor on the forward's device"):
        _C.raster_attribute(call, np.zeros((1, 4, 8), dtype=np.float32), out)
    with pytest.raises(RuntimeError, match="image must be a tensor on the forward's device"):
        _C.raster_attribute(call, None, out)


def test_attribution_zeros_merge_and_mean():
    from hgs.importance import Attribution
    a, b = Attribution.zeros(4, "cpu", channels=2), Attribution.zeros(4, "cpu", channels=2)
    assert (a.acc.dtype, a.wsum.dtype, a.entries.dtype, a.views) == (torch.float64, torch.float64, torch.int64, 0)
    assert a.acc.shape == (4, 2) and Attribution.zeros(3, "cpu").acc.shape == (3, 1)
    a.acc[1], a.wsum[1], a.entries[1], a.views = torch.tensor([1.0, -2.0]), 2.0, 1, 1
    b.acc[1], b.wsum[1], b.entries[1], b.views = torch.tensor([0.5, 0.5]), 2.0, 1, 2
    b.acc[2], b.wsum[2], b.entries[2] = torch.tensor([3.0, 0.0]), 0.75, 2
    b.acc[3] = torch.tensor([7.0, 7.0])                          # (no weight: its mean is 0, not inf)
    m = a.merge(b)
    assert m.acc.tolist() == [[0, 0], [1.5, -1.5], [3.0, 0.0], [7.0, 7.0]] and m.wsum.tolist() == [0, 4.0, 0.75, 0]
    assert m.entries.tolist() == [0, 2, 2, 0] and m.views == 3
    assert m.mean().tolist() == [[0, 0], [0.375, -0.375], [4.0, 0.0], [0, 0]]
    assert a.acc[1].tolist() == [1.0, -2.0]                      # a new object
    n = m.numpy()
    assert set(n) == {"acc", "wsum", "entries", "views"} and n["acc"].dtype == np.float64 and int(n["views"]) == 3
    with pytest.raises(ValueError):
        a.merge(Attribution.zeros(5, "cpu", channels=2))
    with pytest.raises(ValueError):
        a.merge(Attribution.zeros(4, "cpu", channels=3))
    for bad in (0, 4):
        with pytest.raises(ValueError, match="channels"):
            Attribution.zeros(4, "cpu", channels=bad)


# ---- the command -------------------------------------------------------------------------------------------------------
def _run(*argv):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    return subprocess.run([sys.executable, "-m", "hgs.lod_error", *argv], capture_output=True, text=True, env=env)


def test_parse_args_good_and_bad_lines():
    from hgs import lod_error as le
    base = ["a.hier", "e.npz", "--cameras", "c.json", "--tau-px", "3"]
    assert le.parse_args(base) == dict(in_path="a.hier", out_path="e.npz", cameras="c.json", tau_px=3.0, ref_tau_px=0.0,
                                       targets=None, frustum=True, resolution_scale=1.0)
    full = le.parse_args(["--tau-px", "6", "a.hier", "--no-frustum", "e.npz", "--cameras", "c.json", "--ref-tau-px", "1.5",
                          "--resolution-scale", "2"])
    assert (full["tau_px"], full["ref_tau_px"], full["frustum"], full["resolution_scale"], full["targets"]) == \
        (6.0, 1.5, False, 2.0, None)
    t = le.parse_args(base + ["--targets", "gt"])
    assert t["targets"] == "gt" and t["ref_tau_px"] is None
    assert le.parse_args(base[:4] + ["--tau-px", "0"])["tau_px"] == 0.0
    bad = [[], ["a.hier", "e.npz"], base[:4], ["a.hier"] + base[2:], base + ["extra"], base + ["--bogus"],
           base[:4] + ["--tau-px"], base[:4] + ["--tau-px", "x"], base[:4] + ["--tau-px", "-1"],
           base[:4] + ["--tau-px", "nan"], base + ["--tau-px", "2"], base + ["--ref-tau-px", "-0.5"],
           base + ["--ref-tau-px", "nan"], base + ["--ref-tau-px", "1", "--targets", "gt"],
           base + ["--targets", "gt", "--targets", "gt2"], base + ["--resolution-scale", "0"],
           base + ["--resolution-scale", "inf"], base + ["--cameras", "d.json"]]
    for argv in bad:
        assert le.parse_args(argv) is None, argv


def test_command_exits_two_on_usage_and_one_on_bad_targets_and_writes_nothing(tmp_path):
    import contribution_cases as cc
    from hgs import synth
    out = tmp_path / "e.npz"
    for argv in ([], ["a.hier", str(out)], ["a.hier", str(out), "--cameras", "c.json"],
                 ["a.hier", str(out), "--cameras", "c.json", "--tau-px", "3", "--bogus"]):
        r = _run(*argv)
        assert r.returncode == 2 and r.stderr.strip().startswith("usage: python -m hgs.lod_error"), (argv, r.stderr)
    r = _run(str(tmp_path / "none.hier"), str(out), "--cameras", str(tmp_path / "c.json"), "--tau-px", "3")
    assert r.returncode == 2 and "does not exist" in r.stderr
    # files that exist: the targets are read before the hierarchy, so their faults need no GPU
    hier, cams, gt = tmp_path / "in.hier", tmp_path / "c.json", tmp_path / "gt"
    hier.write_bytes(b"")
    cams.write_text(json.dumps([cc.camera_entry(synth.orbit_camera(cc.W, cc.H, k, 2)) for k in range(2)]))
    line = [str(hier), str(out), "--cameras", str(cams), "--tau-px", "3", "--targets", str(gt)]
    r = _run(*line)
    assert r.returncode == 2 and "does not exist" in r.stderr                       # the directory itself
    gt.mkdir()
    np.save(gt / "0.npy", np.zeros((3, cc.H, cc.W), dtype=np.float32))
    r = _run(*line)
    assert r.returncode == 1 and "1.npy" in r.stderr and "nothing written" in r.stderr, r.stderr
    for wrong in (np.zeros((3, cc.H, cc.W + 1), dtype=np.float32), np.zeros((3, cc.H, cc.W)), np.zeros((cc.H, cc.W), dtype=np.float32)):
        np.save(gt / "1.npy", wrong)
        r = _run(*line)
        assert r.returncode == 1 and "1.npy" in r.stderr and f"[3, {cc.H}, {cc.W}]" in r.stderr, r.stderr
    (gt / "1.npy").write_bytes(b"not an array")
    r = _run(*line)
    assert r.returncode == 1 and "1.npy" in r.stderr
    cams.write_text("[]")
    r = _run(*line)
    assert r.returncode == 2 and "non-empty list" in r.stderr
    assert not out.exists()
