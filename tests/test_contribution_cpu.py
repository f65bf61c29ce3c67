"""The contribution statistics without a GPU: the float64 spec (tests/contribution_spec.py) against the oracle's own
autograd and against the image's transmittance, the two exports, every refusal of hgs_raster_contrib, its size query, the
command's usage errors and the rule of low_contribution_mask."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import contribution_spec as cs
import parity as pa
from hgs import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hierarchical-3d-gaussians_amd")
NAMES = ("hgs_raster_contrib_tmp_bytes", "hgs_raster_contrib")
CASES = ((64, 16, 16, 3), (300, 70, 45, 0), (40, 5, 3, 1))


def _view(P, W, H, seed):
    cam, scene, _, _ = pa.default_case(P, W, H, seed)
    g = torch.Generator().manual_seed(seed + 11)
    return cs.oracle_view(scene, cam, colors_precomp=torch.rand(P, 3, generator=g, dtype=torch.float64))


@pytest.fixture(scope="module")
def views():
    return {c: _view(*c) for c in CASES}


@pytest.mark.parametrize("case", CASES)
def test_spec_sum_is_the_oracles_colour_gradient(views, case):
    """d(sum of the masked image channel 0) / d colors_precomp[:, 0] = wsum, all pixels and under a mask."""
    v = views[case]
    wmax, wsum, count = cs.fold(v)
    ref = cs.autograd_wsum(v)
    assert np.abs(wsum - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.all((count > 0) == (wmax > 0)) and np.all(wmax <= 0.99) and np.all(wsum >= wmax)
    mask = (np.arange(v.W * v.H) % 3 != 1)
    _, wsum_m, count_m = cs.fold(v, pixel_mask=mask)
    ref_m = cs.autograd_wsum(v, pixel_mask=mask)
    assert np.abs(wsum_m - ref_m).max() <= 1e-12 * max(1.0, np.abs(ref_m).max())
    assert np.all(count_m <= count) and count_m.sum() < count.sum()


@pytest.mark.parametrize("case", CASES)
def test_spec_weights_add_up_to_the_opacity_of_the_image(views, case):
    """sum_g wsum[g] == sum_p (1 - final_T[p])."""
    v = views[case]
    _, wsum, _ = cs.fold(v)
    assert abs(wsum.sum() - (1.0 - v.out.final_T).sum()) <= 1e-11 * v.W * v.H


def test_spec_slot_map_permutes_and_ignores(views):
    v = views[CASES[1]]
    P = v.P
    base = cs.fold(v)
    perm = np.random.default_rng(0).permutation(P + 9)[:P]
    got = cs.fold(v, slot_of_row=perm, n_slots=P + 9)
    for a, b in zip(base, got):
        assert np.array_equal(a, b[perm]) and b.sum() == a.sum()
    slot = np.where(np.arange(P) % 2 == 0, -1, P + 50)
    assert all(not a.any() for a in cs.fold(v, slot_of_row=slot, n_slots=P))
    twice = cs.fold(v, into=cs.fold(v))
    assert np.array_equal(twice[0], base[0]) and np.array_equal(twice[2], 2 * base[2])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_exports_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgs.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert re.search(rf"\b{name}\b", nm), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.lib().hgs_abi_version() == 14


def test_tmp_bytes_is_monotone_and_covers_the_records():
    lib = _lib.lib()
    grid = [0, 1, 2, 15, 16, 17, 63, 64, 65, 1000, 4097, 1 << 20, 2_667_604, (1 << 28) + 3]
    sizes = [lib.hgs_raster_contrib_tmp_bytes(L) for L in grid]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert all(s >= 16 * max(L, 1) for s, L in zip(sizes, grid))       # one 16-byte record per instance
    assert all(s <= 16 * max(L, 1) + 1024 for s, L in zip(sizes, grid))


FAKE = 0x10000       # never dereferenced: every refusal happens before any HIP call


def _args(P=10, W=32, H=32):
    a = _lib.RasterArgs()
    a.P, a.M, a.sh_degree, a.width, a.height = P, 0, 0, W, H
    a.tanfovx = a.tanfovy = a.scale_modifier = 1.0
    a.bg = a.viewmatrix = a.projmatrix = a.campos = FAKE
    a.means3D = a.opacities = a.colors_precomp = a.cov3D_precomp = FAKE
    return a


def _call(a, L=100, n_slots=10, wmax=FAKE, wsum=FAKE, count=FAKE, slot=None, geom=FAKE, binb=FAKE, img=FAKE, tmp=FAKE):
    lib = _lib.lib()
    rc = lib.hgs_raster_contrib(C.byref(a) if a is not None else None, geom, binb, img, L, None, slot, n_slots, wmax, wsum,
                                count, tmp, None, 0)
    return rc, lib.hgs_last_error().decode()


def test_every_refusal_is_invalid_with_its_message_and_needs_no_gpu():
    INVALID = 1
    for kw, word in ((dict(wmax=None), "null output"), (dict(wsum=None), "null output"), (dict(count=None), "null output"),
                     (dict(n_slots=0), "n_slots = 0"), (dict(n_slots=-3), "n_slots = -3"),
                     (dict(n_slots=9), "n_slots = 9 < P = 10"), (dict(geom=None), "null workspace"),
                     (dict(binb=None), "null workspace"), (dict(img=None), "null workspace"),
                     (dict(tmp=None), "null workspace")):
        rc, msg = _call(_args(), **kw)
        assert rc == INVALID and word in msg and "hgs_raster_contrib" in msg, (kw, rc, msg)
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
    # a slot map lifts the n_slots >= P requirement; nothing to do is OK and touches nothing, GPU or not
    assert _call(_args(P=0), n_slots=1)[0] == 0
    assert _call(_args(), L=0, n_slots=3, slot=FAKE)[0] == 0
    assert _call(_args(), L=0)[0] == 0


# ---- the command -------------------------------------------------------------------------------------------------------
def _run(*argv):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    return subprocess.run([sys.executable, "-m", "hgs.score_hierarchy", *argv], capture_output=True, text=True, env=env)


def test_parse_args_and_usage_errors(tmp_path):
    from hgs import score_hierarchy as sh
    ok = sh.parse_args(["a.hier", "s.npz", "--cameras", "c.json"])
    assert ok == dict(in_path="a.hier", out_path="s.npz", cameras="c.json", tau_px=0.0, frustum=True, resolution_scale=1.0,
                      mask_out=None, max_weight_below=None, sum_below=None, pixels_below=None, unseen="keep")
    full = sh.parse_args(["--tau-px", "3", "a.hier", "--no-frustum", "s.npz", "--cameras", "c.json", "--mask-out", "m.npy",
                          "--pixels-below", "4", "--max-weight-below", "0.01", "--unseen", "remove",
                          "--resolution-scale", "2"])
    assert (full["tau_px"], full["frustum"], full["mask_out"], full["pixels_below"], full["max_weight_below"],
            full["sum_below"], full["unseen"], full["resolution_scale"]) == (3.0, False, "m.npy", 4.0, 0.01, None, "remove", 2.0)
    base = ["a.hier", "s.npz", "--cameras", "c.json"]
    bad = [[], ["a.hier", "s.npz"], ["a.hier", "--cameras", "c.json"], base + ["extra"], base + ["--bogus"],
           base + ["--tau-px"], base + ["--tau-px", "x"], base + ["--tau-px", "-1"], base + ["--tau-px", "nan"],
           base + ["--tau-px", "1", "--tau-px", "2"], base + ["--resolution-scale", "0"], base + ["--mask-out", "m.npy"],
           base + ["--sum-below", "1"], base + ["--unseen", "remove"],
           base + ["--mask-out", "m.npy", "--sum-below", "1", "--unseen", "maybe"],
           base + ["--mask-out", "m.npy", "--sum-below", "x"]]
    for argv in bad:
        assert sh.parse_args(argv) is None, argv
    for argv in (bad[0], bad[1], bad[4]):
        r = _run(*argv)
        assert r.returncode == 2 and r.stderr.strip().startswith("usage: python -m hgs.score_hierarchy"), (argv, r.stderr)
    r = _run(str(tmp_path / "none.hier"), str(tmp_path / "s.npz"), "--cameras", str(tmp_path / "c.json"))
    assert r.returncode == 2 and "does not exist" in r.stderr and not (tmp_path / "s.npz").exists()


def test_camera_entries_follow_the_synthetic_cameras(tmp_path):
    """An entry written from a synth camera's own pose gives that camera's matrices back; bad entries are named."""
    from hgs import score_hierarchy as sh, synth
    cam = synth.orbit_camera(64, 48, 1, 3)
    c2w = cam.world_view_transform.t().double().inverse()
    entry = dict(width=64, height=48, position=c2w[:3, 3].tolist(), rotation=c2w[:3, :3].tolist(),
                 fx=0.5 * 64 / cam.tanfovx, fy=0.5 * 48 / cam.tanfovy)
    got = sh.camera_from_entry(entry, 0)
    assert (got.image_width, got.image_height) == (64, 48)
    assert abs(got.tanfovx - cam.tanfovx) < 1e-12 and abs(got.tanfovy - cam.tanfovy) < 1e-12
    assert torch.allclose(got.world_view_transform, cam.world_view_transform, atol=1e-6)
    assert torch.allclose(got.full_proj_transform, cam.full_proj_transform, atol=1e-5)
    half = sh.camera_from_entry(entry, 0, resolution_scale=2.0)
    assert (half.image_width, half.image_height) == (32, 24) and abs(half.tanfovx - cam.tanfovx) < 1e-12
    for broken in ({k: v for k, v in entry.items() if k != "fx"}, dict(entry, position=[0, 1]), dict(entry, width=0), 7):
        with pytest.raises(ValueError, match="camera 3"):
            sh.camera_from_entry(broken, 3)
    p = tmp_path / "c.json"
    p.write_text("[]")
    with pytest.raises(ValueError, match="non-empty list"):
        sh.read_cameras(str(p))


# ---- the mask ----------------------------------------------------------------------------------------------------------
def test_low_contribution_mask_against_its_numpy_statement():
    from hgs.importance import Scores, low_contribution_mask
    g = np.random.default_rng(4)
    N = 64
    nodes = np.zeros((N, 7), dtype=np.int32)
    nodes[:, 6] = np.where(np.arange(N) < 20, 2, 0)                      # 20 interior nodes, 44 leaves
    wmax = g.choice(np.array([0.0, 0.003, 1 / 255, 0.0039215689, 0.2, 0.99], dtype=np.float32), N)
    wsum = g.choice(np.array([0.0, 0.5, 1.0, 7.25]), N)
    count = g.integers(0, 6, N)
    entries = g.integers(0, 3, N)
    s = Scores(torch.from_numpy(wmax), torch.from_numpy(wsum), torch.from_numpy(count), torch.from_numpy(entries), 2)
    leaf, seen = nodes[:, 6] == 0, entries > 0
    for mw, sb, pb in ((1 / 255, None, None), (None, 1.0, None), (None, None, 3), (0.2, 1.0, None), (0.99, 7.25, 5),
                       (None, None, 2.5)):
        low = seen.copy()
        if mw is not None:
            low &= wmax < np.float32(mw)
        if sb is not None:
            low &= wsum < sb
        if pb is not None:
            low &= count < pb
        for unseen in ("keep", "remove"):
            ref = (leaf & (low | (~seen if unseen == "remove" else False))).astype(np.uint8)
            got = low_contribution_mask(torch.from_numpy(nodes), s, mw, sb, pb, unseen)
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), ref), (mw, sb, pb, unseen)
            assert not got.numpy()[~leaf].any()
    # strict: a value AT the bound stays
    at = low_contribution_mask(torch.from_numpy(nodes), s, max_weight_below=float(np.float32(0.2))).numpy()
    assert not at[wmax == np.float32(0.2)].any()
    with pytest.raises(ValueError, match="at least one"):
        low_contribution_mask(torch.from_numpy(nodes), s)
    with pytest.raises(ValueError, match="unseen"):
        low_contribution_mask(torch.from_numpy(nodes), s, sum_below=1.0, unseen="drop")
    with pytest.raises(ValueError, match="nodes must be"):
        low_contribution_mask(torch.from_numpy(nodes[:5]), s, sum_below=1.0)


def test_scores_zeros_and_merge():
    from hgs.importance import Scores
    a, b = Scores.zeros(4, "cpu"), Scores.zeros(4, "cpu")
    assert (a.wmax.dtype, a.wsum.dtype, a.count.dtype, a.entries.dtype, a.views) == \
        (torch.float32, torch.float64, torch.int64, torch.int64, 0)
    a.wmax[1], a.wsum[1], a.count[1], a.entries[1], a.views = 0.5, 2.0, 3, 1, 1
    b.wmax[1], b.wsum[1], b.count[1], b.entries[1], b.views = 0.25, 1.0, 1, 1, 2
    b.wmax[2], b.wsum[2], b.count[2], b.entries[2] = 0.75, 0.75, 1, 2
    m = a.merge(b)
    assert m.wmax.tolist() == [0, 0.5, 0.75, 0] and m.wsum.tolist() == [0, 3.0, 0.75, 0]
    assert m.count.tolist() == [0, 4, 1, 0] and m.entries.tolist() == [0, 2, 2, 0] and m.views == 3
    with pytest.raises(ValueError):
        a.merge(Scores.zeros(5, "cpu"))
