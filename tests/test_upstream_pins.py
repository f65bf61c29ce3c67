"""Consumes the goldens of the PIN KIT (tests/golden/make_upstream_golden.py -- run where the upstream CUDA extensions
exist): outputs of the UPSTREAM ``diff_gaussian_rasterization`` / ``gaussian_hierarchy._C`` for this repository's seeded
cases.  With a golden present, the oracle (CPU tests) and the HIP path (``-m gpu`` tests) are compared against what the
reference's own extension computed; the three semantics that were restated from memory -- how the kernel uses
``interpolation_weights`` / ``num_node_kids`` (gaussian_renderer/__init__.py:262-263), the cut rule and weight formula
(train_post.py:91-113) and the ``.hier`` byte layout (scene/gaussian_model.py:329,420-427) -- are then PINNED.

No golden is committed yet (the build environment has no CUDA stack): the CPU pin tests SKIP and say so, and parity
stays "unpinned" (DESIGN.md section 5).  The ``-m gpu`` tests then hold the HIP path to the kit's cases as the oracle
computes them (the generator driven through the oracle-backed stand-ins), so that the HIP side of the kit runs.  ``test_pin_kit_plumbing`` runs always: it drives the generator's own case
functions with the oracle-backed stand-ins in place of the upstream modules and feeds the resulting files to the same
checks -- that proves the kit's keys, shapes and call signatures fit together, NOT any value."""
import io
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

from hgs import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.environ.get("HGS_UPSTREAM_GOLDEN_DIR", os.path.join(HERE, "golden"))
REL_TOL = 1e-5


def _golden(name, directory=None):
    path = os.path.join(directory or GOLDEN_DIR, f"upstream_{name}.npz")
    if not os.path.exists(path):
        pytest.skip(f"parity unpinned: {os.path.relpath(path, os.path.dirname(HERE))} absent -- generate it with "
                    "tests/golden/make_upstream_golden.py on a machine with the upstream CUDA extensions")
    return np.load(path, allow_pickle=False)


KIT_CASES = {"raster_config1": "case_config1", "lod_cut": "case_lod_cut", "raster_post": "case_raster_post",
             "raster_needles": "case_needles", "hier_file": "case_hier_file"}


def _kit_case(name):
    """The pin kit's case ``name`` computed by the generator itself with the oracle-backed stand-ins (tests/harness) in
    place of the upstream modules, on the CPU: the oracle's values in the golden's format."""
    import importlib.util
    sys.path.insert(0, HERE)
    from harness import cpu_backends
    import diff_gaussian_rasterization as dgr
    import gaussian_hierarchy._C as gh
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(dgr, "_C", cpu_backends.OracleRasterC)
        mp.setattr(gh, "expand_to_size", cpu_backends.expand_to_size)
        mp.setattr(gh, "get_interpolation_weights", cpu_backends.get_interpolation_weights)
        spec = importlib.util.spec_from_file_location("_pin_kit", os.path.join(HERE, "golden", "make_upstream_golden.py"))
        kit = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(kit)
        mp.setattr(kit, "DEV", "cpu")
        return getattr(kit, KIT_CASES[name])()


def _golden_for_hip(name):
    """(golden, pinned): the upstream golden when it is committed; until then the kit's case as the oracle computes it,
    so that the HIP side of the kit runs and holds the HIP path to the oracle on the kit's cases (parity unpinned)."""
    if os.path.exists(os.path.join(GOLDEN_DIR, f"upstream_{name}.npz")):
        return _golden(name), True
    buf = io.BytesIO()
    np.savez(buf, **_kit_case(name))
    buf.seek(0)
    return np.load(buf, allow_pickle=False), False


def _scene_cam(G):
    scene = synth.Scene(*(torch.from_numpy(np.ascontiguousarray(G["in_" + k])) for k in
                          ("means3D", "scales", "rotations", "opacities", "shs")), int(G["in_sh_degree"]))
    W, H = int(G["cam_W"]), int(G["cam_H"])
    base = synth.make_camera(W, H)
    cam = synth.Camera(W, H, 2 * np.arctan(float(G["cam_tanfovx"])), 2 * np.arctan(float(G["cam_tanfovy"])),
                       torch.from_numpy(G["cam_viewmatrix"]), torch.from_numpy(G["cam_projmatrix"]),
                       torch.from_numpy(G["cam_campos"]), base.znear, base.zfar)
    return scene, cam


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    s = np.abs(b).max()
    return float(np.abs(a - b).max() / s) if s > 0 else float(np.abs(a).max())


def _compare_raster(got_color, got_radii, got_invd, got_grads, G, what):
    assert np.array_equal(np.asarray(got_radii), G["out_radii"]), f"{what}: radii differ from upstream"
    errs = {"color": _rel(got_color, G["out_color"])}
    if bool(G["do_depth"]) and "out_invdepth" in G.files:
        errs["invdepth"] = _rel(got_invd, G["out_invdepth"])
    for k in ("means3D", "means2D", "shs", "opacities", "scales", "rotations"):
        errs["d_" + k] = _rel(got_grads[k], G["out_d_" + k])
    bad = {k: v for k, v in errs.items() if not v <= REL_TOL}
    assert not bad, f"{what} vs upstream golden: {bad} (all: {errs})"


def check_raster_oracle(G, what):
    import parity as pa
    scene, cam = _scene_cam(G)
    kw = {}
    if "interpolation_weights" in G.files:
        kw = dict(interpolation_weights=torch.from_numpy(G["interpolation_weights"]),
                  num_node_kids=torch.from_numpy(G["num_node_kids"]))
    args = (scene, cam, torch.from_numpy(G["bg"]), torch.from_numpy(G["gc"]), torch.from_numpy(G["gd"]))
    if kw:
        # the two readings of interpolation_weights / num_node_kids (oracle/raster_oracle.py: lod_opacity per Gaussian --
        # what the kernels implement -- vs lod_alpha per pixel): say which one upstream's pixels follow before asserting
        fit = {m: _rel(pa.run_oracle(*args, do_depth=bool(G["do_depth"]), mask_fragile=False, lod_mode=m, **kw)[0]
                       .color.detach().numpy(), G["out_color"]) for m in ("opacity", "alpha")}
        print(f"{what}: colour error vs upstream by LOD remap reading: {fit}")
        assert fit["opacity"] <= REL_TOL or fit["alpha"] > REL_TOL, \
            f"upstream follows the per-PIXEL alpha remap ({fit}): move lod_opacity() from K1 into the compositing kernels"
    oo, og = pa.run_oracle(*args, do_depth=bool(G["do_depth"]), mask_fragile=False, **kw)   # the golden's loss covers every pixel
    _compare_raster(oo.color.detach().numpy(), oo.radii.numpy(), oo.invdepth.detach().numpy(),
                    {k: v.numpy() for k, v in og.items()}, G, f"oracle, {what}")


def check_raster_hip(G, what, gpu):
    import parity as pa
    scene, cam = _scene_cam(G)
    kw = {}
    if "interpolation_weights" in G.files:
        kw = dict(interpolation_weights=torch.from_numpy(G["interpolation_weights"]),
                  num_node_kids=torch.from_numpy(G["num_node_kids"]))
    hip = pa.run_hip(scene, cam, torch.from_numpy(G["bg"]), torch.from_numpy(G["gc"]), torch.from_numpy(G["gd"]), gpu,
                     do_depth=bool(G["do_depth"]), grad_mask=None, **kw)
    _compare_raster(hip["color"].numpy(), hip["radii"].numpy(), hip["invdepth"].numpy(),
                    {k: v.numpy() for k, v in hip["grads"].items()}, G, f"HIP, {what}")


def check_needles(G, what, hip_color=None, verdict=True):
    """Which rule for an exponent that ROUNDING made positive does upstream follow -- "power > 0 -> skip" (SURVEY App.
    A.8, the public lineage) or the clamp at 0 of this library's kernels?  In float64 the exponent
    of a positive definite conic is never positive and the two coincide; a float32 conic loses positive definiteness only
    on extreme needles (3 000 px x 0.5 px: a c - b^2 cancels to its last bits; measured: none up to 2 500 px), and then
    on whole stripes of the image.  The oracle is run ALL in float32 under both rules (its operation order is not
    upstream's, so single pixels need not coincide -- how many pixels are far off under each rule is what tells) and, when
    given, the HIP image is held to the golden outside the pixels where the two float32 evaluations disagree.  ``verdict``:
    fail when upstream follows the other rule (meaningless for a golden that is not upstream's)."""
    import parity as pa
    scene, cam = _scene_cam(G)
    args = (scene, cam, torch.from_numpy(G["bg"]), torch.from_numpy(G["gc"]), torch.from_numpy(G["gd"]))
    img = {}
    for rule in ("skip", "clamp"):
        oo, _ = pa.run_oracle(*args, do_depth=True, mask_fragile=False, dtype=torch.float32, positive_power=rule)
        img[rule] = oo.color.detach().double().numpy()
    gold = np.asarray(G["out_color"], np.float64)
    differ = np.abs(img["skip"] - img["clamp"]).max(axis=0) > 1e-6
    fit = {r: float(np.abs(img[r] - gold).max() / max(np.abs(gold).max(), 1e-12)) for r in img}
    n_sk = int((np.abs(img["skip"] - gold).max(axis=0) > 1e-2).sum())
    n_cl = int((np.abs(img["clamp"] - gold).max(axis=0) > 1e-2).sum())
    print(f"{what}: float32 oracle vs upstream -- max error under 'skip' {fit['skip']:.2e} ({n_sk} pixels off by > 1e-2), under "
          f"'clamp' {fit['clamp']:.2e} ({n_cl} pixels); the two rules differ on {int(differ.sum())} of {differ.size} pixels")
    follows = "skip" if n_sk < n_cl else ("clamp" if n_cl < n_sk else "either (the case did not separate them)")
    print(f"{what}: upstream follows: {follows}")
    if hip_color is not None:
        off = np.abs(np.asarray(hip_color, np.float64) - gold).max(axis=0) > 1e-4
        assert not (off & ~differ).any(), f"{what}: {int((off & ~differ).sum())} HIP pixels differ from upstream where the rules agree"
        if verdict and follows == "skip" and (off & differ).any():
            pytest.fail(f"{what}: upstream SKIPS a Gaussian whose float32 exponent is positive; the kernels clamp it: "
                        f"{int((off & differ).sum())} pixels differ -- replace the clamp in render.hip (fwd_pair_live / "
                        "bwd_pair_live) by the skip")
    return follows, int(differ.sum())


def _lod_compare(i, r, p, n, w, k, G, what):
    assert len(r) == int(G[f"n_{i}"]), f"{what}: cut size {len(r)} != upstream {int(G[f'n_{i}'])} at threshold {i}"
    assert np.array_equal(r, G[f"render_indices_{i}"]), f"{what}: render_indices differ (threshold {i})"
    assert np.array_equal(n, G[f"nodes_for_render_indices_{i}"]), f"{what}: nodes_for_render_indices differ"
    up_p = G[f"parent_indices_{i}"]
    # documented deviation: upstream stores -1 for the root's parent, this library the root's own
    # Gaussian (its weight is 1, and -1 would index out of bounds in the in-op gather)
    same = (p == up_p) | (up_p < 0)
    assert same.all(), f"{what}: parent_indices differ (threshold {i})"
    assert np.array_equal(k, G[f"num_siblings_{i}"]), f"{what}: num_siblings differ"
    assert np.abs(w.astype(np.float64) - G[f"weights_{i}"]).max() <= 2e-6, f"{what}: interpolation weights differ"


def check_lod_oracle(G):
    from oracle import lod_oracle as lo
    for i, tau in enumerate(G["taus"]):
        r, p, n = lo.expand_to_size(G["nodes"], G["boxes"], float(tau), G["viewpoint"])
        w, k = lo.get_interpolation_weights(n, float(tau), G["nodes"], G["boxes"], G["viewpoint"])
        _lod_compare(i, r, p, n, w, k, G, "LOD oracle")


def check_lod_hip(G, gpu):
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    nodes, boxes = torch.from_numpy(G["nodes"]).to(gpu), torch.from_numpy(G["boxes"]).to(gpu)
    N = nodes.shape[0]
    vp = torch.from_numpy(G["viewpoint"])
    for i, tau in enumerate(G["taus"]):
        ri = torch.zeros(N, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
        w = torch.zeros(N, device=gpu); ns = torch.zeros(N, dtype=torch.int32, device=gpu)
        n = expand_to_size(nodes, boxes, float(tau), vp.to(gpu), torch.zeros(3), ri, pi, ni)
        get_interpolation_weights(ni[:n], float(tau), nodes, boxes, vp, torch.zeros(3), w, ns)
        _lod_compare(i, ri[:n].cpu().numpy(), pi[:n].cpu().numpy(), ni[:n].cpu().numpy(), w[:n].cpu().numpy(),
                     ns[:n].cpu().numpy(), G, "HIP LOD cut")


def check_hier_file(G):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    names = ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes")
    with tempfile.TemporaryDirectory() as d:
        up = os.path.join(d, "upstream.hier")
        G["file_bytes"].tofile(up)
        back = load_hierarchy(up)                            # an upstream-written file must load ...
        for k, v in zip(names, back):
            want = G["loaded_" + k]
            assert tuple(v.shape) == tuple(want.shape), (k, tuple(v.shape), tuple(want.shape))
            assert np.array_equal(v.numpy(), want), f"load_hierarchy: {k} differs from what upstream load_hierarchy returns"
        ours = os.path.join(d, "ours.hier")
        write_hierarchy(ours, *(torch.from_numpy(G["in_" + k]) for k in names))
        mine = np.fromfile(ours, dtype=np.uint8)             # ... and the same data must be written to the same bytes
        assert mine.shape == G["file_bytes"].shape and np.array_equal(mine, G["file_bytes"]), \
            "write_hierarchy does not produce the upstream file byte for byte"


# ---- CPU: the ORACLE against upstream ----------------------------------------------------------------------------------
def test_oracle_matches_upstream_rasterizer_config1():
    check_raster_oracle(_golden("raster_config1"), "config 1")


def test_oracle_matches_upstream_rasterizer_with_lod_tensors():
    check_raster_oracle(_golden("raster_post"), "render_post-shaped call (pins lod_opacity)")


def test_oracle_needles_skip_or_clamp():
    check_needles(_golden("raster_needles"), "needles")


def test_lod_oracle_matches_upstream_cut_and_weights():
    check_lod_oracle(_golden("lod_cut"))


def test_hier_io_matches_upstream_file():
    check_hier_file(_golden("hier_file"))


# ---- GPU: the HIP path against upstream -------------------------------------------------------------------------------
# (without an upstream golden the kit's case as the oracle computes it stands in: see _golden_for_hip)
def _source(pinned):
    return "" if pinned else " [oracle kit case, parity unpinned]"


@pytest.mark.gpu
def test_hip_matches_upstream_rasterizer_config1(gpu):
    G, pinned = _golden_for_hip("raster_config1")
    check_raster_hip(G, "config 1" + _source(pinned), gpu)


@pytest.mark.gpu
def test_hip_matches_upstream_rasterizer_with_lod_tensors(gpu):
    G, pinned = _golden_for_hip("raster_post")
    check_raster_hip(G, "render_post-shaped call (pins lod_opacity)" + _source(pinned), gpu)


@pytest.mark.gpu
def test_hip_needles_against_upstream(gpu):
    import parity as pa
    G, pinned = _golden_for_hip("raster_needles")
    scene, cam = _scene_cam(G)
    hip = pa.run_hip(scene, cam, torch.from_numpy(G["bg"]), torch.from_numpy(G["gc"]), torch.from_numpy(G["gd"]), gpu,
                     do_depth=True, grad_mask=None)
    check_needles(G, "needles (HIP)" + _source(pinned), hip["color"].numpy(), verdict=pinned)


@pytest.mark.gpu
def test_hip_matches_upstream_cut_and_weights(gpu):
    G, pinned = _golden_for_hip("lod_cut")
    check_lod_hip(G, gpu)


# ---- the kit itself -----------------------------------------------------------------------------------------------------
def test_pin_kit_plumbing(tmp_path):
    """Generator case functions -> .npz -> the checks above, with the oracle-backed stand-ins (tests/harness) playing the
    upstream modules on the CPU.  Values are the oracle's own, so this pins NOTHING; it proves that the generator's
    keys / shapes / call signatures and the consumer fit, so that the first real golden does not die on a typo."""
    for name in KIT_CASES:
        np.savez_compressed(os.path.join(tmp_path, f"upstream_{name}.npz"), **_kit_case(name))
    d = str(tmp_path)
    check_raster_oracle(_golden("raster_config1", d), "config 1 (plumbing)")
    G = _golden("raster_post", d)
    assert int(G["n"]) > 100 and float(((G["interpolation_weights"][:int(G["n"])] > 0) &
                                        (G["interpolation_weights"][:int(G["n"])] < 1)).mean()) > 0.02, \
        "the render_post case must contain nodes in transition, or it would not exercise the LOD opacity"
    check_raster_oracle(G, "render_post shape (plumbing)")
    check_lod_oracle(_golden("lod_cut", d))
    check_hier_file(_golden("hier_file", d))
    # the needle case must SEPARATE the two rules for a positive exponent (here the stand-in's values are the float64
    # oracle's: both float32 evaluations are compared with those, the verdict itself means nothing)
    follows, n_differ = check_needles(_golden("raster_needles", d), "needles (plumbing)")
    assert n_differ > 0, "the needle case does not produce a single float32 exponent above zero: it would pin nothing"
