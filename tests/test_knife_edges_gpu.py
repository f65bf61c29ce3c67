"""HIP on purpose-built knife edges (tests/knife_edges.py): hundreds of pixels whose alpha >= 1/255 or T (1 - alpha) < 1e-4
decision lies inside the oracle's band.  Every one must reproduce an admissible outcome, and the kernels' gradients must
be the float64 gradients of the outcomes they took -- which fails if K7 decides alpha >= 1/255 differently from K6, if
K6's cell lists drop a cell whose alpha is just above 1/255, or if a route's alpha differs from the oracle's by more than
the band."""
import pytest
import torch

import knife_edges as ke
import parity as pa
from hgs import synth

pytestmark = pytest.mark.gpu

# (name, scene variant, do_depth).  Pixels are matched and compared under the default element-wise bound; the
# GRADIENTS are held to 4 x it, the rule of tests/test_scale_parity_gpu.py (3 x what the oracle in the kernels' precision
# split reaches on the same scene): the scenes' needles (0.5 px wide) make d_scales / d_rotations float32 sums with heavy
# cancellation -- that oracle is at 1.04 / 1.29 x the bound on them, the kernels measured 1.0 .. 3.2 x; norm-wise every
# tensor stays within 1e-5.  A kernel that blends a different set of entries than the outcome it reports is off by far
# more (tests/test_knife_edges_cpu.py::test_gradients_of_another_outcome_are_rejected).
GRAD_MIXED_TOL = 4.0
ROUTES = [
    ("sh", dict(), True),
    ("sh_no_depth", dict(), False),
    ("lod_opacity", dict(lod="opacity"), False),
    ("lod_alpha", dict(lod="alpha"), True),
    ("precomp_colours", dict(precomp=True), True),
]


@pytest.mark.parametrize("name,build_kw,do_depth", ROUTES, ids=[r[0] for r in ROUTES])
def test_knife_edge_pixels_take_an_admissible_outcome(gpu, name, build_kw, do_depth, monkeypatch):
    import diff_gaussian_rasterization as dgr
    s = ke.build(seed=1, **build_kw)
    if s["lod_mode"] == "alpha":
        monkeypatch.setattr(dgr._C, "LOD_REMAP", "alpha")
    gc, gd = synth.upstream_grads(ke.H, ke.W, seed=3)
    bg = torch.tensor([0.1, 0.2, 0.3])
    res = pa.verify_pair(s["scene"], s["cam"], bg, gc, gd, gpu, colors_precomp=s["colors_precomp"],
                         interpolation_weights=s["interpolation_weights"], num_node_kids=s["num_node_kids"],
                         do_depth=do_depth, lod_mode=s["lod_mode"], mixed_tol=1.5 if s["lod_mode"] == "alpha" else 1.0)
    st = res["stats"]
    sides = dict(st["sides"])
    print(name, {k: v for k, v in st.items() if not isinstance(v, dict)})
    # the scene really puts its pixels on the edges, of both kinds (so that this test cannot go vacuous)
    assert st["fragile"] >= 600, st["fragile"]
    assert sides.get("alpha_live", 0) + sides.get("alpha_skip", 0) >= 300, sides
    assert sides.get("T_stop", 0) + sides.get("T_continue", 0) >= 300, sides
    pa.assert_verified(f"knife edges {name}", res, mixed_tol=GRAD_MIXED_TOL, fragile_frac=1.0)
    for k in ("color", "invdepth"):            # the pixels themselves at the default bound
        if k in st:
            assert st[k]["mixed"] <= (1.5 if s["lod_mode"] == "alpha" else 1.0), (k, st[k])
