"""The calls the reference's own code makes, replayed through the HIP op.  tests/golden/boundary_*.npz hold what
gaussian_renderer/__init__.py's render / render_post / render_coarse and GaussianModel.create_from_pcd passed across
this repository's boundary while they ran on the CPU oracle (tests/golden/make_boundary_golden.py); this file reads only
those fixtures:

  * every op call, with its settings and arguments placed where the reference places them: radii and every integer
    exact, pixels and every gradient -- means2D on exactly the rows the reference's screen-space tensor has -- within
    REL_TOL of the oracle, every knife-edge pixel on an admissible outcome (``parity.verify``);
  * ``_C.lod_gather`` on the recorded full arrays: bit-identical to the rows the reference's lerp built;
  * every render_post call again through the in-op LOD path (non-empty indices, ``RasterContext(skybox_points=...)``,
    with and without the in-kernel scatter): the same image and radii as the op on the reference-made rows with the
    reference's overwritten weights and kids, and every full-array gradient within REL_TOL of the reference's leaf
    gradients, exactly zero on rows that are neither drawn, nor parents, nor skybox;
  * ``expand_to_size`` / ``get_interpolation_weights`` with the recorded mixed devices and capacities: count, index
    arrays and kids exact, weights as bit patterns;
  * ``distCUDA2`` on the recorded point clouds: within rtol 1e-5 of the float64 brute force."""
import numpy as np
import pytest
import torch

import boundary_fixtures as bf
import parity as pa

pytestmark = pytest.mark.gpu

OPS = bf.cases("op")
LODS = bf.cases("lod")
CUTS = bf.cases("cut")
KNNS = bf.cases("knn")
_ids = lambda cs: [f"{f[:-4]}-{p}" for f, p in cs]


def _load(name):
    return bf.load(f"{bf.GOLDEN}/{name}")


def _upstream(z, op):
    """The recorded upstream gradients; zeros where no backward ran (render_hierarchy.py renders under no_grad)."""
    if f"{op}__gin__color" not in z:
        return torch.zeros(z[f"{op}__out__color"].shape), None
    gc = torch.from_numpy(z[f"{op}__gin__color"].copy())
    gd = torch.from_numpy(z[f"{op}__gin__invdepth"].copy()) if f"{op}__gin__invdepth" in z else None
    return gc, gd


def test_fixtures_are_there():
    assert len(OPS) >= 13 and len(LODS) >= 4 and len(CUTS) >= 7 and len(KNNS) >= 3, (len(OPS), len(LODS), len(CUTS))
    assert "boundary_chain.npz" in {f for f, _ in OPS} | {f for f, _ in CUTS} | {f for f, _ in KNNS}


@pytest.mark.parametrize("name,op", OPS, ids=_ids(OPS))
def test_op_call_replays(gpu, name, op):
    z = _load(name)
    st, ar = bf.settings(z, op, gpu), bf.args(z, op, gpu)
    gc, gd = _upstream(z, op)
    do_depth = bool(st["do_depth"]) and gd is not None
    hip = pa.run_call(st, ar, gc, gd if do_depth else None)
    assert torch.equal(hip["radii"], torch.from_numpy(z[f"{op}__out__radii"]))
    orc = pa.oracle_call(st, ar)
    res = pa.verify(hip, orc, gc, gd if do_depth else torch.zeros(1, st["image_height"], st["image_width"]),
                    do_depth=do_depth)
    res["indices"] = pa.check_indices(hip, res["oracle"])
    print(name, op, {k: (v["maxrel"], v["l2"]) if isinstance(v, dict) else v for k, v in res["stats"].items()})
    pa.assert_verified(f"{name} {op}", res)
    if f"{op}__gout__means2D" not in z:
        return
    # the means2D gradient: one row per row the op drew, the rows the reference's screen-space tensor receives
    g2 = z[f"{op}__gout__means2D"]
    assert hip["grads"]["means2D"].shape == g2.shape
    st2 = pa.err_stats(hip["grads"]["means2D"], torch.from_numpy(g2))
    assert st2["maxrel"] <= pa.REL_TOL and st2["l2"] <= pa.REL_TOL, st2


def _lod(z, lod, gpu):
    op = f"op{int(z[f'{lod}__op'])}"
    full = {k: torch.from_numpy(z[f"{lod}__full__{k}"].copy()).to(gpu) for k in bf.FULL}
    ri = torch.from_numpy(z[f"{lod}__render_indices"].copy()).to(gpu)
    pi = torch.from_numpy(z[f"{lod}__parent_indices"].copy()).to(gpu)
    w = torch.from_numpy(z[f"{lod}__weights"].copy()).to(gpu)
    kids = torch.from_numpy(z[f"{lod}__kids"].copy()).to(gpu)
    return op, full, ri, pi, w, kids, int(z[f"{lod}__skybox"])


@pytest.mark.parametrize("name,lod", LODS, ids=_ids(LODS))
def test_lod_gather_reproduces_the_reference_rows(gpu, name, lod):
    import diff_gaussian_rasterization as dgr
    z = _load(name)
    op, full, ri, pi, w, kids, sky = _lod(z, lod, gpu)
    n = ri.numel()
    rows = dgr._C.lod_gather(ri, pi, w, full["xyz"], full["scaling"], full["rotation"], full["features"],
                             full["opacity"])
    for k, got in zip(("xyz", "scaling", "rotation", "features", "opacity"), rows):
        want = torch.from_numpy(z[f"{op}__arg__{bf.ROW_ARG[k]}"][:n].copy())
        assert torch.equal(got.cpu(), want), (k, int((got.cpu() != want).sum()))


@pytest.mark.parametrize("in_kernel", [True, False], ids=["in_kernel_scatter", "separate_scatter"])
@pytest.mark.parametrize("name,lod", LODS, ids=_ids(LODS))
def test_in_op_lod_matches_the_reference_glue(gpu, name, lod, in_kernel, monkeypatch):
    import diff_gaussian_rasterization as dgr
    z = _load(name)
    op, full, ri, pi, w, kids, sky = _lod(z, lod, gpu)
    n, G = ri.numel(), full["xyz"].shape[0]
    gc, _ = _upstream(z, op)
    st = bf.settings(z, op, gpu)
    # (a) the op on the rows the reference's glue built, with its overwritten weights / kids (as recorded)
    a = pa.run_call(st, bf.args(z, op, gpu), gc, None)
    # (b) the in-op LOD path on the full arrays
    monkeypatch.setattr(dgr._C, "lod_scatter_in_kernel", in_kernel)
    leaves = {k: v.clone().requires_grad_(True) for k, v in full.items()}
    m2 = torch.zeros(G, 3, device=gpu, requires_grad=True)
    st_b = dict(st, render_indices=ri, parent_indices=pi, interpolation_weights=w, num_node_kids=kids)
    ctx = dgr.RasterContext(skybox_points=sky) if sky else None
    color, radii, _ = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**st_b), context=ctx)(
        means3D=leaves["xyz"], means2D=m2, shs=leaves["features"], opacities=leaves["opacity"],
        scales=leaves["scaling"], rotations=leaves["rotation"])
    (color * gc.to(gpu)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(radii.cpu(), a["radii"])
    assert torch.equal(color.detach().cpu(), a["color"]), float((color.detach().cpu() - a["color"]).abs().max())
    assert torch.equal(kids.cpu(), torch.from_numpy(z[f"{lod}__kids"])), "the caller's kids must be left untouched"
    assert torch.equal(w.cpu(), torch.from_numpy(z[f"{lod}__weights"])), "the caller's weights must be left untouched"
    touched = torch.zeros(G, dtype=torch.bool)
    touched[ri.long().cpu()] = True
    touched[pi[:n].long().cpu()] = True
    touched[G - sky:] = sky > 0
    for k in bf.FULL:
        got, want = leaves[k].grad.cpu(), torch.from_numpy(z[f"{lod}__leafgrad__{k}"])
        s = pa.err_stats(got, want)
        assert s["maxrel"] <= pa.REL_TOL and s["l2"] <= pa.REL_TOL, (k, s)
        assert float(got[~touched].abs().sum()) == 0.0, k
    s = pa.err_stats(m2.grad.cpu(), torch.from_numpy(z[f"{lod}__viewspace_grad"]))
    assert s["maxrel"] <= pa.REL_TOL and s["l2"] <= pa.REL_TOL, ("means2D", s)
    assert float(m2.grad[n + sky:].abs().sum()) == 0.0


@pytest.mark.parametrize("name,cut", CUTS, ids=_ids(CUTS))
def test_cut_calls_replay_exactly(gpu, name, cut):
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    z = _load(name)
    t = lambda k: torch.from_numpy(z[f"{cut}__{k}"].copy())
    nodes, boxes = t("nodes").to(gpu), t("boxes").to(gpu)
    cap = z[f"{cut}__capacity"]
    ri, pi, ni = (torch.zeros(int(c), dtype=torch.int32, device=gpu) for c in cap)
    # train_post.py:91-113: viewpoint on the GPU for the cut, on the CPU for the weights; viewdir torch.zeros((3))
    n = expand_to_size(nodes, boxes, float(z[f"{cut}__size"]), t("viewpoint").to(gpu), t("viewdir"), ri, pi, ni)
    assert n == int(z[f"{cut}__count"])
    for k, v in (("render_indices", ri), ("parent_indices", pi), ("nodes_for_render_indices", ni)):
        assert np.array_equal(v[:n].cpu().numpy(), z[f"{cut}__{k}"]), k
    wc = z[f"{cut}__w_capacity"]
    w = torch.zeros(int(wc[0]), device=gpu)
    kids = torch.zeros(int(wc[1]), dtype=torch.int32, device=gpu)
    get_interpolation_weights(ni[:n], float(z[f"{cut}__w_size"]), nodes, boxes, t("w_viewpoint"), torch.zeros((3)), w,
                              kids)
    assert np.array_equal(w[:n].cpu().numpy().view(np.uint32), z[f"{cut}__weights"].view(np.uint32))
    assert np.array_equal(kids[:n].cpu().numpy(), z[f"{cut}__kids"])


@pytest.mark.parametrize("name,knn", KNNS, ids=_ids(KNNS))
def test_dist_knn3_on_the_point_clouds_create_from_pcd_hands_it(gpu, name, knn):
    from simple_knn._C import distCUDA2
    z = _load(name)
    got = distCUDA2(torch.from_numpy(z[f"{knn}__points"].copy()).to(gpu)).cpu()
    want = torch.from_numpy(z[f"{knn}__dist"])
    rel = ((got.double() - want.double()).abs() / want.double().abs().clamp_min(1e-30)).max().item()
    assert torch.allclose(got, want, rtol=1e-5, atol=0.0), rel
