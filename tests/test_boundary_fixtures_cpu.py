"""The boundary fixtures without a GPU: schema and size limits, the oracle and the LOD oracle still reproducing what
was recorded (drift guards), the shared torch restatement of render_post's lerp bit for bit against the rows the
reference's own code built, and -- where a reference checkout exists -- a regeneration that must reproduce every
array of the committed direct-call files."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import boundary_fixtures as bf
import parity as pa
from harness.recorder import ARGS, SETTINGS
from oracle import lod_oracle as lo

REF = os.environ.get("HGS_REFERENCE", "/root/reference")
FILES = bf.files()
_KEY = re.compile(r"^(op\d+__(site|fragile|set__(%s)|arg__(%s)|out__(color|radii|invdepth)|gin__(color|invdepth)|"
                  r"gout__(%s))|lod\d+__(op|skybox|render_indices|parent_indices|weights|kids|viewspace_grad|"
                  r"(full|leafgrad)__(%s))|cut\d+__(nodes|boxes|size|viewpoint|viewdir|capacity|count|render_indices|"
                  r"parent_indices|nodes_for_render_indices|w_size|w_viewpoint|w_capacity|weights|kids)|"
                  r"knn\d+__(points|dist))$" % ("|".join(SETTINGS), "|".join(ARGS), "|".join(ARGS), "|".join(bf.FULL)))


def _z(path):
    return bf.load(path)


def test_fixture_files_respect_schema_and_size_limits():
    names = [os.path.basename(f) for f in FILES]
    assert names == sorted(["boundary_chain.npz", "boundary_direct.npz"] + [f"boundary_lod_{c}.npz" for c in
                                                      ("cut", "cut_skybox", "cut_deg1", "edges")]), names
    sizes = [os.path.getsize(f) for f in FILES]
    assert max(sizes) <= 1 << 20 and sum(sizes) <= 4 << 20, sizes
    for f in FILES:
        z = _z(f)                                           # (np.load with allow_pickle=False)
        for k, v in z.items():
            assert _KEY.match(k), (f, k)
            assert v.dtype.kind in "biuf", (f, k, v.dtype)
        for op in bf.records(z, "op"):
            assert all(f"{op}__set__{s}" in z for s in SETTINGS), (f, op)
            assert int(z[f"{op}__site"]) in (0, 1, 2) and z[f"{op}__set__image_height"].ndim == 0
            for k in ("out__color", "out__radii", "out__invdepth", "arg__means3D", "arg__means2D"):
                assert f"{op}__{k}" in z, (f, op, k)
            # a backward ran (both sides of it recorded) or none did (render_hierarchy.py renders under no_grad)
            assert (f"{op}__gin__color" in z) == (f"{op}__gout__means2D" in z), (f, op)
            assert f"{op}__gin__color" in z or os.path.basename(f) == "boundary_chain.npz", (f, op)
        for lod in bf.records(z, "lod"):
            op = f"op{int(z[f'{lod}__op'])}"
            assert int(z[f"{op}__site"]) == 1 and int(z[f"{op}__fragile"]) == 0, (f, lod)
    sites = [int(_z(f)[f"{op}__site"]) for f in FILES for op in bf.records(_z(f), "op")]
    assert sorted(set(sites)) == [0, 1, 2]


@pytest.mark.parametrize("name,op", bf.cases("op"), ids=[f"{f[:-4]}-{p}" for f, p in bf.cases("op")])
def test_oracle_reproduces_the_recorded_op_calls(name, op):
    z = _z(os.path.join(bf.GOLDEN, name))
    st, ar = bf.settings(z, op, "cpu"), bf.args(z, op, "cpu")
    orc = pa.oracle_call(st, ar)
    out = orc()
    assert np.array_equal(out.radii.numpy() if torch.is_tensor(out.radii) else out.radii, z[f"{op}__out__radii"])
    assert int(out.fragile.sum()) == int(z[f"{op}__fragile"])
    close = lambda a, b: float((a.double() - b.double()).abs().max()) <= 1e-6 * max(float(b.abs().max()), 1e-30)
    assert close(out.color.detach(), torch.from_numpy(z[f"{op}__out__color"]))
    if bool(st["do_depth"]):           # (without depth the op returns zeros, which the oracle does not compute)
        assert close(out.invdepth.detach().reshape(z[f"{op}__out__invdepth"].shape),
                     torch.from_numpy(z[f"{op}__out__invdepth"]))
    if f"{op}__gin__color" not in z:
        return
    loss = (out.color * torch.from_numpy(z[f"{op}__gin__color"]).double()).sum()
    if f"{op}__gin__invdepth" in z:
        loss = loss + (out.invdepth * torch.from_numpy(z[f"{op}__gin__invdepth"]).double()).sum()
    loss.backward()
    grads = orc.grads()
    for n in ARGS:
        if f"{op}__gout__{n}" in z:
            assert close(grads[n].reshape(z[f"{op}__gout__{n}"].shape), torch.from_numpy(z[f"{op}__gout__{n}"])), n


@pytest.mark.parametrize("name,cut", bf.cases("cut"), ids=[f"{f[:-4]}-{p}" for f, p in bf.cases("cut")])
def test_lod_oracle_reproduces_the_recorded_cuts(name, cut):
    z = _z(os.path.join(bf.GOLDEN, name))
    r, p, nn = lo.expand_to_size(z[f"{cut}__nodes"], z[f"{cut}__boxes"], float(z[f"{cut}__size"]),
                                 z[f"{cut}__viewpoint"])
    assert len(r) == int(z[f"{cut}__count"]) <= int(z[f"{cut}__capacity"].min())
    assert np.array_equal(r, z[f"{cut}__render_indices"]) and np.array_equal(p, z[f"{cut}__parent_indices"])
    assert np.array_equal(nn, z[f"{cut}__nodes_for_render_indices"])
    w, k = lo.get_interpolation_weights(nn, float(z[f"{cut}__w_size"]), z[f"{cut}__nodes"], z[f"{cut}__boxes"],
                                        z[f"{cut}__w_viewpoint"])
    assert np.array_equal(w.view(np.uint32), z[f"{cut}__weights"].view(np.uint32)) and np.array_equal(k, z[f"{cut}__kids"])


@pytest.mark.parametrize("name,lod", bf.cases("lod"), ids=[f"{f[:-4]}-{p}" for f, p in bf.cases("lod")])
def test_lerp_helper_matches_the_reference_rows_bit_for_bit(name, lod):
    """tests/boundary_fixtures.lod_lerp (what tests/test_lod_gpu.py feeds the op) against the rows the reference's
    render_post built, the skybox tail it appended and the weights / kids it overwrote."""
    z = _z(os.path.join(bf.GOLDEN, name))
    op = f"op{int(z[f'{lod}__op'])}"
    full = {k: torch.from_numpy(z[f"{lod}__full__{k}"]) for k in bf.FULL}
    ri = torch.from_numpy(z[f"{lod}__render_indices"]).long()
    n, sky, G = ri.numel(), int(z[f"{lod}__skybox"]), full["xyz"].shape[0]
    pi = torch.from_numpy(z[f"{lod}__parent_indices"])[:n].long()
    w = torch.from_numpy(z[f"{lod}__weights"])
    rows = bf.lod_lerp(full, ri, pi, w[:n])
    for k in bf.FULL:
        got = torch.from_numpy(z[f"{op}__arg__{bf.ROW_ARG[k]}"])
        assert got.shape[0] == n + sky
        assert torch.equal(rows[k], got[:n]), k
        assert torch.equal(full[k][G - sky:], got[n:]), k                 # the skybox: the LAST sky rows, in order
    w_op = torch.from_numpy(z[f"{op}__set__interpolation_weights"])
    k_op = torch.from_numpy(z[f"{op}__set__num_node_kids"])
    kids = torch.from_numpy(z[f"{lod}__kids"])
    assert torch.equal(w_op[:n], w[:n]) and torch.equal(k_op[:n], kids[:n])
    assert bool((w_op[n:n + sky] == 1).all()) and bool((k_op[n:n + sky] == 1).all())
    assert torch.equal(w_op[n + sky:], w[n + sky:]) and torch.equal(k_op[n + sky:], kids[n + sky:])
    assert z[f"{op}__set__render_indices"].size == 0 and z[f"{op}__set__parent_indices"].size == 0
    g = z[f"{lod}__viewspace_grad"]
    assert np.array_equal(g[:n + sky], z[f"{op}__gout__means2D"]) and not g[n + sky:].any()


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gaussian_renderer")), reason="no reference checkout (HGS_REFERENCE)")
def test_direct_call_fixtures_regenerate():
    spec = importlib.util.spec_from_file_location("make_boundary_golden",
                                                  os.path.join(bf.GOLDEN, "make_boundary_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    files = gen.build(REF)                  # (the chain samples get the schema check only: training drifts with BLAS)
    assert sorted(files) == sorted(os.path.basename(f) for f in FILES if not f.endswith("boundary_chain.npz"))
    for name, arrs in files.items():
        z = _z(os.path.join(bf.GOLDEN, name))
        assert sorted(arrs) == sorted(z), name
        for k, v in arrs.items():
            ref = z[k]
            assert v.dtype == ref.dtype and v.shape == ref.shape, (name, k)
            if v.dtype.kind == "f":
                scale = float(np.abs(ref).max()) if ref.size else 0.0
                assert float(np.abs(v.astype(np.float64) - ref).max(initial=0.0)) <= 1e-6 * max(scale, 1e-30), (name, k)
            else:
                assert np.array_equal(v, ref), (name, k)
