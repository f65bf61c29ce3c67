"""TSDF fusion and surface-net extraction without a GPU: what the spec (tests/tsdf_spec.py)
produces on analytic depth maps, its invariants, the C ABI's refusals and size query, the PLY writer, the command's
parser and exits.

Figures of the spec on this file's scenes (printed by the tests):
  plane    a fronto-parallel plane at z = 1.03 seen by one camera, voxel 0.05: every vertex' z is the float32 nearest to
           1.03 -- measured maximum 0.24 ulp of the coordinate (2.9e-8); asserted with a factor of 2
  sphere   R = 0.4 at depth 1.5, four orbit cameras at 80 x 60, voxel 0.05: | |v - c| - R | at most 0.0113 against the
           bound sqrt(3) voxel + e_pix = 0.0866 + 0.1262 (e_pix is large: neighbouring pixels at the silhouette)"""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import tsdf_spec as ts
from hgs import _lib, synth

F = np.float32


# ---- a minimal reader of the PLY files write_mesh_ply writes -------------------------------------------------------------
def read_ply(path):
    """-> dict(vertices, normals, colours or None, faces) of a binary little-endian PLY with float / uchar vertex
    properties and one list property (uchar count, int indices) per face."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props, current = {}, {}, None
    for line in lines[2:-1]:
        tok = line.split()
        if tok[0] == "element":
            current = tok[1]
            counts[current] = int(tok[2])
            props[current] = []
        elif tok[0] == "property":
            props[current].append(tok[1:])
    assert list(counts) == ["vertex", "face"] and props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    vdt = np.dtype([(p[1], {"float": "<f4", "uchar": "u1"}[p[0]]) for p in props["vertex"]])
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    nv, nf = counts["vertex"], counts["face"]
    assert len(data) == end + nv * vdt.itemsize + nf * fdt.itemsize
    v = np.frombuffer(data, vdt, nv, end)
    fc = np.frombuffer(data, fdt, nf, end + nv * vdt.itemsize)
    assert (fc["n"] == 3).all()
    col = np.stack([v[k] for k in ("red", "green", "blue")], -1) if "red" in vdt.names else None
    return dict(vertices=np.stack([v[k] for k in "xyz"], -1), normals=np.stack([v["n" + k] for k in "xyz"], -1),
                colours=col, faces=fc["v"].copy())


# ---- scenes ----------------------------------------------------------------------------------------------------------------
PLANE_Z = 1.03
PLANE_ULP_MEASURED = 0.24        # ulp of the coordinate: the spec's largest distance to the plane on plane_scene()
SPHERE_C, SPHERE_R = (0.0, 0.0, 1.5), 0.4


def plane_scene():
    cam = synth.make_camera(80, 60)
    depth = ts.plane_depth(cam, (0.0, 0.0, 1.0), PLANE_Z)
    assert (depth > 0).all()
    vol = ts.new_volume((-0.3, -0.3, 0.7), 0.05, (13, 13, 13))
    return vol, [ts.view_of(cam, depth)]


def sphere_scene(colour=False):
    cams = [synth.orbit_camera(80, 60, k, 4, radius=0.6) for k in range(4)]
    depths = [ts.sphere_depth(cam, SPHERE_C, SPHERE_R) for cam in cams]
    rgb = [np.stack([(d > 0) * 0.25 * (k + 1), d * 0.3, 1.0 - d * 0.3]) for k, d in enumerate(depths)]
    vol = ts.new_volume((-0.55, -0.55, 0.95), 0.05, (23, 23, 14), colour=colour)
    return vol, [ts.view_of(cam, d, rgb=c if colour else None) for cam, d, c in zip(cams, depths, rgb)], depths


@pytest.fixture(scope="module")
def sphere():
    vol, views, depths = sphere_scene(colour=True)
    ts.integrate(vol, views)
    return vol, views, depths, ts.extract(vol, 1.0)


# ---- properties of the spec ------------------------------------------------------------------------------------------------
def test_a_fronto_parallel_plane_is_met_within_ulps():
    vol, views = plane_scene()
    seen = ts.integrate(vol, views)
    assert seen.all()
    mesh = ts.extract(vol, 1.0)
    assert mesh.vertices.shape[0] == 12 * 12 and mesh.faces.shape[0] == 2 * 11 * 11
    ulp = float(np.spacing(F(PLANE_Z)))
    err = np.abs(mesh.vertices[:, 2].astype(np.float64) - PLANE_Z) / ulp
    print(f"plane: {mesh.vertices.shape[0]} vertices, at most {err.max():.2f} ulp ({err.max() * ulp:.2e}) off z = {PLANE_Z}")
    assert err.max() <= 2 * PLANE_ULP_MEASURED
    # x and y: a crossing only along z leaves the cell's centre line
    centre = vol.lo[None, :2] + vol.voxel * (mesh.cells[:, :2].astype(F) + F(0.5))
    assert np.array_equal(mesh.vertices[:, :2], centre)
    # the surface faces the camera: normals along -z, every triangle wound to match
    assert np.array_equal(mesh.normals, np.tile(np.array([0, 0, -1], F), (mesh.vertices.shape[0], 1)))
    v = mesh.vertices.astype(np.float64)[mesh.faces]
    assert (np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])[:, 2] < 0).all()


def test_a_sphere_is_met_within_a_voxel_diagonal_and_the_pixel_step(sphere):
    vol, views, depths, mesh = sphere
    assert mesh.vertices.shape[0] > 200
    e_pix = ts.e_pix(depths)
    bound = math.sqrt(3.0) * float(vol.voxel) + e_pix
    err = np.abs(np.linalg.norm(mesh.vertices.astype(np.float64) - np.array(SPHERE_C), axis=1) - SPHERE_R)
    print(f"sphere: {mesh.vertices.shape[0]} vertices, | |v - c| - R | <= {err.max():.4f}; bound sqrt(3) voxel + e_pix = "
          f"{math.sqrt(3.0) * float(vol.voxel):.4f} + {e_pix:.4f}")
    assert err.max() <= bound
    # normals point away from the centre, colours are means of what the views painted
    out = (mesh.vertices.astype(np.float64) - np.array(SPHERE_C)) * mesh.normals
    assert (out.sum(1) > 0).all()
    assert mesh.colours.shape == mesh.vertices.shape and (mesh.colours >= 0).all() and (mesh.colours <= 1).all()


def test_a_batch_equals_a_sequence_of_single_views():
    vol, views, _ = sphere_scene(colour=True)
    one = vol.copy()
    ts.integrate(vol, views)
    for v in views:
        ts.integrate(one, [v])
    for a, b in ((vol.tsdf, one.tsdf), (vol.weight, one.weight), (vol.colour, one.colour)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_faces_are_proper_triangles_over_active_cells(sphere):
    vol, _, _, mesh = sphere
    V = mesh.vertices.shape[0]
    f = mesh.faces
    assert f.dtype == np.int32 and f.shape[0] == 2 * mesh.quad_edges.shape[0] and f.shape[0] > 0
    assert f.min() >= 0 and f.max() < V
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
    assert int(mesh.active.sum()) == V
    nx, ny, nz = vol.dims
    for (i, j, k, axis) in mesh.quad_edges[:: max(1, mesh.quad_edges.shape[0] // 200)]:
        for o in ts.quad_cells(int(axis)):
            ci, cj, ck = i + o[0], j + o[1], k + o[2]
            assert 0 <= ci < nx - 1 and 0 <= cj < ny - 1 and 0 <= ck < nz - 1 and mesh.active[ck, cj, ci]
    # vertices by ascending cell index, faces by ascending (edge, axis)
    lin = (mesh.cells[:, 2] * ny + mesh.cells[:, 1]) * nx + mesh.cells[:, 0]
    assert (np.diff(lin) > 0).all()
    e = mesh.quad_edges
    key = ((e[:, 2] * ny + e[:, 1]) * nx + e[:, 0]) * 3 + e[:, 3]
    assert (np.diff(key) > 0).all()
    # every face normal agrees with the vertex normals around it
    v = mesh.vertices.astype(np.float64)[f]
    fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    assert ((fn * mesh.normals[f].astype(np.float64).sum(1)).sum(1) > 0).all()


def test_degenerate_volumes_extract_nothing():
    for dims in ((1, 1, 1), (5, 1, 3), (2, 2, 2)):
        vol = ts.new_volume((0, 0, 0), 0.1, dims)
        vol.weight[:] = 2.0
        mesh = ts.extract(vol)
        assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3)
    vol = ts.new_volume((0, 0, 0), 0.1, (2, 2, 2))
    vol.weight[:] = 2.0
    vol.tsdf[0] = -0.5                       # one active cell: a vertex, no quad (no edge has four cells)
    mesh = ts.extract(vol)
    assert mesh.vertices.shape == (1, 3) and mesh.faces.shape == (0, 3)
    assert np.allclose(mesh.vertices[0], [0.05, 0.05, 0.1 / 3], atol=1e-7) and np.array_equal(mesh.normals[0], [0, 0, 1])


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------
FAKE = 4096          # a non-null, aligned address: every case below is refused before anything is followed


def _volume(**kw):
    f = dict(tsdf=FAKE, weight=FAKE, colour=None, lo=(C.c_float * 3)(0, 0, 0), voxel=0.1, nx=4, ny=4, nz=4, trunc=0.4,
             max_weight=math.inf)
    f.update(kw)
    return _lib.TsdfVolume(**f)


def _views(n=1, **kw):
    f = dict(depth=FAKE, weight=None, rgb=None, W=8, H=6, view=(C.c_float * 12)(*([0.0] * 12)), tanfovx=1.0, tanfovy=1.0,
             z_min=0.01)
    f.update(kw)
    return (_lib.TsdfView * 8)(*[_lib.TsdfView(**f) for _ in range(n)])


def _refused(rc, *words):
    msg = _lib.lib().hgs_last_error().decode()
    assert rc == 1, (rc, msg)
    assert all(w in msg for w in words), msg


def test_integrate_refusals_name_their_reason():
    lib = _lib.lib()
    call = lambda vol, views, n: lib.hgs_tsdf_integrate(C.byref(vol), views, n, None, 0)
    for n in (0, 9, -1):
        _refused(call(_volume(), _views(), n), "n_views")
    _refused(call(_volume(nx=2048, ny=2048, nz=512), _views(), 1), "2^31 - 1")
    _refused(call(_volume(nx=0), _views(), 1), "bad sizes")
    for bad in (0.0, -1.0, math.inf, math.nan):
        _refused(call(_volume(voxel=bad), _views(), 1), "voxel")
        _refused(call(_volume(trunc=bad), _views(), 1), "trunc")
    for bad in (0.0, -2.0, math.nan):
        _refused(call(_volume(max_weight=bad), _views(), 1), "max_weight")
    _refused(call(_volume(), _views(W=0), 1), "view 0", "pixels")
    _refused(call(_volume(), _views(H=-3), 1), "view 0", "pixels")
    _refused(call(_volume(tsdf=None), _views(), 1), "null", "tsdf")
    _refused(call(_volume(weight=None), _views(), 1), "null", "weight")
    _refused(call(_volume(), _views(depth=None), 1), "null", "depth")
    _refused(call(_volume(), _views(rgb=FAKE), 1), "rgb", "colour")
    two = _views(2)
    two[1].depth = None
    _refused(call(_volume(), two, 2), "depth of view 1")
    _refused(lib.hgs_tsdf_integrate(None, _views(), 1, None, 0), "null")
    _refused(lib.hgs_tsdf_integrate(C.byref(_volume()), None, 1, None, 0), "null")


def test_extract_refusals_name_their_reason():
    lib = _lib.lib()
    totals = (C.c_int64 * 2)()
    plan = lambda vol, mw=1.0, tmp=FAKE: lib.hgs_tsdf_extract_plan(C.byref(vol), mw, tmp, totals, None, 0)
    apply_ = lambda vol, tmp=FAKE, v=FAKE, n=FAKE, c=None, f=FAKE: lib.hgs_tsdf_extract_apply(C.byref(vol), tmp, v, n, c, f, None, 0)
    for bad in (0.0, -1.0, math.inf, math.nan):
        _refused(plan(_volume(), mw=bad), "min_weight")
        _refused(plan(_volume(voxel=bad)), "voxel")
        _refused(apply_(_volume(trunc=bad)), "trunc")
    _refused(plan(_volume(max_weight=0.0)), "max_weight")
    _refused(plan(_volume(), tmp=None), "null", "tmp")
    _refused(apply_(_volume(), tmp=None), "null", "tmp")
    _refused(plan(_volume(), tmp=FAKE + 4), "aligned")
    _refused(plan(_volume(tsdf=None)), "null")
    _refused(apply_(_volume(weight=None)), "null")
    _refused(plan(_volume(nx=2048, ny=2048, nz=512)), "2^31 - 1")
    _refused(plan(_volume(nx=2048, ny=2048, nz=400)), "32-bit")        # a volume, but not one to extract from
    _refused(apply_(_volume(), c=FAKE), "colours", "no colour")
    _refused(apply_(_volume(), v=None), "null")
    _refused(apply_(_volume(), f=None), "null")
    _refused(apply_(_volume()), "hgs_tsdf_extract_plan")               # no plan on this (device, tmp)


def test_the_size_query_needs_no_gpu():
    lib = _lib.lib()
    up = lambda b: (b + 255) // 256 * 256
    for dims in ((1, 1, 1), (2, 2, 2), (65, 7, 9), (512, 512, 512)):
        N = dims[0] * dims[1] * dims[2]
        nblk = (N + 255) // 256
        chunks = max(1, (nblk + 8191) // 8192)
        assert lib.hgs_tsdf_extract_tmp_bytes(*dims) == 3 * up(N) + 2 * up(4 * (nblk + 1)) + 2 * up(8 * chunks), dims
    assert lib.hgs_tsdf_extract_tmp_bytes(0, 4, 4) == 0 and lib.hgs_tsdf_extract_tmp_bytes(4, -1, 4) == 0
    assert lib.hgs_tsdf_extract_tmp_bytes(2048, 2048, 512) == 0 and lib.hgs_tsdf_extract_tmp_bytes(2048, 2048, 400) == 0
    assert lib.hgs_tsdf_extract_tmp_bytes(2048, 2048, 341) > 0


def test_struct_layouts_match_the_header():
    assert C.sizeof(_lib.TsdfVolume) == 64 and _lib.TsdfVolume.voxel.offset == 36 and _lib.TsdfVolume.trunc.offset == 52
    assert C.sizeof(_lib.TsdfView) == 96 and _lib.TsdfView.view.offset == 32 and _lib.TsdfView.z_min.offset == 88


# ---- Python layer -----------------------------------------------------------------------------------------------------------
def test_the_ply_writer_round_trips(sphere, tmp_path):
    from hgs.meshing import write_mesh_ply
    _, _, _, mesh = sphere
    m = dict(vertices=mesh.vertices, normals=mesh.normals, colours=mesh.colours, faces=mesh.faces)
    path = tmp_path / "sub" / "mesh.ply"
    write_mesh_ply(str(path), m)
    back = read_ply(path)
    assert np.array_equal(back["vertices"].view(np.uint32), mesh.vertices.view(np.uint32))
    assert np.array_equal(back["normals"].view(np.uint32), mesh.normals.view(np.uint32))
    assert np.array_equal(back["faces"], mesh.faces)
    assert np.array_equal(back["colours"], np.rint(np.clip(mesh.colours.astype(np.float64), 0, 1) * 255).astype(np.uint8))
    m.pop("colours")
    write_mesh_ply(str(path), m)
    back = read_ply(path)
    assert back["colours"] is None and np.array_equal(back["faces"], mesh.faces)
    empty = dict(vertices=np.zeros((0, 3), F), normals=np.zeros((0, 3), F), faces=np.zeros((0, 3), np.int32))
    write_mesh_ply(str(path), empty)
    assert read_ply(path)["vertices"].shape == (0, 3)


def test_volume_dims_and_the_voxel_that_fits():
    from hgs import meshing
    assert meshing.volume_dims((0, 0, 0), (1, 0.5, 0), 0.25) == (5, 3, 1)
    assert meshing.volume_dims((-1, -1, -1), (-1, -1, -1), 0.1) == (1, 1, 1)
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="voxel"):
            meshing.volume_dims((0, 0, 0), (1, 1, 1), bad)
    with pytest.raises(ValueError, match="lo <= hi"):
        meshing.volume_dims((0, 0, 0), (1, -1, 1), 0.1)
    lo, hi = (0, 0, 0), (100, 100, 20)
    s = meshing.fitting_voxel(lo, hi)
    n = meshing.volume_dims(lo, hi, s)
    assert n[0] * n[1] * n[2] <= meshing.MAX_EXTRACT_SAMPLES < np.prod(meshing.volume_dims(lo, hi, s * 0.97), dtype=np.int64)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            meshing.TsdfVolume((0, 0, 0), (1, 1, 1), 0.1)


# ---- the command -------------------------------------------------------------------------------------------------------------
def test_the_commands_parser():
    from hgs import mesh_hierarchy as mh
    base = ["in.hier", "out.ply", "--cameras", "c.json", "--voxel", "0.05"]
    a = mh.parse_args(base + ["--roi", "0", "0", "0", "1", "2", "3"])
    assert a == dict(in_path="in.hier", out_path="out.ply", cameras="c.json", roi=(0, 0, 0, 1, 2, 3), voxel=0.05, trunc=None,
                     tau_px=0.0, min_alpha=0.5, min_weight=1.0, colour=True, frustum=True, resolution_scale=1.0,
                     volume_out=None)
    a = mh.parse_args(["--roi-root", "--no-colour", "--trunc", "0.3", "--tau-px", "3", "--min-alpha", "0.8", "--min-weight",
                       "2", "--no-frustum", "--resolution-scale", "2", "--volume-out", "v.npz"] + base)
    assert a["roi"] is None and not a["colour"] and not a["frustum"] and a["trunc"] == 0.3 and a["tau_px"] == 3.0
    assert a["min_alpha"] == 0.8 and a["min_weight"] == 2.0 and a["resolution_scale"] == 2.0 and a["volume_out"] == "v.npz"
    roi = ["--roi", "0", "0", "0", "1", "1", "1"]
    for bad in (base,                                            # no region
                base + roi + ["--roi-root"],                     # two regions
                base[:1] + base[2:] + roi,                       # one path
                base[:2] + ["--voxel", "0.05"] + roi,            # no cameras
                base[:4] + roi,                                  # no voxel
                base + ["--roi", "0", "0", "0", "1", "1"],       # five numbers
                base + ["--roi", "0", "0", "2", "1", "1", "1"],  # lo > hi
                base + ["--roi", "0", "0", "x", "1", "1", "1"],
                base + roi + ["--voxel", "0.1"],                 # twice
                base[:4] + ["--voxel", "0"] + roi, base[:4] + ["--voxel", "-1"] + roi, base[:4] + ["--voxel", "inf"] + roi,
                base + roi + ["--trunc", "0"], base + roi + ["--min-weight", "0"], base + roi + ["--min-alpha", "1.5"],
                base + roi + ["--tau-px", "-1"], base + roi + ["--resolution-scale", "0"], base + roi + ["--frobnicate"],
                base + roi + ["--no-colour", "--no-colour"]):
        assert mh.parse_args(bad) is None, bad


def test_the_commands_exits(tmp_path, capsys):
    from hgs import mesh_hierarchy as mh
    hier, cams = tmp_path / "in.hier", tmp_path / "cameras.json"
    hier.write_bytes(b"")
    cam = synth.make_camera(16, 12)
    c2w = cam.world_view_transform.t().double().inverse()
    cams.write_text(json.dumps([dict(width=16, height=12, fx=10.0, fy=10.0, position=c2w[:3, 3].tolist(),
                                     rotation=c2w[:3, :3].tolist())]))
    out = tmp_path / "out.ply"
    args = [str(hier), str(out), "--cameras", str(cams), "--voxel", "0.0625"]
    assert mh.main(args) == 2 and "usage:" in capsys.readouterr().err                       # no region
    assert mh.main([str(tmp_path / "none.hier")] + args[1:] + ["--roi-root"]) == 2
    assert "does not exist" in capsys.readouterr().err
    bad = tmp_path / "bad.json"
    bad.write_text("[{}]")
    assert mh.main(args[:2] + ["--cameras", str(bad), "--voxel", "0.0625", "--roi-root"]) == 2
    assert "camera 0" in capsys.readouterr().err
    # a region of too many samples: refused before the file is read, the voxel that fits is named and does fit
    roi = ["--roi", "0", "0", "0", "100", "100", "100"]
    assert mh.main(args + roi) == 1
    err = capsys.readouterr().err
    assert "nothing written" in err and "1601 x 1601 x 1601" in err and "--voxel" in err and not out.exists()
    fits = float(err.split("--voxel ")[-1].split()[0])
    from hgs import meshing
    assert np.prod(meshing.volume_dims((0, 0, 0), (100, 100, 100), fits), dtype=np.int64) <= meshing.MAX_EXTRACT_SAMPLES
