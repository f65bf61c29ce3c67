"""Host side of the hierarchy creator (no GPU): the PLY reader against the test fixture's reader, its rejections, the
row selection of ``python -m hgs.create_hierarchy``, the size checks of the C ABI and the resources of the builder's
kernels."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from harness import ply_to_hier            # noqa: F401  (puts the plyfile shim on sys.path)
from hgs import _lib, create_hierarchy, ply
from hier_build_common import save_ply_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc")


@pytest.mark.parametrize("M", [16, 4])
def test_ply_reader_matches_the_fixture_reader(tmp_path, M):
    path = str(tmp_path / "point_cloud.ply")
    save_ply_layout(path, 257, M, seed=M)
    got = ply.read_ply(path)
    want = ply_to_hier.scene_from_ply(path)                  # [P,16,3] SH, zero-padded
    assert got.shs.shape == (257, M, 3) and got.sh_degree == int(np.sqrt(M)) - 1
    for name in ("means3D", "scales", "rotations", "opacities"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert torch.equal(got.shs, want.shs[:, :M])
    assert float(want.shs[:, M:].abs().sum()) == 0.0


def test_ply_reader_degree_0(tmp_path):
    """M = 1 (no f_rest): the fixture reader needs f_rest properties, so the same rows are written once with M = 16 (read
    by the fixture) and once without f_rest (read by the product reader)."""
    from plyfile import PlyData, PlyElement
    full = str(tmp_path / "full.ply")
    el = save_ply_layout(full, 300, 16, seed=3)
    names = [n for n in el.dtype.names if not n.startswith("f_rest_")]
    dc = np.zeros(el.shape[0], dtype=[(n, "f4") for n in names])
    for n in names:
        dc[n] = el[n]
    path = str(tmp_path / "dc.ply")
    PlyData([PlyElement.describe(dc, "vertex")]).write(path)
    got = ply.read_ply(path)
    want = ply_to_hier.scene_from_ply(full)
    assert got.shs.shape == (300, 1, 3) and got.sh_degree == 0
    for name in ("means3D", "scales", "rotations", "opacities"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert torch.equal(got.shs, want.shs[:, :1])


def _write_raw(path, fmt, props, P=4, dtype="<f4"):
    head = ["ply", f"format {fmt} 1.0", f"element vertex {P}"] + [f"property {t} {n}" for n, t in props] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if fmt == "ascii":
            for _ in range(P):
                f.write((" ".join("0" for _ in props) + "\n").encode())
        else:
            f.write(np.zeros(P * len(props), dtype=dtype).tobytes())


_LAYOUT = [(n, "float") for n in ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity",
                                  "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]]


@pytest.mark.parametrize("case,props,fmt,needle", [
    ("ascii", _LAYOUT, "ascii", "ascii"),
    ("big_endian", _LAYOUT, "binary_big_endian", "binary_big_endian"),
    ("missing_rot_3", _LAYOUT[:-1], "binary_little_endian", "rot_3"),
    ("double", [(n, "double" if n == "scale_1" else t) for n, t in _LAYOUT], "binary_little_endian", "scale_1"),
])
def test_ply_reader_rejects_what_save_ply_does_not_write(tmp_path, case, props, fmt, needle):
    path = str(tmp_path / f"{case}.ply")
    _write_raw(path, fmt, props, dtype=">f4" if "big" in fmt else "<f4")
    with pytest.raises(ply.PlyFormatError, match=needle):
        ply.read_ply(path)
    # the unmodified layout reads
    good = str(tmp_path / "good.ply")
    _write_raw(good, "binary_little_endian", _LAYOUT)
    assert ply.read_ply(good).P == 4


def test_select_rows_drops_the_skybox_and_applies_the_chunk_bounds(tmp_path):
    half = 2.0                                                # extent 4 -> |d| <= 2 kept
    up = float(np.nextafter(np.float32(2.5), np.float32(10)))
    xyz = torch.tensor([[9.0, 9.0, 9.0],                      # skybox rows (far outside: dropped as skybox anyway)
                        [0.5, 0.5, 0.0],
                        [2.5, 0.5, 7.0],                       # |dx| = 2 exactly: kept (z plays no part)
                        [up, 0.5, 0.0],                        # one float above: dropped
                        [0.5, -1.5, 0.0],                      # |dy| = 2: kept
                        [0.5, -1.5000002, 0.0],                # dropped
                        [0.5, 0.5, -100.0]])                   # kept
    bounds = (torch.tensor([0.5, 0.5, 0.0]), torch.tensor([2 * half, 1.0, 1.0]))
    assert create_hierarchy.select_rows(xyz, 1, bounds).tolist() == [1, 2, 4, 6]
    assert create_hierarchy.select_rows(xyz, 2, bounds).tolist() == [2, 4, 6]
    assert create_hierarchy.select_rows(xyz, 0, None).tolist() == list(range(7))
    assert create_hierarchy.select_rows(xyz, 3, None).tolist() == [3, 4, 5, 6]
    # bounds files as the reference writes them
    chunk = tmp_path / "chunk"
    chunk.mkdir()
    assert create_hierarchy.read_chunk_bounds(str(chunk)) is None       # no bounds files: every row
    (chunk / "center.txt").write_text("0.5 0.5 0.0\n")
    assert create_hierarchy.read_chunk_bounds(str(chunk)) is None       # both are needed
    (chunk / "extent.txt").write_text("4.0 1.0 1.0\n")
    c, e = create_hierarchy.read_chunk_bounds(str(chunk))
    assert c.tolist() == [0.5, 0.5, 0.0] and e.tolist() == [4.0, 1.0, 1.0]
    assert create_hierarchy.select_rows(xyz, 1, (c, e)).tolist() == [1, 2, 4, 6]


def test_skybox_count_comes_from_beside_the_ply_then_the_scaffold(tmp_path):
    model = tmp_path / "model"; model.mkdir()
    scaffold = tmp_path / "scaffold"; scaffold.mkdir()
    ply_path = str(model / "point_cloud.ply")
    assert create_hierarchy.read_skybox_count(ply_path, str(scaffold)) == 0
    assert create_hierarchy.read_skybox_count(ply_path) == 0
    (scaffold / "pc_info.txt").write_text("100000")
    assert create_hierarchy.read_skybox_count(ply_path, str(scaffold)) == 100000
    (model / "pc_info.txt").write_text("123\n")
    assert create_hierarchy.read_skybox_count(ply_path, str(scaffold)) == 123


def test_command_usage_error_without_a_gpu():
    assert create_hierarchy.main(["only", "two"]) == 2


def test_tmp_bytes_need_no_gpu_and_grow_with_P():
    lib = _lib.lib()
    sizes = [lib.hgs_hier_build_tmp_bytes(p) for p in (1, 2, 1000, 1_000_000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[-2]
    assert sizes[-1] >= 1_000_000 * (3 * 4 + (2 - 1e-6) * 88)     # keys, order, per-node range + double moments
    for bad in (0, -1, (1 << 30) + 1):
        assert lib.hgs_hier_build_tmp_bytes(bad) == 0
    assert lib.hgs_hier_build_tmp_bytes(1 << 30) > 0


@pytest.mark.parametrize("P,M,needle", [(0, 16, b"P=0"), (-5, 16, b"P=-5"), ((1 << 30) + 1, 16, b"P=1073741825"),
                                        (10, 2, b"M=2"), (10, 0, b"M=0"), (10, 25, b"M=25")])
def test_build_checks_sizes_before_touching_the_device(P, M, needle):
    """Returns an error with a message, without a GPU and before any HIP call (every pointer is null here)."""
    lib = _lib.lib()
    rc = lib.hgs_hier_build(*([None] * 5), P, M, *([None] * 7), None, None, 0)
    assert rc != 0
    msg = lib.hgs_last_error()
    assert b"bad sizes" in msg and needle in msg, msg


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("c++filt")),
                    reason="needs hipcc (cross-compiles without a GPU) and c++filt")
def test_builder_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    rows = {r["kernel"]: r for r in kernel_resources.collect([os.path.join(CSRC, "hier_build.hip")])}
    for k in ("hb_bounds_kernel", "hb_morton_kernel", "hb_root_kernel", "hb_level_kernel", "hb_merge_kernel"):
        assert k in rows, (k, sorted(rows))
    for k, r in rows.items():
        assert r["scratch"] == 0, f"{k} uses {r['scratch']} bytes of scratch per lane"
