"""Host side of the hierarchy merger (no GPU): the command's usage errors, the .hier header peek against the loader, the
size checks of the C ABI and the resources of the merger's kernels."""
import ctypes as C
import os
import shutil
import struct
import sys

import pytest
import torch

from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
from hgs import _lib, hierarchy, merge_hierarchies, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc")
CAM = synth.make_camera(64, 48)


def test_usage_errors_return_2(tmp_path, capsys):
    assert merge_hierarchies.main([]) == 2
    assert merge_hierarchies.main(["trained", "0", "chunks", "out.hier"]) == 2     # no chunk name
    assert "usage" in capsys.readouterr().err
    for root_type in ("1", "2", "-1", "x"):
        assert merge_hierarchies.main([str(tmp_path), root_type, str(tmp_path), str(tmp_path / "m.hier"), "a"]) == 2
        assert "root type" in capsys.readouterr().err
    # a chunk without hierarchy.hier_opt or hierarchy.hier
    (tmp_path / "trained" / "a").mkdir(parents=True)
    (tmp_path / "trained" / "b").mkdir()
    (tmp_path / "trained" / "a" / "hierarchy.hier").write_bytes(b"")
    assert merge_hierarchies.main([str(tmp_path / "trained"), "0", str(tmp_path), str(tmp_path / "m.hier"), "a",
                                   "b"]) == 2
    err = capsys.readouterr().err
    assert "b" in err and "hier_opt" in err
    assert not (tmp_path / "m.hier").exists()


def test_chunk_file_prefers_hier_opt(tmp_path):
    d = tmp_path / "c"
    d.mkdir()
    assert merge_hierarchies.chunk_file(str(tmp_path), "c") == (None, False)
    (d / "hierarchy.hier").write_bytes(b"x")
    assert merge_hierarchies.chunk_file(str(tmp_path), "c") == (str(d / "hierarchy.hier"), True)
    (d / "hierarchy.hier_opt").write_bytes(b"x")
    assert merge_hierarchies.chunk_file(str(tmp_path), "c") == (str(d / "hierarchy.hier_opt"), False)


def _with_tail(h, tail, seed=0):
    """h with `tail` random rows appended behind its node rows (G = N + tail), as save_hier appends the skybox."""
    if tail == 0:
        return h
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    M = h.shs.shape[1]
    return hierarchy.Hierarchy(torch.cat([h.xyz, r(tail, 3)]), torch.cat([h.shs, r(tail, M, 3)]),
                               torch.cat([h.alpha, r(tail, 1).abs()]), torch.cat([h.log_scales, r(tail, 3)]),
                               torch.cat([h.rots, r(tail, 4)]), h.nodes, h.boxes)


def _layout(path):
    lib = _lib.lib()
    hh = _lib.HierHost()
    _lib.check(lib.hgs_hier_load(str(path).encode(), C.byref(hh)), "hgs_hier_load")
    try:
        return hh.P, hh.N, hh.M, hh.reserved
    finally:
        lib.hgs_hier_free(C.byref(hh))


def _write_upstream_half(path, h):
    """The upstream half layout (P < 0; rot / scale / alpha / sh as IEEE half), which write_hierarchy does not write."""
    G = h.xyz.shape[0]
    f16 = lambda t: t.numpy().astype("<f2").tobytes()
    with open(path, "wb") as f:
        f.write(struct.pack("<i", -G))
        f.write(h.xyz.numpy().astype("<f4").tobytes())
        f.write(f16(h.rots) + f16(h.log_scales) + f16(h.alpha) + f16(h.shs))
        f.write(struct.pack("<i", h.nodes.shape[0]))
        f.write(h.nodes.numpy().astype("<i4").tobytes() + h.boxes.numpy().astype("<f4").tobytes())


@pytest.mark.parametrize("M,tail", [(16, 0), (16, 37), (4, 0), (4, 5), (1, 11)])
def test_header_peek_agrees_with_the_loader(tmp_path, M, tail):
    h = hierarchy.build_hierarchy(synth.make_scene(50, CAM, seed=M + tail))
    h = hierarchy.Hierarchy(h.xyz, h.shs[:, :M].contiguous(), h.alpha, h.log_scales, h.rots, h.nodes, h.boxes)
    h = _with_tail(h, tail, seed=tail)
    path = tmp_path / "c.hier"
    write_hierarchy(str(path), h.xyz, h.shs, h.alpha, h.log_scales, h.rots, h.nodes, h.boxes)
    xyz, shs, _, _, _, nodes, _ = load_hierarchy(str(path))
    G, N, M_, layout = hierarchy.read_hier_header(str(path))
    assert (G, N, M_) == (xyz.shape[0], nodes.shape[0], shs.shape[1]) == (99 + tail, 99, M)
    assert layout == (hierarchy.HIER_UPSTREAM if M == 16 else hierarchy.HIER_PRIVATE) == _layout(path)[3]
    if M == 16:
        half = tmp_path / "half.hier"
        _write_upstream_half(half, h)
        assert hierarchy.read_hier_header(str(half)) == (99 + tail, 99, 16, hierarchy.HIER_UPSTREAM_HALF)
        assert _layout(half) == (99 + tail, 99, 16, hierarchy.HIER_UPSTREAM_HALF)


def test_header_peek_rejects_what_the_loader_rejects(tmp_path):
    h = hierarchy.build_hierarchy(synth.make_scene(20, CAM, seed=1))
    path = tmp_path / "c.hier"
    write_hierarchy(str(path), h.xyz, h.shs, h.alpha, h.log_scales, h.rots, h.nodes, h.boxes)
    data = path.read_bytes()
    for name, blob in (("short", data[:-1]), ("long", data + b"\0"), ("empty", b""), ("tiny", b"\1\0")):
        bad = tmp_path / f"{name}.hier"
        bad.write_bytes(blob)
        with pytest.raises(ValueError, match="neither"):
            hierarchy.read_hier_header(str(bad))
        with pytest.raises(RuntimeError):
            load_hierarchy(str(bad))


def test_merge_layout_is_the_spec_numbering():
    a = hierarchy.build_hierarchy(synth.make_scene(7, CAM, seed=1))
    b = hierarchy.build_hierarchy(synth.make_scene(1, CAM, seed=2))
    c = hierarchy.build_hierarchy(synth.make_scene(5, CAM, seed=3))
    m = hierarchy.merge_hierarchies([a, b, c])
    bases, N = hierarchy.merge_layout([13, 1, 9])
    assert N == m.num_nodes == 1 + 3 + 12 + 0 + 8
    assert bases == [4, 16, 16]
    # chunk a's node 1 lands at bases[0], chunk c's at bases[2]
    assert torch.equal(m.xyz[bases[0]], a.xyz[1]) and torch.equal(m.xyz[bases[2]], c.xyz[1])
    assert torch.equal(m.xyz[2], b.xyz[0])


def _view(G, N, M=16):
    return _lib.HierView(G, N, M, 0, None, None, None, None, None, None, None)


@pytest.mark.parametrize("chunk,k,base,merged,needle", [
    ((1, 0), 1, 2, (2, 2), b"chunk N=0"),
    ((4, -3), 1, 2, (2, 2), b"chunk N=-3"),
    ((4, 5), 1, 2, (6, 6), b"chunk G=4 < N=5"),
    ((5, 5), 1, 2, (1 << 31, 1 << 31), b"merged N=2147483648"),
    ((5, 5), 2, 3, (3 + (1 << 32), 3 + (1 << 32)), b"merged N=4294967299"),
    ((5, 5), 1, 2, (1, 1), b"merged N=1"),
    ((5, 5), 0, 2, (6, 6), b"k=0"),
    ((5, 5), 1, 1, (6, 6), b"base=1"),
    ((5, 5), 1, 3, (6, 6), b"base=3"),
    ((5, 5), 2, 2, (7, 7), b"base=2"),
    ((5, 5), 1, 2, (6, 7), b"merged G=6 != N=7"),
])
def test_place_checks_sizes_before_touching_the_device(chunk, k, base, merged, needle):
    """Returns an error naming the bad size, without a GPU and before any HIP call (every pointer is null here)."""
    lib = _lib.lib()
    rep = _lib.HierMergeReport()
    rc = lib.hgs_hier_merge_place(C.byref(_view(*chunk)), 0, k, base, C.byref(_view(*merged)), None, C.byref(rep),
                                  None, 0)
    assert rc == 1                                                            # HGS_ERR_INVALID
    msg = lib.hgs_last_error()
    assert b"bad sizes" in msg and needle in msg, msg


def test_place_checks_index_and_sh_count():
    lib = _lib.lib()
    rep = _lib.HierMergeReport()
    for index, M, needle in ((2, 16, b"index=2"), (-1, 16, b"index=-1"), (0, 4, b"chunk M=4 != merged M=16")):
        rc = lib.hgs_hier_merge_place(C.byref(_view(5, 5, M)), index, 2, 3, C.byref(_view(11, 11)), None, C.byref(rep),
                                      None, 0)
        assert rc == 1 and needle in lib.hgs_last_error(), lib.hgs_last_error()
    # valid sizes reach the null-pointer check, still without a HIP call
    rc = lib.hgs_hier_merge_place(C.byref(_view(5, 5)), 1, 2, 3, C.byref(_view(11, 11)), None, C.byref(rep), None, 0)
    assert rc == 1 and lib.hgs_last_error() == b"null argument"


@pytest.mark.parametrize("k,merged,needle", [(0, (3, 3), b"k=0"), (3, (3, 3), b"merged N=3"),
                                             (1, (1 << 31, 1 << 31), b"merged N=2147483648"),
                                             (1, (3, 3, 65), b"merged M=65")])
def test_root_checks_sizes_before_touching_the_device(k, merged, needle):
    lib = _lib.lib()
    assert lib.hgs_hier_merge_root(C.byref(_view(*merged)), k, None, 0) == 1
    msg = lib.hgs_last_error()
    assert b"bad sizes" in msg and needle in msg, msg


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("c++filt")),
                    reason="needs hipcc (cross-compiles without a GPU) and c++filt")
def test_merger_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    rows = {r["kernel"]: r for r in kernel_resources.collect([os.path.join(CSRC, "hier_merge.hip")])}
    for k in ("hm_nodes_kernel", "hm_root_kernel"):
        assert k in rows, (k, sorted(rows))
    for k, r in rows.items():
        assert r["scratch"] == 0, f"{k} uses {r['scratch']} bytes of scratch per lane"
