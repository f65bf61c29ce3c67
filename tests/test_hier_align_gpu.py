"""The HIP rotation aligner (hgs.hierarchy.align_hierarchy_gpu, csrc/hier_align.hip) against the numpy spec
hgs.hierarchy.align_hierarchy on GPU-built and GPU-merged hierarchies: the same group element at every node, log_scales
bit for bit, rots within 2 float32 ulp; the spec's properties on the device output itself; a skybox tail; malformed
hierarchies; guard bytes around tmp and the two in-place arrays; renders through the in-op LOD path at weight 1 (equal)
and at the cut's own weights (different); the creator command with and without ``--align``."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity as pa
import ws_guard as wg
from hgs import _lib, create_hierarchy, hierarchy, synth
from test_hier_align_cpu import BOUND, bits, check_properties
from test_hier_merge_gpu import _chunk, _cpu, _ulps, _with_tail

pytestmark = pytest.mark.gpu

CAM = synth.make_camera(256, 160)
SIZES = [1, 2, 3, 257, 2000]
ARRAYS = ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes")


def _clone(h):
    return hierarchy.Hierarchy(*(getattr(h, k).clone() for k in ARRAYS))


def _built(P, gpu, kind=synth.make_scene):
    return hierarchy.build_hierarchy_gpu(kind(P, CAM, seed=3).to(gpu), gpu)


def device_choice(h0, a):
    """The group element behind every row of the device output ``a`` of input ``h0`` (host): the candidate
    +- q (x) g_j nearest to the written quaternion.  -> (j [N], the distance to it in float32 ulp [N])."""
    N = h0.num_nodes
    g, perms = hierarchy.align_group()
    c = hierarchy._quat_mul(h0.rots[:N].double().numpy()[:, None, :], g[None])            # [N,24,4]
    out = a.rots[:N].double().numpy()[:, None, :]
    dist = np.minimum(np.abs(c - out).max(2), np.abs(c + out).max(2))
    j = dist.argmin(1)
    cj = c[np.arange(N), j]
    cj = np.where((np.abs(cj - out[:, 0]).max(1) <= np.abs(cj + out[:, 0]).max(1))[:, None], cj, -cj)
    ulp = _ulps(torch.from_numpy(cj.astype(np.float32)), a.rots[:N]).max(1).values.numpy()
    moved = np.take_along_axis(h0.log_scales[:N].numpy(), perms[j], 1)
    assert np.array_equal(moved.view(np.uint32), a.log_scales[:N].numpy().view(np.uint32)), "scales do not follow the axes"
    return j, ulp


def compare_to_spec(h0, a):
    """a: the device's alignment of h0 (both host); against align_hierarchy(h0)."""
    N = h0.num_nodes
    choice = np.zeros(N, dtype=np.int64)
    spec = hierarchy.align_hierarchy(h0, choice)
    j, ulp = device_choice(h0, a)
    assert int(ulp.max()) <= 2, int(ulp.max())
    assert np.array_equal(j, choice), np.nonzero(j != choice)[0][:8]
    assert torch.equal(bits(a.log_scales), bits(spec.log_scales)), "log_scales must be bit-exact"
    u = int(_ulps(a.rots, spec.rots).max())
    assert u <= 2, f"rots: {u} ulp"
    return spec, choice


def check_device_alignment(h, gpu):
    """h: an unaligned device hierarchy (consumed).  Spec equality, properties 1-5 on the device output, and 6: a second
    device alignment changes no bit.  -> (the input, the device output), both on the host."""
    h0 = _cpu(_clone(h))
    assert hierarchy.align_hierarchy_gpu(h) is h
    a = _cpu(_clone(h))
    compare_to_spec(h0, a)
    check_properties(h0, a)
    hierarchy.align_hierarchy_gpu(h)
    for k in ARRAYS:
        assert torch.equal(bits(getattr(h, k).cpu()), bits(getattr(a, k))), f"a second alignment changed {k}"
    return h0, a


@pytest.mark.parametrize("kind", [synth.make_scene, synth.make_scene_trained_like], ids=["uniform", "trained_like"])
@pytest.mark.parametrize("P", SIZES)
def test_device_alignment_of_builder_output(gpu, P, kind):
    h0, a = check_device_alignment(_built(P, gpu, kind), gpu)
    if P >= 257:       # negative control: the input is far from aligned, so the test above moved most rows
        assert float((hierarchy.alignment_dots(h0) < BOUND).mean()) > 0.5
        changed = (bits(a.rots) != bits(h0.rots)).any(1) | (bits(a.log_scales) != bits(h0.log_scales)).any(1)
        assert int(changed.sum()) > P


def test_the_build_flag(gpu):
    sc = synth.make_scene(257, CAM, seed=3).to(gpu)
    plain, flagged = hierarchy.build_hierarchy_gpu(sc, gpu), hierarchy.build_hierarchy_gpu(sc, gpu, align=True)
    default = hierarchy.build_hierarchy_gpu(sc)
    for k in ARRAYS:
        assert torch.equal(bits(getattr(default, k)), bits(getattr(plain, k))), k
    hierarchy.align_hierarchy_gpu(plain)
    for k in ARRAYS:
        assert torch.equal(bits(getattr(flagged, k)), bits(getattr(plain, k))), k


def test_merged_layout(gpu):
    """Three chunks side by side under a new axis-aligned root: the numbering is not BFS (a level's nodes lie in three
    runs), and the chunk roots align against the identity rotation."""
    chunks = [_chunk(P, seed=3 + i, dev=gpu, shift=(3.0 * i, -2.0 * i)) for i, P in enumerate((5, 64, 257))]
    hm = hierarchy.merge_hierarchies_gpu(chunks, gpu)
    depth = hm.nodes[:, 0].cpu().numpy()
    assert (np.diff(depth) < 0).any(), "the merged numbering is expected not to be level by level"
    assert hm.rots[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    stats = {}
    flagged = hierarchy.merge_hierarchies_gpu(chunks, gpu, stats, align=True)
    assert stats["align_ms"] > 0.0 and stats["merge_ms"] > 0.0
    h0, a = check_device_alignment(hm, gpu)
    for k in ARRAYS:
        assert torch.equal(bits(getattr(flagged, k).cpu()), bits(getattr(a, k))), k
    plain = hierarchy.merge_hierarchies_gpu(chunks, gpu, align=False)
    for k in ARRAYS:
        assert torch.equal(bits(getattr(plain, k).cpu()), bits(getattr(h0, k))), k


def test_a_skybox_tail_is_not_touched(gpu):
    h = _with_tail(_built(257, gpu), 7, seed=7)
    assert h.xyz.shape[0] == h.num_nodes + 7
    h0, a = check_device_alignment(h, gpu)
    N = h0.num_nodes
    for k in ("xyz", "shs", "alpha", "log_scales", "rots"):
        assert torch.equal(bits(getattr(a, k)[N:]), bits(getattr(h0, k)[N:])), k
    # the same rows as without the tail
    plain = _cpu(hierarchy.align_hierarchy_gpu(_built(257, gpu)))
    assert torch.equal(bits(a.rots[:N]), bits(plain.rots)) and torch.equal(bits(a.log_scales[:N]), bits(plain.log_scales))


def _corrupt(kind, nodes):
    """-> (the check that must fail, its first offending node); ``nodes`` [N,7] (device) is modified in place."""
    N = nodes.shape[0]
    leaf = N - 1                                   # the last node of a BFS numbering has no children
    if kind == "depth_off_by_one":
        nodes[leaf, 0] += 1
        return 2, leaf
    if kind == "depth_too_large":
        nodes[leaf, 0] = 256
        return 0, leaf
    if kind == "negative_depth":
        nodes[300, 0] = -3
        return 0, 300
    if kind == "parent_out_of_range":
        nodes[77, 1] = N
        return 1, 77
    if kind == "negative_parent":
        nodes[77, 1] = -1
        return 1, 77
    if kind == "second_root":
        nodes[leaf, 0] = 0
        return 3, leaf
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["depth_off_by_one", "depth_too_large", "negative_depth", "parent_out_of_range",
                                  "negative_parent", "second_root"])
def test_a_malformed_hierarchy_is_reported_and_left_untouched(gpu, kind):
    h = _built(257, gpu)
    assert int(h.nodes[-1, 6]) == 0
    check, node = _corrupt(kind, h.nodes)
    before = _cpu(_clone(h))
    with pytest.raises(hierarchy.HierarchyAlignError) as e:
        hierarchy.align_hierarchy_gpu(h)
    assert e.value.node == node and e.value.check == hierarchy.ALIGN_CHECKS[check], (e.value.check, e.value.node)
    assert f"node {node}" in str(e.value)
    for k in ARRAYS:
        assert torch.equal(bits(getattr(h, k).cpu()), bits(getattr(before, k))), f"{k} was modified"


def test_an_interior_depth_error_names_the_first_offender(gpu):
    """A wrong depth at an interior node also puts its children one level off: the smallest index is the one named."""
    h = _built(257, gpu)
    i = 5
    kids = int(h.nodes[i, 5])
    assert int(h.nodes[i, 6]) == 2 and kids > i
    h.nodes[i, 0] += 1
    before = _cpu(_clone(h))
    rep = _lib.HierAlignReport()
    tmp = torch.empty(_lib.lib().hgs_hier_align_tmp_bytes(h.num_nodes), dtype=torch.uint8, device=gpu)
    rc = _lib.lib().hgs_hier_align(h.nodes.data_ptr(), h.num_nodes, h.log_scales.data_ptr(), h.rots.data_ptr(),
                                   tmp.data_ptr(), C.byref(rep), C.c_void_p(torch.cuda.current_stream().cuda_stream),
                                   gpu.index or 0)
    assert rc == 1 and list(rep.first_bad) == [-1, -1, i, -1] and rep.roots == 1
    assert b"first offending node 5" in _lib.lib().hgs_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(h.rots.cpu()), bits(before.rots)) and torch.equal(bits(h.log_scales.cpu()), bits(before.log_scales))


@pytest.mark.parametrize("P", [1, 2, 3, 257, 2000])          # N = 1, 3, 5, 513, 3999: off the 64-lane wave grid
def test_the_call_stays_in_bounds(gpu, P):
    """tmp, log_scales and rots each in an allocation of its own between guards (tests/ws_guard.py); tmp filled with 0x00
    and with 0xFF: intact guards, results that do not depend on what tmp held, and the spec's result."""
    lib = _lib.lib()
    h = _cpu(_built(P, gpu))
    N = h.num_nodes
    assert N == 2 * P - 1

    def run(fill):
        gs = []

        def put(name, t):
            g = wg.guarded(t.numel() * t.element_size(), gpu, 0x00, name)
            g.body.copy_(t.contiguous().reshape(-1).view(torch.uint8).to(gpu))
            gs.append(g)
            return g

        nodes, ls, rots = put("nodes", h.nodes), put("log_scales", h.log_scales), put("rots", h.rots)
        tmp = wg.guarded(lib.hgs_hier_align_tmp_bytes(N), gpu, fill, "tmp")
        gs.append(tmp)
        rep = _lib.HierAlignReport()
        _lib.check(lib.hgs_hier_align(nodes.addr, N, ls.addr, rots.addr, tmp.addr, C.byref(rep),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream), gpu.index or 0), "hgs_hier_align")
        wg.check(*gs)
        assert list(rep.first_bad) == [-1] * 4 and rep.roots == 1
        assert rep.levels == int(h.nodes[:, 0].max()) + 1
        assert torch.equal(nodes.view(torch.int32, N, 7).cpu(), h.nodes), "nodes were modified"
        return ls.view(torch.float32, N, 3).cpu().clone(), rots.view(torch.float32, N, 4).cpu().clone()

    (ls0, r0), (ls1, r1) = run(0x00), run(0xFF)
    assert torch.equal(bits(ls0), bits(ls1)) and torch.equal(bits(r0), bits(r1)), "the result depends on tmp's contents"
    compare_to_spec(h, hierarchy.Hierarchy(h.xyz, h.shs, h.alpha, ls0, r0, h.nodes, h.boxes))


def _cut(h, k, gpu):
    """The LOD cut of ``h`` (device) at granularity k pixels from CAM: (n, ri, pi, weights, num_siblings)."""
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    G = h.num_nodes
    ri = torch.zeros(G, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(G, device=gpu); ns = torch.zeros(G, dtype=torch.int32, device=gpu)
    tau = 2 * k * CAM.tanfovx / (0.5 * CAM.image_width)
    n = expand_to_size(h.nodes, h.boxes, tau, CAM.camera_center.to(gpu), torch.zeros(3), ri, pi, ni)
    get_interpolation_weights(ni[:n], tau, h.nodes, h.boxes, CAM.camera_center.cpu(), torch.zeros(3), w, ns)
    return n, ri, pi, w, ns


def _render(h, cut, w, gpu):
    import diff_gaussian_rasterization as dgr
    n, ri, pi, _, ns = cut
    G = h.num_nodes
    kw = pa.settings_kwargs(CAM, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=w, num_node_kids=ns)
    kw["render_indices"], kw["parent_indices"] = ri[:n].contiguous(), pi
    r = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw))
    with torch.no_grad():
        color, _, _ = r(means3D=h.xyz, means2D=torch.zeros(G, 3, device=gpu), shs=h.shs, opacities=h.alpha.abs(),
                        scales=torch.exp(h.log_scales), rotations=torch.nn.functional.normalize(h.rots))
    return color.cpu()


def test_renders_through_the_in_op_lod_path(gpu):
    """Aligning re-parametrises Gaussians without changing them: a cut rendered with every interpolation weight forced
    to 1 is the same image (within 1e-5 of its maximum, the tolerance of test_hier_build_gpu for re-parametrised
    nodes).  At the cut's own weights, most of them strictly between 0 and 1, the interpolated ellipsoids differ and
    so do the images: the comparison above does run the interpolation."""
    plain = _built(257, gpu)
    aligned = hierarchy.align_hierarchy_gpu(_clone(plain))
    cut = _cut(plain, 16.0, gpu)                   # nodes and boxes are the same in both
    n, w = cut[0], cut[3]
    assert 64 < n < plain.num_nodes
    blending = float(((w[:n] > 0) & (w[:n] < 1)).float().mean())
    assert blending >= 0.25, blending
    ones = torch.ones_like(w)
    a1, b1 = _render(aligned, cut, ones, gpu), _render(plain, cut, ones, gpu)
    assert float(b1.max()) > 0.05
    st = pa.err_stats(a1, b1)
    assert st["maxrel"] <= 1e-5 and st["l2"] <= 1e-5, st
    aw, bw = _render(aligned, cut, w, gpu), _render(plain, cut, w, gpu)
    diff = float((aw - bw).abs().max()) / float(bw.abs().max())
    assert diff > 1e-5, diff


def test_create_hierarchy_command_with_and_without_the_flag(gpu, tmp_path):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from hgs import ply
    from hier_build_common import save_ply_layout
    ply_path = str(tmp_path / "point_cloud.ply")
    save_ply_layout(ply_path, 600, 16, seed=8)
    chunk = tmp_path / "chunk"
    chunk.mkdir()
    # today's output, restated: the GPU build of the rows, written as it is
    h = hierarchy.build_hierarchy_gpu(ply.read_ply(ply_path).to(gpu), gpu)
    ref = str(tmp_path / "ref.hier")
    write_hierarchy(ref, *(getattr(h, k) for k in ARRAYS))
    assert create_hierarchy.main([ply_path, str(chunk), str(tmp_path / "plain")]) == 0
    assert (tmp_path / "plain" / "hierarchy.hier").read_bytes() == open(ref, "rb").read()
    for i, argv in enumerate((["--align", ply_path, str(chunk), str(tmp_path / "a0")],
                              [ply_path, str(chunk), "--align", str(tmp_path / "a1")])):
        assert create_hierarchy.main(argv) == 0
        got = hierarchy.Hierarchy(*load_hierarchy(str(tmp_path / f"a{i}" / "hierarchy.hier")))
        want = _cpu(hierarchy.align_hierarchy_gpu(_clone(h)))
        ref_a = str(tmp_path / f"ref_a{i}.hier")
        write_hierarchy(ref_a, *(getattr(want, k) for k in ARRAYS))
        want = hierarchy.Hierarchy(*load_hierarchy(ref_a))
        for k in ARRAYS:
            assert torch.equal(bits(getattr(got, k)), bits(getattr(want, k))), k
        assert float((hierarchy.alignment_dots(got) < BOUND).mean()) == 0.0
    assert (tmp_path / "a0" / "hierarchy.hier").read_bytes() != open(ref, "rb").read()


def test_align_hierarchy_command(gpu, tmp_path, capsys):
    """python -m hgs.align_hierarchy <in> <out>, in-process: a file with a skybox tail behind its node rows."""
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from hgs import align_hierarchy as cmd
    h = _cpu(_with_tail(_built(257, gpu), 7, seed=2))
    src, dst = str(tmp_path / "hierarchy.hier_opt"), str(tmp_path / "out" / "aligned.hier")
    write_hierarchy(src, *(getattr(h, k) for k in ARRAYS))
    assert cmd.main([src, dst]) == 0
    line = capsys.readouterr().out
    assert "N = 513 nodes" in line and "7 rows behind them" in line and "-> 0.0 %" in line and " ms" in line
    h0, got = hierarchy.Hierarchy(*load_hierarchy(src)), hierarchy.Hierarchy(*load_hierarchy(dst))
    assert got.xyz.shape[0] == 520
    check_properties(h0, got)
    compare_to_spec(h0, got)
