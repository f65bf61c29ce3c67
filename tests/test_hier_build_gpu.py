"""The HIP hierarchy builder (hgs.hierarchy.build_hierarchy_gpu, csrc/hier_build.hip) against the numpy spec
hgs.hierarchy.build_hierarchy on the same scenes: nodes, boxes and leaf rows bit-exact, interior rows to rounding
(covariances compared, not quaternions: eigenvectors are sign- and order-ambiguous); the LOD cut and a render on top of
it; a 10 M-leaf property check with the build time; and the creator command end to end."""
import numpy as np
import pytest
import torch

import parity as pa
from hgs import hierarchy, synth

pytestmark = pytest.mark.gpu

CAM = synth.make_camera(256, 160)


def _scene(kind, P, seed=0, sh_degree=3):
    if kind == "uniform":
        return synth.make_scene(P, CAM, seed=seed, sh_degree=sh_degree)
    if kind == "trained_like":
        return synth.make_scene_trained_like(P, CAM, seed=seed, sh_degree=sh_degree)
    sc = synth.make_scene(P, CAM, seed=seed, sh_degree=sh_degree)
    g = torch.Generator().manual_seed(seed + 1)
    if kind == "duplicates":          # many rows on few distinct positions: long runs of equal Morton codes
        xyz = sc.means3D[torch.randint(0, max(P // 50, 1), (P,), generator=g)].contiguous()
    elif kind == "coincident":        # every row at one point: hi == lo
        xyz = sc.means3D[:1].repeat(P, 1).contiguous()
    elif kind == "needles":           # two axes 1e-4 of the third
        s = sc.scales.clone()
        s[:, 1:] *= 1e-4
        return synth.Scene(sc.means3D, s.contiguous(), sc.rotations, sc.opacities, sc.shs, sh_degree)
    else:
        raise ValueError(kind)
    return synth.Scene(xyz, sc.scales, sc.rotations, sc.opacities, sc.shs, sh_degree)


def _cov(log_scales, rots):
    """[N,3,3] float64 covariance R(q) diag(exp(2 log_scales)) R(q)^T."""
    q = rots.double().numpy()
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    R = hierarchy._rot_from_quat(q)
    L = R * np.exp(log_scales.double().numpy())[:, None, :]
    return L @ L.transpose(0, 2, 1)


def _bits(t):
    return t.contiguous().view(torch.int32)


def compare_to_spec(hg, hr):
    """hg: GPU build (any device), hr: build_hierarchy (CPU)."""
    hg = hierarchy.Hierarchy(*(t.cpu() for t in (hg.xyz, hg.shs, hg.alpha, hg.log_scales, hg.rots, hg.nodes, hg.boxes)))
    assert torch.equal(hg.nodes, hr.nodes)
    assert torch.equal(_bits(hg.boxes), _bits(hr.boxes)), "boxes must be bit-exact"
    leaf = hr.nodes[:, 3] == 1
    for k in ("xyz", "shs", "alpha", "rots"):
        assert torch.equal(_bits(getattr(hg, k)[leaf]), _bits(getattr(hr, k)[leaf])), f"leaf {k} must be bit-exact"
    ulps = (_bits(hg.log_scales[leaf]).long() - _bits(hr.log_scales[leaf]).long()).abs()
    assert int(ulps.max()) <= 1, int(ulps.max())
    inner = ~leaf
    if not bool(inner.any()):
        return
    pa.assert_stats("interior", {k: pa.err_stats(getattr(hg, k)[inner], getattr(hr, k)[inner])
                                 for k in ("xyz", "shs", "alpha")})
    norms = hg.rots[inner].double().norm(dim=1)
    assert float((norms - 1).abs().max()) <= 1e-6
    cg, cr = _cov(hg.log_scales[inner], hg.rots[inner]), _cov(hr.log_scales[inner], hr.rots[inner])
    rel = np.linalg.norm(cg - cr, axis=(1, 2)) / np.linalg.norm(cr, axis=(1, 2))
    assert float(rel.max()) <= 1e-5, (float(rel.max()), int(rel.argmax()))


CASES = [("uniform", P, 3) for P in (1, 2, 3, 5, 64, 65, 1000, 4097, 100_003, 300_000)] + \
        [("trained_like", P, 3) for P in (65, 4097, 100_003)] + \
        [("uniform", P, 0) for P in (1, 5, 1000, 4097)] + [("trained_like", 4097, 0)] + \
        [("duplicates", 20_000, 3), ("duplicates", 999, 0), ("coincident", 1000, 3), ("coincident", 2, 0),
         ("needles", 4097, 3)]


@pytest.mark.parametrize("kind,P,deg", CASES)
def test_gpu_build_matches_the_numpy_spec(gpu, kind, P, deg):
    sc = _scene(kind, P, seed=P % 97, sh_degree=deg)
    hg = hierarchy.build_hierarchy_gpu(sc.to(gpu))
    assert hg.nodes.device == hg.xyz.device == gpu
    assert hg.shs.shape == (2 * P - 1, 16, 3) and hg.alpha.shape == (2 * P - 1, 1)
    compare_to_spec(hg, hierarchy.build_hierarchy(sc))


def test_sh_degree_2_input(gpu):
    sc = _scene("uniform", 777, seed=4, sh_degree=2)
    compare_to_spec(hierarchy.build_hierarchy_gpu(sc), hierarchy.build_hierarchy(sc))


def _canonical(h):
    """The numpy build's interior (log_scales, rots) re-expressed in the builder's parametrisation of the same
    covariance (ascending eigenvalues, each axis' largest component positive, proper rotation): the LOD blend
    interpolates scales and rotations separately, so two renders compare only in one parametrisation."""
    inner = (h.nodes[:, 3] == 0).numpy()
    q = h.rots.double().numpy()[inner]
    R = hierarchy._rot_from_quat(q / np.linalg.norm(q, axis=1, keepdims=True))
    ls = h.log_scales.double().numpy()[inner]
    order = np.argsort(ls, axis=1, kind="stable")
    ls = np.take_along_axis(ls, order, 1)
    R = np.take_along_axis(R, order[:, None, :], 2)
    lead = np.take_along_axis(R, np.abs(R).argmax(axis=1)[:, None, :], 1)[:, 0, :]
    R = R * np.where(lead < 0, -1.0, 1.0)[:, None, :]
    R[np.linalg.det(R) < 0, :, 0] *= -1
    rots, log_scales = h.rots.clone(), h.log_scales.clone()
    rots[torch.from_numpy(inner)] = torch.from_numpy(hierarchy._quat_from_rot(R)).float()
    log_scales[torch.from_numpy(inner)] = torch.from_numpy(ls).float()
    return hierarchy.Hierarchy(h.xyz, h.shs, h.alpha, log_scales, rots, h.nodes, h.boxes)


@pytest.mark.parametrize("P", [1000, 50_000])
def test_lod_cut_on_the_gpu_build_equals_the_cut_on_the_spec(gpu, P):
    from gaussian_hierarchy import _C as gh
    sc = synth.make_scene(P, CAM, seed=2)
    hr, hg = hierarchy.build_hierarchy(sc), hierarchy.build_hierarchy_gpu(sc.to(gpu))
    nr, br = hr.nodes.to(gpu), hr.boxes.to(gpu)
    assert gh._boxes_nested(hg.nodes, hg.boxes)
    G = hg.num_nodes
    out = {k: [torch.zeros(G, dtype=torch.int32, device=gpu) for _ in range(3)] for k in ("r", "g")}
    w = {k: torch.zeros(G, device=gpu) for k in ("r", "g")}
    ns = {k: torch.zeros(G, dtype=torch.int32, device=gpu) for k in ("r", "g")}
    for vp in (torch.tensor([0.0, 0.0, 0.0]), torch.tensor([0.3, -0.1, 5.0]), torch.tensor([1.0, 2.0, -4.0])):
        for tau in (0.0, 0.002, 0.01, 0.06, 0.5, 1e4):
            n = {}
            for k, (nodes, boxes) in (("r", (nr, br)), ("g", (hg.nodes, hg.boxes))):
                n[k] = gh.expand_to_size(nodes, boxes, tau, vp.to(gpu), torch.zeros(3), *out[k])
                gh.get_interpolation_weights(out[k][2][:n[k]], tau, nodes, boxes, vp, torch.zeros(3), w[k], ns[k])
            assert n["r"] == n["g"]
            for a, b in zip(out["r"], out["g"]):
                assert torch.equal(a[:n["r"]], b[:n["r"]])
            assert torch.equal(_bits(w["r"][:n["r"]]), _bits(w["g"][:n["r"]]))
            assert torch.equal(ns["r"][:n["r"]], ns["g"][:n["r"]])


def test_in_op_lod_render_of_the_gpu_build_matches_the_spec(gpu):
    """One frame through the rasterizer's in-op LOD interpolation (as test_lod_gpu.py's in-op case): the GPU-built
    hierarchy against the numpy-built one."""
    import diff_gaussian_rasterization as dgr
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    sc = synth.make_scene(4000, CAM, seed=9)
    hr = _canonical(hierarchy.build_hierarchy(sc))
    hg = hierarchy.build_hierarchy_gpu(sc.to(gpu))
    nodes, boxes = hg.nodes, hg.boxes
    G = hg.num_nodes
    ri = torch.zeros(G, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(G, device=gpu); ns = torch.zeros(G, dtype=torch.int32, device=gpu)
    tau = (2 * (4 + 0.5)) * CAM.tanfovx / (0.5 * CAM.image_width)
    n = expand_to_size(nodes, boxes, tau, CAM.camera_center.to(gpu), torch.zeros(3), ri, pi, ni)
    assert 0 < n < G
    get_interpolation_weights(ni[:n], tau, nodes, boxes, CAM.camera_center.cpu(), torch.zeros(3), w, ns)
    assert bool(((w[:n] > 0) & (w[:n] < 1)).any()), "the cut must blend for the comparison to mean anything"

    def render(h):
        kw = pa.settings_kwargs(CAM, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=w,
                                num_node_kids=ns)
        kw["render_indices"], kw["parent_indices"] = ri[:n].contiguous(), pi
        r = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw))
        with torch.no_grad():
            color, radii, _ = r(means3D=h.xyz.to(gpu), means2D=torch.zeros(G, 3, device=gpu), shs=h.shs.to(gpu),
                                opacities=h.alpha.to(gpu).abs(), scales=torch.exp(h.log_scales.to(gpu)),
                                rotations=torch.nn.functional.normalize(h.rots.to(gpu)))
        return color.cpu(), radii.cpu()

    cg, rg = render(hg)
    cr, rr = render(hr)
    assert float(cr.max()) > 0.05
    st = pa.err_stats(cg, cr)
    assert st["maxrel"] <= 1e-5 and st["l2"] <= 1e-5, st


def test_ten_million_leaves_properties_and_time(gpu):
    P = 10_000_000
    sc = synth.make_scene(P, CAM, seed=11).to(gpu)
    hierarchy.build_hierarchy_gpu(sc)                                   # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    h = hierarchy.build_hierarchy_gpu(sc)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    print(f"build of {P} leaves: {ms:.2f} ms")
    assert ms <= 100.0, ms
    N = 2 * P - 1
    nd = h.nodes.long()
    assert nd.shape == (N, 7)
    ids = torch.arange(N, device=gpu)
    assert torch.equal(nd[:, 2], ids)
    leaf = nd[:, 6] == 0
    assert int(leaf.sum()) == P
    assert torch.equal(nd[:, 3], leaf.long()) and torch.equal(nd[:, 4], (~leaf).long())
    assert bool((nd[leaf, 5] == 0).all()) and bool((nd[~leaf, 6] == 2).all())
    inner = ids[~leaf]
    c0 = nd[inner, 5]
    for c in (c0, c0 + 1):
        assert torch.equal(nd[c, 1], inner) and torch.equal(nd[c, 0], nd[inner, 0] + 1)
    assert int(nd[0, 1]) == -1 and int(nd[0, 0]) == 0
    kids = torch.zeros(N, dtype=torch.int32, device=gpu)
    kids[c0] += 1
    kids[c0 + 1] += 1
    assert int(kids[0]) == 0 and bool((kids[1:] == 1).all()), "every node but the root is exactly one node's child"
    # leaf positions: the input multiset
    def rows_sorted(t):
        a = t.cpu().numpy().view(np.int32)
        return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
    a, b = rows_sorted(h.xyz[leaf]), rows_sorted(sc.means3D)
    assert np.array_equal(a, b)
    al = h.alpha[~leaf]
    assert bool(((al >= 0) & (al <= 1)).all())
    # the root against the w-weighted float64 moments of every input row (associative: independent of the topology)
    s = sc.scales.double()
    op = sc.opacities.double().reshape(-1)
    w = op * s.prod(1)
    W = w.sum()
    x = sc.means3D.double()
    mu = (w[:, None] * x).sum(0) / W
    q = sc.rotations.double()
    r, qx, qy, qz = q.unbind(1)
    R = torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r * qz), 2 * (qx * qz + r * qy),
                     2 * (qx * qy + r * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r * qx),
                     2 * (qx * qz - r * qy), 2 * (qy * qz + r * qx), 1 - 2 * (qx * qx + qy * qy)], 1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    d = x - mu
    cov = ((w[:, None, None] * (L @ L.transpose(1, 2))).sum(0) + (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(0)) / W
    del L, R
    sh = (w[:, None, None] * sc.shs.double()).sum(0) / W
    alpha = (w * op).sum() / W
    root_xyz = h.xyz[0].double()
    assert float((root_xyz - mu).abs().max()) <= 1e-5 * float(x.abs().max()), (root_xyz, mu)
    croot = torch.from_numpy(_cov(h.log_scales[:1].cpu(), h.rots[:1].cpu())[0])
    assert float((croot - cov.cpu()).norm() / cov.norm()) <= 1e-5
    assert float((h.shs[0].double() - sh).abs().max()) <= 1e-5 * float(sc.shs.abs().max())
    assert abs(float(h.alpha[0, 0]) - float(alpha)) <= 1e-5


def test_create_hierarchy_command(gpu, tmp_path):
    """python -m hgs.create_hierarchy <ply> <chunk dir> <out dir> <scaffold dir>, in-process: 100 skybox rows first
    (pc_info.txt beside the PLY), a chunk dir with center.txt / extent.txt; the .hier it writes against
    write_hierarchy(build_hierarchy(selected rows)), and the shapes train_post.py's create_from_hier relies on."""
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from hgs import create_hierarchy, ply
    from hier_build_common import save_ply_layout
    P, sky = 20_000, 100
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-3.0, 3.0, (P, 3)).astype(np.float32)
    xyz[:sky] = rng.uniform(40.0, 60.0, (sky, 3))
    model = tmp_path / "model" / "point_cloud" / "iteration_30000"
    model.mkdir(parents=True)
    ply_path = str(model / "point_cloud.ply")
    save_ply_layout(ply_path, P, 16, seed=6, xyz=xyz)
    (model / "pc_info.txt").write_text(str(sky))
    chunk = tmp_path / "chunk"
    chunk.mkdir()
    (chunk / "center.txt").write_text("0.25 -0.5 0.0")
    (chunk / "extent.txt").write_text("4.0 4.0 10.0")
    scaffold = tmp_path / "scaffold"
    scaffold.mkdir()
    out_dir = tmp_path / "trained_chunk"
    assert create_hierarchy.main([ply_path, str(chunk), str(out_dir), str(scaffold)]) == 0
    got = load_hierarchy(str(out_dir / "hierarchy.hier"))
    # the expected selection, restated
    full = ply.read_ply(ply_path)
    d = np.abs(xyz - np.float32([0.25, -0.5, 0.0]))
    keep = np.nonzero((np.maximum(d[:, 0], d[:, 1]) <= np.float32(2.0)) & (np.arange(P) >= sky))[0]
    assert 0.2 * P < keep.size < 0.8 * P
    sel = create_hierarchy.subset(full, torch.from_numpy(keep))
    ref_path = str(tmp_path / "ref.hier")
    hr = hierarchy.build_hierarchy(sel)
    write_hierarchy(ref_path, hr.xyz, hr.shs, hr.alpha, hr.log_scales, hr.rots, hr.nodes, hr.boxes)
    want = load_hierarchy(ref_path)
    N = 2 * keep.size - 1
    xyz_g, shs_g, alpha_g, ls_g, rots_g, nodes_g, boxes_g = got
    # create_from_hier (scene/gaussian_model.py:326-399) takes one Gaussian per node and splits shs into dc / rest
    assert xyz_g.shape == (N, 3) and shs_g.shape == (N, 16, 3) and alpha_g.shape == (N, 1)
    assert ls_g.shape == (N, 3) and rots_g.shape == (N, 4) and nodes_g.shape == (N, 7) and boxes_g.shape == (N, 2, 4)
    compare_to_spec(hierarchy.Hierarchy(*got), hierarchy.Hierarchy(*want))
