"""The HIP hierarchy merger (hgs.hierarchy.merge_hierarchies_gpu, csrc/hier_merge.hip) against the torch spec
hgs.hierarchy.merge_hierarchies on chunks trimmed to their first N rows: nodes, boxes and every non-root row bit for bit,
the root row within 2 float32 ulp; skybox tails; corrupt chunks; the consolidation command end to end (in-process);
the LOD cut and a render on the merged hierarchy; device memory against the spec's; a ~30 M-node structure check."""
import numpy as np
import pytest
import torch

import parity as pa
from hgs import hierarchy, merge_hierarchies, synth

pytestmark = pytest.mark.gpu

CAM = synth.make_camera(256, 160)


def _chunk(P, seed, dev, shift=(0.0, 0.0)):
    sc = synth.make_scene(P, CAM, seed=seed)
    xyz = sc.means3D + torch.tensor([shift[0], shift[1], 0.0])
    sc = synth.Scene(xyz.contiguous(), sc.scales, sc.rotations, sc.opacities, sc.shs, sc.sh_degree)
    return hierarchy.build_hierarchy_gpu(sc.to(dev), dev)


def _cpu(h):
    return hierarchy.Hierarchy(*(t.cpu() for t in (h.xyz, h.shs, h.alpha, h.log_scales, h.rots, h.nodes, h.boxes)))


def _trim(h):
    N = h.num_nodes
    return hierarchy.Hierarchy(h.xyz[:N], h.shs[:N], h.alpha[:N], h.log_scales[:N], h.rots[:N], h.nodes, h.boxes)


def _with_tail(h, tail, seed):
    """h with `tail` random rows appended behind its node rows (G = N + tail), as save_hier appends the skybox."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(h.xyz.device)
    M = h.shs.shape[1]
    return hierarchy.Hierarchy(torch.cat([h.xyz, 50 + r(tail, 3)]), torch.cat([h.shs, r(tail, M, 3)]),
                               torch.cat([h.alpha, r(tail, 1).abs()]), torch.cat([h.log_scales, r(tail, 3)]),
                               torch.cat([h.rots, r(tail, 4)]), h.nodes, h.boxes)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ulps(a, b):
    """float32 ulp distance, sign-aware."""
    o = lambda t: (lambda i: torch.where(i < 0, -(i & 0x7FFFFFFF), i))(_bits(t).long())
    return (o(a) - o(b)).abs()


def compare_to_spec(hg, hs):
    """hg: merge_hierarchies_gpu (any device), hs: merge_hierarchies on the trimmed chunks."""
    hg, hs = _cpu(hg), _cpu(hs)
    assert torch.equal(hg.nodes, hs.nodes)
    assert torch.equal(_bits(hg.boxes), _bits(hs.boxes)), "boxes must be bit-exact"
    for k in ("xyz", "shs", "alpha", "log_scales", "rots"):
        a, b = getattr(hg, k), getattr(hs, k)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert torch.equal(_bits(a[1:]), _bits(b[1:])), f"non-root {k} must be bit-exact"
        u = int(_ulps(a[:1], b[:1]).max())
        assert u <= 2, f"root {k}: {u} ulp"


@pytest.mark.parametrize("Ps", [[300], [1, 1000], [1, 37, 4097, 2, 100_003]])
@pytest.mark.parametrize("where", ["device", "host", "path"])
def test_gpu_merge_matches_the_spec(gpu, tmp_path, Ps, where):
    from gaussian_hierarchy._C import write_hierarchy
    chunks = [_chunk(P, seed=i + P % 13, dev=gpu, shift=(3.0 * i, -2.0 * i)) for i, P in enumerate(Ps)]
    if where == "host":
        sources = [_cpu(c) for c in chunks]
    elif where == "path":
        sources = []
        for i, c in enumerate(chunks):
            p = str(tmp_path / f"c{i}.hier")
            write_hierarchy(p, c.xyz, c.shs, c.alpha, c.log_scales, c.rots, c.nodes, c.boxes)
            sources.append(p)
    else:
        sources = chunks
    hg = hierarchy.merge_hierarchies_gpu(sources, gpu)
    assert hg.nodes.device == hg.xyz.device == gpu
    N = 1 + len(Ps) + sum(2 * P - 2 for P in Ps)
    assert hg.num_nodes == N and hg.xyz.shape == (N, 3) and hg.shs.shape == (N, 16, 3) and hg.alpha.shape == (N, 1)
    compare_to_spec(hg, hierarchy.merge_hierarchies([_cpu(c) for c in chunks]))


def test_sh_degree_1_chunks_keep_their_coefficient_count(gpu):
    """Chunks of 4 SH coefficients (the private layout's case) merge to [N, 4, 3] rows."""
    chunks = [_chunk(P, seed=P, dev=gpu) for P in (50, 70)]
    chunks = [hierarchy.Hierarchy(c.xyz, c.shs[:, :4].contiguous(), c.alpha, c.log_scales, c.rots, c.nodes, c.boxes)
              for c in chunks]
    hg = hierarchy.merge_hierarchies_gpu(chunks)
    assert hg.shs.shape == (hg.num_nodes, 4, 3)
    compare_to_spec(hg, hierarchy.merge_hierarchies([_cpu(c) for c in chunks]))


@pytest.mark.parametrize("where", ["device", "host", "path"])
def test_skybox_tails_are_dropped(gpu, tmp_path, where):
    from gaussian_hierarchy._C import write_hierarchy
    chunks = [_chunk(P, seed=P, dev=gpu, shift=(4.0 * i, 0.0)) for i, P in enumerate((1, 513, 2000))]
    tailed = [_with_tail(c, t, seed=t) for c, t in zip(chunks, (7, 1000, 1))]
    assert all(t.xyz.shape[0] > t.num_nodes for t in tailed)
    if where == "host":
        tailed = [_cpu(t) for t in tailed]
    elif where == "path":
        paths = []
        for i, t in enumerate(tailed):
            p = str(tmp_path / f"c{i}.hier_opt")
            write_hierarchy(p, t.xyz, t.shs, t.alpha, t.log_scales, t.rots, t.nodes, t.boxes)
            paths.append(p)
        tailed = paths
    got = _cpu(hierarchy.merge_hierarchies_gpu(tailed, gpu))
    want = _cpu(hierarchy.merge_hierarchies_gpu(chunks, gpu))
    for k in ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes"):
        assert torch.equal(_bits(getattr(got, k)), _bits(getattr(want, k))), k
    compare_to_spec(got, hierarchy.merge_hierarchies([_cpu(_trim(c)) for c in chunks]))


def _corrupt(kind, h):
    """-> (chunk with one defect, check name fragment, first offending node)."""
    h = _cpu(h)
    nodes = h.nodes.clone()
    N = nodes.shape[0]
    if kind == "start":
        nodes[5, 2] = 6
        node, check = 5, "start"
    elif kind == "leaf_merged":
        i = int((nodes[:, 6] == 0).nonzero()[3])
        nodes[i, 4] = 1
        node, check = i, "start"
    elif kind == "unclaimed_child":                      # node 9's parent is the root, whose children are 1 and 2
        nodes[9, 1] = 0
        node, check = 9, "claiming"
    elif kind == "parent_out_of_range":
        nodes[11, 1] = N
        node, check = 11, "claiming"
    elif kind == "root_parent":
        nodes[0, 1] = 3
        node, check = 0, "claiming"
    elif kind == "children_past_N":
        i = int((nodes[:, 6] > 0).nonzero()[-1])         # the last interior node
        nodes[i, 5] = N - 1
        node, check = i, "children range"
    elif kind == "children_count_sum":                   # two ranges claim node 2: the sum is N
        nodes[1, 5], nodes[1, 6] = 2, int(nodes[1, 6]) + 1
        node, check = None, "sum to N - 1"
    else:
        raise ValueError(kind)
    return hierarchy.Hierarchy(h.xyz, h.shs, h.alpha, h.log_scales, h.rots, nodes, h.boxes), check, node


@pytest.mark.parametrize("kind", ["start", "leaf_merged", "unclaimed_child", "parent_out_of_range", "root_parent",
                                  "children_past_N", "children_count_sum"])
def test_corrupt_chunks_raise_a_named_error(gpu, tmp_path, kind):
    from gaussian_hierarchy._C import write_hierarchy
    good = _chunk(100, seed=3, dev=gpu)
    bad, check, node = _corrupt(kind, _chunk(64, seed=4, dev=gpu))
    with pytest.raises(hierarchy.ChunkValidationError, match="chunk 1") as ei:
        hierarchy.merge_hierarchies_gpu([good, bad, good])
    assert check in ei.value.check and ei.value.node == node and ei.value.chunk == "chunk 1", (ei.value.check,
                                                                                             ei.value.node)
    p = str(tmp_path / "bad.hier")
    write_hierarchy(p, bad.xyz, bad.shs, bad.alpha, bad.log_scales, bad.rots, bad.nodes, bad.boxes)
    with pytest.raises(hierarchy.ChunkValidationError, match="bad.hier") as ei:
        hierarchy.merge_hierarchies_gpu([p])
    assert ei.value.node == node


def _setup_chunks(root, specs, dev):
    """specs: (name, P, tail, file name, center, extent) -> the chunks (device, untrimmed) as written."""
    from gaussian_hierarchy._C import write_hierarchy
    trained, chunks_dir = root / "trained_chunks", root / "chunks"
    out = []
    for i, (name, P, tail, fname, center, extent) in enumerate(specs):
        h = _chunk(P, seed=20 + i, dev=dev, shift=(5.0 * i, 0.0))
        if tail:
            h = _with_tail(h, tail, seed=i)
        d = trained / name
        d.mkdir(parents=True)
        write_hierarchy(str(d / fname), h.xyz, h.shs, h.alpha, h.log_scales, h.rots, h.nodes, h.boxes)
        if center is not None:
            (chunks_dir / name).mkdir(parents=True)
            (chunks_dir / name / "center.txt").write_text(" ".join(str(v) for v in center))
            (chunks_dir / name / "extent.txt").write_text(" ".join(str(v) for v in extent))
        out.append(h)
    return trained, chunks_dir, out


def test_merge_command_end_to_end(gpu, tmp_path, capsys):
    from gaussian_hierarchy._C import load_hierarchy
    specs = [("0_0", 3000, 400, "hierarchy.hier_opt", (0.0, 0.0, 0.0), (4.0, 4.0, 10.0)),
             ("0_1", 1234, 0, "hierarchy.hier", (5.0, 0.5, 0.0), (3.0, 3.0, 3.0)),
             ("1_0", 777, 55, "hierarchy.hier_opt", (10.0, 0.0, 1.0), (100.0, 1.0, 1.0))]
    trained, chunks_dir, chunks = _setup_chunks(tmp_path, specs, gpu)
    out = tmp_path / "out" / "merged.hier"
    names = [s[0] for s in specs]
    assert merge_hierarchies.main([str(trained), "0", str(chunks_dir), str(out)] + names) == 0
    printed = capsys.readouterr().out
    assert "0_1: no hierarchy.hier_opt" in printed and "dropped 455 skybox rows" in printed, printed
    got = hierarchy.Hierarchy(*load_hierarchy(str(out)))
    trimmed = [_cpu(_trim(c)) for c in chunks]
    compare_to_spec(got, hierarchy.merge_hierarchies(trimmed))
    # drift: leaves outside their chunk's square, counted with numpy
    drift = 0
    for (_, _, _, _, center, extent), c in zip(specs, trimmed):
        leaf = (c.nodes[:, 6] == 0).numpy()
        d = np.abs(c.xyz.numpy()[leaf] - np.float32(center))
        drift += int((np.maximum(d[:, 0], d[:, 1]) > np.float32(0.5) * np.float32(extent[0])).sum())
    assert 0 < drift < sum(s[1] for s in specs)
    assert f" {drift} leaves outside their chunk" in printed, (drift, printed)


def test_merge_command_writes_nothing_for_a_corrupt_chunk(gpu, tmp_path, capsys):
    from gaussian_hierarchy._C import write_hierarchy
    specs = [("a", 500, 10, "hierarchy.hier_opt", None, None), ("b", 300, 0, "hierarchy.hier_opt", None, None)]
    trained, chunks_dir, chunks = _setup_chunks(tmp_path, specs, gpu)
    bad, _, node = _corrupt("unclaimed_child", chunks[1])
    write_hierarchy(str(trained / "b" / "hierarchy.hier_opt"), bad.xyz, bad.shs, bad.alpha, bad.log_scales, bad.rots,
                    bad.nodes, bad.boxes)
    out = tmp_path / "merged.hier"
    assert merge_hierarchies.main([str(trained), "0", str(chunks_dir), str(out), "a", "b"]) == 1
    err = capsys.readouterr().err
    assert "hierarchy.hier_opt" in err and f"first offending node {node}" in err, err
    assert not out.exists()


def test_lod_cut_weights_and_render_on_the_merged_file(gpu, tmp_path):
    """expand_to_size + get_interpolation_weights + one frame through the in-op LOD path: the merged file (written and
    loaded back) against the spec's hierarchy, at a tau whose cut excludes the root."""
    import diff_gaussian_rasterization as dgr
    from gaussian_hierarchy import _C as gh
    chunks = [_chunk(P, seed=30 + i, dev=gpu, shift=(0.6 * i - 0.6, 0.3 * i)) for i, P in enumerate((3000, 2500, 4001))]
    m = hierarchy.merge_hierarchies_gpu(chunks, gpu)
    path = str(tmp_path / "merged.hier")
    gh.write_hierarchy(path, m.xyz, m.shs, m.alpha, m.log_scales, m.rots, m.nodes, m.boxes)
    hg = hierarchy.Hierarchy(*(t.to(gpu) for t in gh.load_hierarchy(path)))
    hs = hierarchy.merge_hierarchies(chunks)                           # the spec on the device-held chunks
    G = hg.num_nodes
    assert gh._boxes_nested(hg.nodes, hg.boxes)
    tau = (2 * (4 + 0.5)) * CAM.tanfovx / (0.5 * CAM.image_width)
    cut = {}
    for key, h in (("g", hg), ("s", hs)):
        ri = torch.zeros(G, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
        w = torch.zeros(G, device=gpu); ns = torch.zeros(G, dtype=torch.int32, device=gpu)
        n = gh.expand_to_size(h.nodes, h.boxes, tau, CAM.camera_center.to(gpu), torch.zeros(3), ri, pi, ni)
        gh.get_interpolation_weights(ni[:n], tau, h.nodes, h.boxes, CAM.camera_center.cpu(), torch.zeros(3), w, ns)
        cut[key] = (n, ri, pi, ni, w, ns)
    n = cut["g"][0]
    assert n == cut["s"][0] and 0 < n < G
    for a, b in zip(cut["g"][1:], cut["s"][1:]):
        assert torch.equal(_bits(a[:n]) if a.dtype == torch.float32 else a[:n],
                           _bits(b[:n]) if b.dtype == torch.float32 else b[:n])
    _, ri, pi, ni, w, ns = cut["g"]
    assert not bool((ri[:n] == 0).any()), "the cut must exclude the root"
    assert bool(((w[:n] > 0) & (w[:n] < 1)).any()), "the cut must blend for the comparison to mean anything"

    def render(h):
        kw = pa.settings_kwargs(CAM, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=w,
                                num_node_kids=ns)
        kw["render_indices"], kw["parent_indices"] = ri[:n].contiguous(), pi
        r = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw))
        with torch.no_grad():
            color, radii, _ = r(means3D=h.xyz, means2D=torch.zeros(G, 3, device=gpu), shs=h.shs,
                                opacities=h.alpha.abs(), scales=torch.exp(h.log_scales),
                                rotations=torch.nn.functional.normalize(h.rots))
        return color.cpu(), radii.cpu()

    cg, rg = render(hg)
    cs, rs = render(hs)
    assert float(cs.max()) > 0.05
    assert torch.equal(rg, rs)
    if bool((pi[:n] == 0).any()):        # a chunk root blends with the root row (2 ulp of the spec's)
        st = pa.err_stats(cg, cs)
        assert st["maxrel"] <= 1e-5 and st["l2"] <= 1e-5, st
    else:
        assert torch.equal(cg, cs)


def _hier_bytes(N, M=16):
    return N * (12 + 12 * M + 4 + 12 + 16 + 28 + 32)


def test_device_memory_of_a_merge_from_files(gpu, tmp_path):
    """Peak device memory over merge_hierarchies_gpu with path sources (8 chunks of ~250 k leaves): at most the merged
    hierarchy + one chunk's staged nodes + 64 MB, and below the spec's own peak on the same chunks held on the device."""
    from gaussian_hierarchy._C import write_hierarchy
    Ps = [250_000 + 1000 * i for i in range(8)]
    paths = []
    for i, P in enumerate(Ps):
        h = _chunk(P, seed=40 + i, dev=gpu, shift=(2.0 * i, 0.0))
        p = str(tmp_path / f"c{i}.hier")
        write_hierarchy(p, h.xyz, h.shs, h.alpha, h.log_scales, h.rots, h.nodes, h.boxes)
        paths.append(p)
        del h
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    _, N = hierarchy.merge_layout([2 * P - 1 for P in Ps])
    bound = _hier_bytes(N) + 28 * (2 * max(Ps) - 1) + (64 << 20)
    base = torch.cuda.memory_allocated(gpu)
    torch.cuda.reset_peak_memory_stats(gpu)
    hg = hierarchy.merge_hierarchies_gpu(paths, gpu)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(gpu) - base
    print(f"merge of {len(Ps)} chunk files, N = {N}: device peak {peak / 2**20:.1f} MB, merged "
          f"{_hier_bytes(N) / 2**20:.1f} MB, bound {bound / 2**20:.1f} MB")
    assert peak <= bound, (peak, bound)
    # the spec on the same chunks, held on the device
    from gaussian_hierarchy._C import load_hierarchy
    chunks = [hierarchy.Hierarchy(*(t.to(gpu) for t in load_hierarchy(p))) for p in paths]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(gpu)
    torch.cuda.reset_peak_memory_stats(gpu)
    hs = hierarchy.merge_hierarchies(chunks)
    torch.cuda.synchronize()
    spec_peak = torch.cuda.max_memory_allocated(gpu) - base
    print(f"spec peak {spec_peak / 2**20:.1f} MB (the chunks themselves not counted)")
    assert bound < spec_peak, (bound, spec_peak)
    compare_to_spec(hg, hs)


def test_thirty_million_nodes_structure_and_time(gpu):
    Ps = [2_500_000 + 1111 * i for i in range(6)]
    chunks = [hierarchy.build_hierarchy_on_device(P, CAM, gpu, seed=50 + i) for i, P in enumerate(Ps)]
    _, N = hierarchy.merge_layout([c.num_nodes for c in chunks])
    assert N > 29_000_000
    hierarchy.merge_hierarchies_gpu(chunks[:1], gpu)                          # warm-up
    stats = {}
    torch.cuda.synchronize()
    h = hierarchy.merge_hierarchies_gpu(chunks, gpu, stats)
    torch.cuda.synchronize()
    print(f"merge of {len(Ps)} device-resident chunks, N = {N} nodes ({_hier_bytes(N) / 2**30:.2f} GB): "
          f"{stats['merge_ms']:.2f} ms on the device")
    del chunks
    nd = h.nodes.long()
    assert nd.shape == (N, 7)
    ids = torch.arange(N, device=gpu)
    assert torch.equal(nd[:, 2], ids)
    assert nd[0].tolist() == [0, -1, 0, 0, 1, 1, len(Ps)]
    par = nd[1:, 1]
    assert bool(((par >= 0) & (par < N)).all())
    ps, pc = nd[par, 5], nd[par, 6]
    assert bool(((ids[1:] >= ps) & (ids[1:] < ps + pc)).all()), "every node inside its parent's children range"
    assert torch.equal(nd[1:, 0], nd[par, 0] + 1), "depth = parent depth + 1"
    assert int(nd[:, 6].sum()) == N - 1
    al = h.alpha[0, 0]
    assert 0.0 <= float(al) <= 1.0 and bool(torch.isfinite(h.xyz[0]).all() & torch.isfinite(h.log_scales[0]).all())
