"""GPU parity of the hierarchy LOD cut, distCUDA2 and the render_post-style hierarchy rendering flow
(train_post.py:91-129, render_hierarchy.py:58-92) against the CPU oracles.  Index outputs bit-exact."""
import numpy as np
import pytest
import torch

from boundary_fixtures import lod_lerp
from hgs import hierarchy, synth
from oracle import lod_oracle as lo

pytestmark = pytest.mark.gpu


def _setup(P, gpu, seed=2):
    cam = synth.make_camera(256, 160)
    h = hierarchy.build_hierarchy(synth.make_scene(P, cam, seed=seed))
    return h, cam, h.nodes.to(gpu), h.boxes.to(gpu)


@pytest.mark.parametrize("P", [1, 2, 1000, 50_000])
def test_expand_to_size_and_weights_match_oracle(gpu, P):
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    h, cam, nodes, boxes = _setup(P, gpu)
    G = h.xyz.shape[0]
    ri = torch.zeros(G, dtype=torch.int32, device=gpu)
    pi = torch.zeros(G, dtype=torch.int32, device=gpu)
    ni = torch.zeros(G, dtype=torch.int32, device=gpu)
    w = torch.zeros(G, dtype=torch.float32, device=gpu)
    ns = torch.zeros(G, dtype=torch.int32, device=gpu)
    for vp in (torch.tensor([0.0, 0.0, 0.0]), torch.tensor([0.3, -0.1, 5.0]), torch.tensor([1.0, 2.0, -4.0])):
        for tau in (0.0, 0.002, 0.01, 0.06, 0.5, 1e4):
            # call shapes exactly as train_post.py:91-113: viewpoint on the GPU for expand, CPU for the weights
            n = expand_to_size(nodes, boxes, tau, vp.to(gpu), torch.zeros(3), ri, pi, ni)
            r_o, p_o, n_o = lo.expand_to_size(h.nodes.numpy(), h.boxes.numpy(), tau, vp.numpy())
            assert n == len(r_o), (P, tau, n, len(r_o))
            assert np.array_equal(ri[:n].cpu().numpy(), r_o)
            assert np.array_equal(pi[:n].cpu().numpy(), p_o)
            assert np.array_equal(ni[:n].cpu().numpy(), n_o)
            get_interpolation_weights(ni[:n], tau, nodes, boxes, vp.cpu(), torch.zeros(3), w, ns)
            w_o, k_o = lo.get_interpolation_weights(n_o, tau, h.nodes.numpy(), h.boxes.numpy(), vp.numpy())
            assert np.array_equal(ns[:n].cpu().numpy(), k_o)
            assert np.array_equal(w[:n].cpu().numpy().view(np.uint32), w_o.view(np.uint32)), "weights must be bit-exact"


def test_viewpoint_on_the_gpu_is_cached_per_tensor_and_follows_in_place_edits(gpu):
    """expand_to_size takes the viewpoint as a GPU tensor (train_post.py:96); with set_viewpoint_cache(True) the wrapper
    remembers its host copy on the tensor object, keyed by (data_ptr, version counter): the same tensor again costs no
    device-to-host read, an in-place edit is seen, another tensor with other values is another viewpoint.  Off (the
    default): nothing is remembered."""
    from gaussian_hierarchy import _C as gh
    from gaussian_hierarchy._C import expand_to_size
    h, cam, nodes, boxes = _setup(20_000, gpu)
    G = h.xyz.shape[0]
    ri = torch.zeros(G, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    tau = 0.06
    a, b = torch.tensor([0.0, 0.0, 0.0]), torch.tensor([1.0, 2.0, -4.0])
    want = {k: lo.expand_to_size(h.nodes.numpy(), h.boxes.numpy(), tau, v.numpy())[0] for k, v in (("a", a), ("b", b))}
    assert not np.array_equal(want["a"], want["b"])
    vp = a.to(gpu)
    n = expand_to_size(nodes, boxes, tau, vp, torch.zeros(3), ri, pi, ni)
    assert not hasattr(vp, "_hgs_vec3")                  # default: no cache; a write that bypasses the version counter
    vp.data.copy_(b)                                     # is therefore seen
    n = expand_to_size(nodes, boxes, tau, vp, torch.zeros(3), ri, pi, ni)
    assert np.array_equal(ri[:n].cpu().numpy(), want["b"])
    prev = gh.set_viewpoint_cache(True)
    try:
        vp = a.to(gpu)
        for _ in range(2):                               # second call: served from the tensor's cached host copy
            n = expand_to_size(nodes, boxes, tau, vp, torch.zeros(3), ri, pi, ni)
            assert np.array_equal(ri[:n].cpu().numpy(), want["a"])
        assert getattr(vp, "_hgs_vec3")[0] == (vp.data_ptr(), vp._version)
        vp.copy_(b)                                      # in place: the version counter moves, the cache is stale
        n = expand_to_size(nodes, boxes, tau, vp, torch.zeros(3), ri, pi, ni)
        assert np.array_equal(ri[:n].cpu().numpy(), want["b"])
        n = expand_to_size(nodes, boxes, tau, a.to(gpu), torch.zeros(3), ri, pi, ni)      # a fresh tensor
        assert np.array_equal(ri[:n].cpu().numpy(), want["a"])
    finally:
        gh.set_viewpoint_cache(prev)


def test_single_pass_and_level_by_level_cuts_agree(gpu):
    """Hierarchies whose boxes nest take the single-pass kernel (hgs_expand_to_size_nested), anything else the
    level-by-level expansion; both must give the oracle's cut.  A hierarchy is made non-nested by letting one box stick
    out of its parent's (in place: the cached answer of the nesting check must be invalidated by the edit)."""
    import ctypes as C
    from gaussian_hierarchy import _C as gh
    from gaussian_hierarchy._C import expand_to_size
    from hgs import _lib
    h, cam, nodes, boxes = _setup(20_000, gpu, seed=4)
    G = h.xyz.shape[0]
    assert gh._boxes_nested(nodes, boxes)
    ri = torch.zeros(G, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    vp = torch.tensor([0.3, -0.2, -0.5])
    lib = _lib.lib()
    tmp = torch.empty(lib.hgs_expand_tmp_bytes(G), dtype=torch.uint8, device=gpu)
    p = _lib.ptr
    v3 = lambda t: (C.c_float * 3)(*[float(x) for x in t])
    for tau in (0.0, 0.004, 0.03, 0.4, 1e4):
        r_o, p_o, n_o = lo.expand_to_size(h.nodes.numpy(), h.boxes.numpy(), tau, vp.numpy())
        for fn in (lib.hgs_expand_to_size_nested, lib.hgs_expand_to_size):
            cnt = C.c_int32(0)
            ri.fill_(-7); pi.fill_(-7); ni.fill_(-7)
            _lib.check(fn(p(nodes), p(boxes), G, float(tau), v3(vp), v3(torch.zeros(3)), p(ri), p(pi), p(ni), G, p(tmp),
                          C.byref(cnt), C.c_void_p(torch.cuda.current_stream().cuda_stream), 0), "expand")
            n = cnt.value
            assert n == len(r_o)
            assert np.array_equal(ri[:n].cpu().numpy(), r_o) and np.array_equal(pi[:n].cpu().numpy(), p_o)
            assert np.array_equal(ni[:n].cpu().numpy(), n_o)
    # a child box that sticks out of its parent's: the sizes are no longer monotone for every viewpoint
    child = int(torch.nonzero(h.nodes[:, 1] > 0)[5])
    boxes[child, 1, :3] += 50.0
    hb = h.boxes.clone(); hb[child, 1, :3] += 50.0
    assert not gh._boxes_nested(nodes, boxes)
    for tau in (0.004, 0.03, 0.4):
        n = expand_to_size(nodes, boxes, tau, vp.to(gpu), torch.zeros(3), ri, pi, ni)     # picks the general path
        r_o, p_o, n_o = lo.expand_to_size(h.nodes.numpy(), hb.numpy(), tau, vp.numpy())
        assert n == len(r_o) and np.array_equal(ri[:n].cpu().numpy(), r_o) and np.array_equal(ni[:n].cpu().numpy(), n_o)


def test_dist_knn3_matches_brute_force(gpu):
    from simple_knn._C import distCUDA2
    g = torch.Generator().manual_seed(3)
    for P in (4, 300, 5000):
        pts = torch.randn(P, 3, generator=g) * torch.tensor([3.0, 1.0, 0.2])
        pts[: P // 10] = pts[: P // 10].round()                      # clusters + exact duplicates
        got = distCUDA2(pts.to(gpu)).cpu()
        d2 = torch.cdist(pts.double(), pts.double()) ** 2
        d2.fill_diagonal_(float("inf"))
        ref = d2.topk(3, dim=1, largest=False).values.mean(1).float()
        assert torch.allclose(got, ref, rtol=1e-4, atol=1e-6), P


def test_render_post_flow(gpu):
    """The whole hierarchy-mode step of train_post.py / render_hierarchy.py with our packages: cut ->
    weights -> attribute lerp (as gaussian_renderer/__init__.py:199-234) -> rasterizer with the LOD tensors."""
    import diff_gaussian_rasterization as dgr
    import parity as pa
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    h, cam, nodes, boxes = _setup(3000, gpu, seed=5)
    G = h.xyz.shape[0]
    dev = gpu
    ri = torch.zeros(G, dtype=torch.int32, device=dev); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(G, device=dev); ns = torch.zeros(G, dtype=torch.int32, device=dev)
    tau = (2 * (3 + 0.5)) * cam.tanfovx / (0.5 * cam.image_width)           # render_hierarchy.py:55-56, tau=3
    n = expand_to_size(nodes, boxes, tau, cam.camera_center.to(dev), torch.zeros(3), ri, pi, ni)
    assert 0 < n < G
    get_interpolation_weights(ni[:n], tau, nodes, boxes, cam.camera_center.cpu(), torch.zeros(3), w, ns)
    full = dict(xyz=h.xyz.to(dev), scaling=torch.exp(h.log_scales.to(dev)),
                rotation=torch.nn.functional.normalize(h.rots.to(dev)), opacity=h.alpha.to(dev).abs(),
                features=h.shs.to(dev))
    L = lod_lerp(full, ri[:n].long(), pi[:n].long(), w[:n])
    scene = synth.Scene(*(L[k].cpu() for k in ("xyz", "scaling", "rotation", "opacity", "features")), 3)
    gc, gd = synth.upstream_grads(cam.image_height, cam.image_width)
    bg = torch.zeros(3)
    res = pa.verify_pair(scene, cam, bg, gc, gd, dev, interpolation_weights=w, num_node_kids=ns, do_depth=False)
    idx, st = res["indices"], res["stats"]
    print(idx, st)
    assert all(v == 0 for v in idx.values()), idx
    assert st["fragile_unmatched"] == 0 and st["fragile_unenumerated"] == 0, st
    assert st["n_contrib_mismatch"] == 0, st["n_contrib_mismatch"]
    for k, v in st.items():
        if isinstance(v, dict):
            assert v["maxrel"] <= pa.REL_TOL and v["l2"] <= pa.REL_TOL, (k, v)


def test_million_leaf_hierarchy_cut_and_render(gpu):
    """BASELINE config 3/5 shape: a 1 M-leaf hierarchy (2 M nodes) resident on the GPU, cut per view for a few
    granularities (render_hierarchy.py:55-66), weights, python-side lerp, 1080p render (forward only, like
    render_hierarchy.py's @torch.no_grad loop).  Cut + weights bit-exact vs the oracle; image sanity."""
    import diff_gaussian_rasterization as dgr
    import parity as pa
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    W, H = 1920, 1080
    cam = synth.make_camera(W, H)
    h = hierarchy.build_hierarchy(synth.make_scene(1_000_000, cam, seed=0))
    nodes, boxes = h.nodes.to(gpu), h.boxes.to(gpu)
    G = h.xyz.shape[0]
    ri = torch.zeros(G, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(G, device=gpu); ns = torch.zeros(G, dtype=torch.int32, device=gpu)
    full = dict(xyz=h.xyz.to(gpu), scaling=torch.exp(h.log_scales.to(gpu)),
                rotation=torch.nn.functional.normalize(h.rots.to(gpu)), opacity=h.alpha.to(gpu).abs(),
                features=h.shs.to(gpu))
    prev_n = None
    for tau_px in (0.0, 3.0, 15.0):
        tau = (2 * (tau_px + 0.5)) * cam.tanfovx / (0.5 * W)
        n = expand_to_size(nodes, boxes, tau, cam.camera_center.to(gpu), torch.zeros(3), ri, pi, ni)
        r_o, p_o, n_o = lo.expand_to_size(h.nodes.numpy(), h.boxes.numpy(), tau, cam.camera_center.numpy())
        assert n == len(r_o) and np.array_equal(ri[:n].cpu().numpy(), r_o) and np.array_equal(pi[:n].cpu().numpy(), p_o)
        get_interpolation_weights(ni[:n], tau, nodes, boxes, cam.camera_center.cpu(), torch.zeros(3), w, ns)
        w_o, k_o = lo.get_interpolation_weights(n_o, tau, h.nodes.numpy(), h.boxes.numpy(), cam.camera_center.numpy())
        assert np.array_equal(w[:n].cpu().numpy().view(np.uint32), w_o.view(np.uint32))
        assert np.array_equal(ns[:n].cpu().numpy(), k_o)
        if prev_n is not None:
            assert n <= prev_n
        prev_n = n
        with torch.no_grad():
            L = lod_lerp(full, ri[:n].long(), pi[:n].long(), w[:n])
            rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(
                cam, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=w, num_node_kids=ns))
            color, radii, _ = dgr.GaussianRasterizer(rs)(
                means3D=L["xyz"].contiguous(), means2D=torch.zeros(n, 3, device=gpu),
                shs=L["features"].contiguous(), opacities=L["opacity"].contiguous(),
                scales=L["scaling"].contiguous(), rotations=L["rotation"].contiguous())
        assert torch.isfinite(color).all() and float(color.max()) > 0.05
        assert int((radii > 0).sum()) > 0.5 * n
        print(f"tau={tau_px}px: cut {n} of {G} nodes, mean colour {float(color.mean()):.4f}")


def in_op_lod_against_python_glue(gpu, h, cam, skybox, n, ri, pi, w, ns):
    """The body of test_in_op_lod_interpolation_matches_python_glue behind its cut: ``h`` a host hierarchy, ``ri``,
    ``pi``, ``w``, ``ns`` device tensors of G = N + skybox entries whose first ``n`` hold a cut of it (also called by
    tests/test_hier_chain_gpu.py on a pruned hierarchy)."""
    import diff_gaussian_rasterization as dgr
    import parity as pa
    G = h.xyz.shape[0] + skybox
    gc, gd = synth.upstream_grads(cam.image_height, cam.image_width)
    gc = gc.to(gpu)
    sky = synth.make_scene(max(skybox, 1), cam, seed=77, s_px=(6.0, 20.0), z_range=(25.0, 40.0))   # far, large

    def leaves():
        tail = lambda a, b: torch.cat((a, b[:skybox].to(a)))
        mk = lambda t: t.to(gpu).clone().requires_grad_(True)
        return dict(xyz=mk(tail(h.xyz, sky.means3D)), sc=mk(tail(torch.exp(h.log_scales), sky.scales)),
                    rot=mk(tail(torch.nn.functional.normalize(h.rots), sky.rotations)), shs=mk(tail(h.shs, sky.shs)),
                    op=mk(tail(h.alpha.abs(), sky.opacities)))

    def settings(render_indices, parent_indices, weights, kids):
        kw = pa.settings_kwargs(cam, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=weights,
                                num_node_kids=kids)
        kw["render_indices"], kw["parent_indices"] = render_indices, parent_indices
        return dgr.GaussianRasterizationSettings(**kw)

    # (a) python-side lerp exactly as the reference glue, rows handed to the op
    A = leaves()
    r, p = ri[:n].long(), pi[:n].long()
    L = lod_lerp(dict(xyz=A["xyz"], scaling=A["sc"], rotation=A["rot"], opacity=A["op"], features=A["shs"]), r, p, w[:n])
    sk = torch.arange(G - skybox, G, device=gpu)
    cat = lambda base, full: torch.cat((base, full[sk])).contiguous()
    wa, ka = w.clone(), ns.clone()                       # gaussian_renderer/__init__.py:232-234
    wa[n:n + skybox] = 1.0
    ka[n:n + skybox] = 1
    m2a = torch.zeros(n + skybox, 3, device=gpu, requires_grad=True)
    e = torch.empty(0, dtype=torch.int32, device=gpu)
    ca, ra, _ = dgr.GaussianRasterizer(settings(e, e, wa, ka))(
        means3D=cat(L["xyz"], A["xyz"]), means2D=m2a, shs=cat(L["features"], A["shs"]),
        opacities=cat(L["opacity"], A["op"]), scales=cat(L["scaling"], A["sc"]), rotations=cat(L["rotation"], A["rot"]))
    (ca * gc).sum().backward()
    # (b) in-op: full arrays + index tensors (+ the skybox count on the context)
    B = leaves()
    m2b = torch.zeros(G, 3, device=gpu, requires_grad=True)
    ctx = dgr.RasterContext(skybox_points=skybox) if skybox else None
    cb, rb, _ = dgr.GaussianRasterizer(settings(ri[:n].contiguous(), pi, w, ns), context=ctx)(
        means3D=B["xyz"], means2D=m2b, shs=B["shs"], opacities=B["op"], scales=B["sc"], rotations=B["rot"])
    (cb * gc).sum().backward()
    assert rb.shape[0] == n + skybox and torch.equal(ra, rb)
    if skybox:
        assert int((rb[n:] > 0).sum()) > 0, "the skybox must be on screen for the case to mean anything"
    # the in-op lerp rounds exactly like the torch expression (two rounded products, one rounded sum): same rows in,
    # same pixels out -- bit for bit, so no blend decision can flip between the two routes
    assert torch.equal(ca.detach(), cb.detach())
    touched = torch.zeros(G, dtype=torch.bool, device=gpu); touched[r] = True; touched[p] = True; touched[sk] = True
    for k in A:
        ga, gb = A[k].grad, B[k].grad
        scale = float(ga.abs().max())
        assert float((ga - gb).abs().max()) <= 2e-5 * scale, (k, float((ga - gb).abs().max()), scale)
        assert float(gb[~touched].abs().sum()) == 0.0
        if skybox:
            assert float(gb[sk].abs().sum()) > 0.0


@pytest.mark.parametrize("skybox", [0, 37])
def test_in_op_lod_interpolation_matches_python_glue(gpu, skybox):
    """render_indices / parent_indices passed NON-empty to the op must reproduce exactly what
    render_post's Python block (gaussian_renderer/__init__.py:199-234, restated here in torch) feeds it,
    forward and backward (gradients land on node AND parent rows) -- including the skybox rows the reference appends
    from the TAIL of the arrays with weight 1 / 1 sibling (:220-234; RasterContext.skybox_points here)."""
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    h, cam, nodes, boxes = _setup(4000, gpu, seed=9)
    Gh = h.xyz.shape[0]
    G = Gh + skybox
    ri = torch.zeros(G, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(G, device=gpu); ns = torch.zeros(G, dtype=torch.int32, device=gpu)
    tau = (2 * (4 + 0.5)) * cam.tanfovx / (0.5 * cam.image_width)
    n = expand_to_size(nodes, boxes, tau, cam.camera_center.to(gpu), torch.zeros(3), ri, pi, ni)
    assert 0 < n < Gh
    get_interpolation_weights(ni[:n], tau, nodes, boxes, cam.camera_center.cpu(), torch.zeros(3), w, ns)
    in_op_lod_against_python_glue(gpu, h, cam, skybox, n, ri, pi, w, ns)


@pytest.mark.parametrize("order", ["as_emitted", "shuffled"])
def test_in_kernel_lod_scatter_equals_separate_scatter(gpu, order):
    """The backward of the in-op LOD interpolation scatters node / parent gradients inside its per-Gaussian kernels
    (hgs_raster_args.lod_scatter: run-leader sums when the parents are non-decreasing, atomic adds otherwise) -- same
    gradients as the row gradients + hgs_lod_gather_bwd route, for the order expand_to_size emits and for a shuffled
    cut (parents no longer sorted: the atomic fallback)."""
    import diff_gaussian_rasterization as dgr
    import parity as pa
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    h, cam, nodes, boxes = _setup(6000, gpu, seed=4)
    G = h.xyz.shape[0]
    ri = torch.zeros(G, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(G, device=gpu); ns = torch.zeros(G, dtype=torch.int32, device=gpu)
    tau = (2 * (3 + 0.5)) * cam.tanfovx / (0.5 * cam.image_width)
    n = expand_to_size(nodes, boxes, tau, cam.camera_center.to(gpu), torch.zeros(3), ri, pi, ni)
    assert 300 < n < G           # several workgroups: runs of siblings cross their boundaries
    get_interpolation_weights(ni[:n], tau, nodes, boxes, cam.camera_center.cpu(), torch.zeros(3), w, ns)
    if order == "shuffled":
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(gpu)
        for t in (ri, pi, w, ns):
            t[:n] = t[:n][perm]
        assert bool((pi[1:n] < pi[:n - 1]).any())
    else:
        assert not bool((pi[1:n] < pi[:n - 1]).any())
    gc, _ = synth.upstream_grads(cam.image_height, cam.image_width)
    gc = gc.to(gpu)
    kw = pa.settings_kwargs(cam, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=w, num_node_kids=ns)
    kw["render_indices"], kw["parent_indices"] = ri[:n].contiguous(), pi
    rs = dgr.GaussianRasterizationSettings(**kw)

    def run(in_kernel):
        mk = lambda t: t.to(gpu).clone().requires_grad_(True)
        L = dict(xyz=mk(h.xyz), sc=mk(torch.exp(h.log_scales)), rot=mk(torch.nn.functional.normalize(h.rots)),
                 shs=mk(h.shs), op=mk(h.alpha.abs()))
        m2 = torch.zeros(G, 3, device=gpu, requires_grad=True)
        dgr._C.lod_scatter_in_kernel = in_kernel
        try:
            c, _, _ = dgr.GaussianRasterizer(rs)(means3D=L["xyz"], means2D=m2, shs=L["shs"], opacities=L["op"],
                                                scales=L["sc"], rotations=L["rot"])
            (c * gc).sum().backward()
        finally:
            dgr._C.lod_scatter_in_kernel = True
        return c.detach(), {k: v.grad for k, v in L.items()}, m2.grad

    ca, ga, m2a = run(True)
    cb, gb, m2b = run(False)
    assert torch.equal(ca, cb) and torch.equal(m2a, m2b)
    for k in ga:
        scale = float(gb[k].abs().max())
        assert scale > 0
        err = float((ga[k] - gb[k]).abs().max())
        assert err <= 2e-6 * scale, (k, err, scale)
    if order == "as_emitted":      # no atomics on this route: bit-reproducible
        _, ga2, _ = run(True)
        assert all(torch.equal(ga[k], ga2[k]) for k in ga)


def test_config5_scale_50m_node_hierarchy_4k(gpu):
    """BASELINE config 5 at its stated size: a 50 M-node hierarchy (25 M leaves, 15 GB) fully resident in HBM -- on a
    288 GB part the reference's "VRAM-budgeted streaming" is not needed -- cut per view and rendered at 3840x2160
    through the in-op LOD path (forward only, as render_hierarchy.py).  The full-array oracle is too slow here, so
    the cut is checked through size-independent properties: sorted unique indices, every leaf covered by exactly one
    cut node, the size criterion (oracle formula on the cut nodes and their parents), weights bit-exact vs the oracle."""
    import json, os, time
    import diff_gaussian_rasterization as dgr
    import parity as pa
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    W, H, P = 3840, 2160, 25_000_000
    cam = synth.make_camera(W, H)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    h = hierarchy.build_hierarchy_on_device(P, cam, torch.device(gpu), seed=0)
    torch.cuda.synchronize(); t_build = time.perf_counter() - t0
    G = h.nodes.shape[0]
    assert G == 2 * P - 1
    ri = torch.zeros(G, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(G, device=gpu); ns = torch.zeros(G, dtype=torch.int32, device=gpu)
    vp = cam.camera_center.to(gpu)
    depth = h.nodes[:, 0].long()
    level_counts = torch.unique_consecutive(depth, return_counts=True)[1].tolist()    # BFS numbering: levels are contiguous
    is_leaf = h.nodes[:, 6] == 0
    log = {"case": "config5_50M_nodes_4k", "nodes": G, "build_s": t_build}
    prev_n = None
    for tau_px in (1.0, 6.0):
        tau = (2 * tau_px + 1) * cam.tanfovx / (0.5 * W)                    # render_hierarchy.py:55-56
        expand_to_size(h.nodes, h.boxes, tau, vp, torch.zeros(3), ri, pi, ni)      # warm-up (workspace allocation)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        n = expand_to_size(h.nodes, h.boxes, tau, vp, torch.zeros(3), ri, pi, ni)
        torch.cuda.synchronize(); t_cut = time.perf_counter() - t0
        get_interpolation_weights(ni[:n], tau, h.nodes, h.boxes, cam.camera_center.cpu(), torch.zeros(3), w, ns)
        torch.cuda.synchronize(); t_w = time.perf_counter() - t0 - t_cut
        assert 0 < n < G
        r = ri[:n].long()
        assert bool((r[1:] > r[:-1]).all())                                  # ascending, unique
        # coverage: push the cut marks down the tree level by level; every leaf must end with exactly 1
        mark = torch.zeros(G, dtype=torch.int32, device=gpu)
        mark[r] = 1
        a = level_counts[0]
        for cnt in level_counts[1:]:
            ids = torch.arange(a, a + cnt, device=gpu)
            mark[ids] += mark[h.nodes[ids, 1].long()]
            a += cnt
        assert bool((mark[is_leaf] == 1).all())
        # size criterion with the oracle's formula on the cut nodes / their parents only
        nodes_cut = h.nodes[r].cpu().numpy(); boxes_cut = h.boxes[r].cpu().numpy()
        par = nodes_cut[:, 1].astype(np.int64)
        s_node = lo.node_size(boxes_cut, np.arange(n), cam.camera_center.numpy())
        assert ((s_node < np.float32(tau)) | (nodes_cut[:, 6] == 0)).all()
        has_par = par >= 0
        boxes_par = h.boxes[torch.from_numpy(par[has_par]).to(gpu)].cpu().numpy()
        s_par = lo.node_size(boxes_par, np.arange(boxes_par.shape[0]), cam.camera_center.numpy())
        assert (s_par >= np.float32(tau)).all()
        assert np.array_equal(pi[:n].cpu().numpy()[has_par], par[has_par])
        # weights: closed form on (size, parent size), bit-exact
        wn = w[:n].cpu().numpy()
        assert (wn >= 0).all() and (wn <= 1).all()
        sub = np.random.default_rng(0).choice(n, size=min(n, 200_000), replace=False)
        sub.sort()
        ids_sub = r[torch.from_numpy(sub).to(gpu)].cpu().numpy()
        need = np.unique(np.concatenate([ids_sub, par[sub][par[sub] >= 0]]))
        remap = {int(v): i for i, v in enumerate(need)}
        nodes_s = h.nodes[torch.from_numpy(need).to(gpu)].cpu().numpy().copy()
        boxes_s = h.boxes[torch.from_numpy(need).to(gpu)].cpu().numpy()
        nodes_s[:, 1] = [remap.get(int(p_), -1) for p_ in nodes_s[:, 1]]
        w_o, k_o = lo.get_interpolation_weights(np.array([remap[int(v)] for v in ids_sub]), tau, nodes_s, boxes_s,
                                                cam.camera_center.numpy())
        assert np.array_equal(wn[sub].view(np.uint32), w_o.view(np.uint32))
        if prev_n is not None:
            assert n <= prev_n
        prev_n = n
        # render through the in-op LOD path
        with torch.no_grad():
            kw = pa.settings_kwargs(cam, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=w,
                                    num_node_kids=ns)
            kw["render_indices"], kw["parent_indices"] = ri[:n].contiguous(), pi
            rast = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw))
            args = dict(means3D=h.xyz, means2D=torch.zeros(G, 3, device=gpu), shs=h.shs, opacities=h.alpha,
                        scales=torch.exp(h.log_scales), rotations=h.rots)
            color, radii, _ = rast(**args)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            color, radii, _ = rast(**args)
            torch.cuda.synchronize(); t_render = time.perf_counter() - t0
        assert torch.isfinite(color).all() and float(color.max()) > 0.05
        assert int((radii > 0).sum()) > 0.5 * n
        log[f"tau{tau_px:g}px"] = {"cut": n, "cut_ms": t_cut * 1e3, "weights_ms": t_w * 1e3,
                                   "render_4k_ms": t_render * 1e3}
        print(f"tau={tau_px}px: cut {n} of {G}; cut {t_cut*1e3:.2f} ms, weights {t_w*1e3:.2f} ms, 4K render {t_render*1e3:.2f} ms")
    try:
        out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_log.jsonl"), "a") as f:
            f.write(json.dumps(log) + "\n")
    except OSError:
        pass


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("o", [0.3, 0.9, 1.3])
def test_lod_remap_parent_vs_children_on_the_device(gpu, k, o):
    """The KAT of tests/test_oracle_kat.py::test_lod_remap_parent_vs_children through the HIP op: one parent against
    its k coincident children at w = 0.  The device must reproduce the ORACLE's images (both follow the per-Gaussian
    remap ``lod_opacity``), and therefore also its distance from the remap's own rationale -- zero only at the
    centre, up to 0.29 in alpha for o = 1.3, k = 8 (profiles/r04_lod_remap_kat.txt)."""
    import json, os
    import parity as pa
    import test_oracle_kat as kat
    bg = torch.zeros(3)

    def hip_render(scene, cam, weights, kids):
        z = torch.zeros(cam.image_height, cam.image_width)
        return pa.run_hip(scene, cam, bg, z[None].expand(3, -1, -1), z[None], gpu, interpolation_weights=weights,
                          num_node_kids=kids, grad_mask=None)["color"].double()

    e_hip, parent_hip = kat.lod_parent_vs_children(hip_render, k, o)
    e_or, parent_or = kat.lod_parent_vs_children(kat._oracle_lod_render("opacity"), k, o)
    assert (parent_hip - parent_or).abs().max() <= 1e-5
    assert abs(e_hip - e_or) <= 2e-5
    exp = kat.lod_remap_expected(k, o)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_log.jsonl"), "a") as f:
            f.write(json.dumps({"case": "lod_remap_kat", "k": k, "o": o, "device_children_vs_parent": e_hip,
                                "oracle_children_vs_parent": e_or, "predicted": exp}) + "\n")
    except OSError:
        pass


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("o", [0.3, 0.9, 1.3])
def test_per_pixel_lod_remap_children_composite_like_their_parent(gpu, k, o, monkeypatch):
    """The same KAT with the remap applied per PIXEL to alpha inside K6 (``_C.LOD_REMAP = "alpha"``,
    hgs_raster_args.lod_per_pixel): k coincident children at w = 0 must give the parent's image at EVERY pixel, up to the
    share both readings lose to the 1/255 skip rule (each child carries ~alpha / k) -- and the device must reproduce the
    oracle's ``lod_mode="alpha"`` images."""
    import diff_gaussian_rasterization as dgr
    import parity as pa
    import test_oracle_kat as kat
    monkeypatch.setattr(dgr._C, "LOD_REMAP", "alpha")
    bg = torch.zeros(3)

    def hip_render(scene, cam, weights, kids):
        z = torch.zeros(cam.image_height, cam.image_width)
        return pa.run_hip(scene, cam, bg, z[None].expand(3, -1, -1), z[None], gpu, interpolation_weights=weights,
                          num_node_kids=kids, grad_mask=None)["color"].double()

    e_hip, parent_hip = kat.lod_parent_vs_children(hip_render, k, o)
    e_or, parent_or = kat.lod_parent_vs_children(kat._oracle_lod_render("alpha"), k, o)
    assert (parent_hip - parent_or).abs().max() <= 1e-5
    assert e_hip <= 1.01 * k / 255.0 and abs(e_hip - e_or) <= 2e-5, (e_hip, e_or)


@pytest.mark.gpu
@pytest.mark.parametrize("do_depth", [True, False])
def test_per_pixel_lod_remap_matches_the_oracle(gpu, do_depth, monkeypatch):
    """render_post's call shape (gaussian_renderer/__init__.py:247-277: weights and sibling counts longer than P,
    abs-activated opacities above 1) with the per-pixel remap: pixels and EVERY gradient against
    ``rasterize(lod_mode="alpha")``, indices bit-exact -- and the images of the two readings must actually differ."""
    import diff_gaussian_rasterization as dgr
    import parity as pa
    cam, scene, gc, gd = pa.default_case(3000, 208, 144, seed=23)
    g = torch.Generator().manual_seed(24)
    scene.opacities = (scene.opacities * 1.35).contiguous()
    w = torch.rand(scene.P + 50, generator=g)
    w[torch.rand(scene.P + 50, generator=g) < 0.2] = 1.0            # rows that are not in transition
    kids = torch.randint(1, 9, (scene.P + 50,), generator=g, dtype=torch.int32)
    bg = torch.tensor([0.1, 0.2, 0.05])
    monkeypatch.setattr(dgr._C, "LOD_REMAP", "alpha")
    # (norm-wise 1e-5 as everywhere; element-wise 1.5 x the bound: v_log_f32 / v_exp_f32 / v_rcp_f32 sit in every live
    # pixel's alpha AND in its derivative here -- measured 1.1 on d_means2D, 0.1 on the pixels)
    res = pa.verify_pair(scene, cam, bg, gc, gd, gpu, interpolation_weights=w, num_node_kids=kids, do_depth=do_depth,
                         lod_mode="alpha", mixed_tol=1.5)
    hip = res["hip"]
    pa.assert_verified("per-pixel LOD remap", res, mixed_tol=1.5, fragile_frac=1.0)
    monkeypatch.setattr(dgr._C, "LOD_REMAP", "opacity")
    other = pa.run_hip(scene, cam, bg, gc, gd, gpu, interpolation_weights=w, num_node_kids=kids, do_depth=do_depth,
                       grad_mask=None)
    assert (other["color"] - hip["color"]).abs().max() > 1e-2        # the two readings are different images


def _chain(n):
    """Node k has the single child k + 1 and one row, k: merged at the inner nodes, a leaf row at the last.  Every box
    is the same box, so the boxes nest and every node has the same size from every viewpoint."""
    nodes = np.zeros((n, 7), dtype=np.int32)
    k = np.arange(n)
    nodes[:, 0], nodes[:, 1], nodes[:, 2] = k, k - 1, k
    nodes[:-1, 4], nodes[:-1, 5], nodes[:-1, 6] = 1, k[1:], 1
    nodes[-1, 3] = 1
    boxes = np.tile(np.array([[-1.0, -1.0, -1.0, 1e3], [1.0, 1.0, 1.0, 0.0]], dtype=np.float32), (n, 1, 1))
    return nodes, boxes


@pytest.mark.parametrize("n", [8, 9, 64, 65])
def test_level_route_polls_every_8_levels_and_refuses_more_than_64(gpu, n):
    """The level-by-level route launches 8 levels, then looks at the frontier size: chains of 8, 9 and 64 nodes end at
    the first poll, need a second one, and end at the last poll the route has.  hgs_expand_to_size and
    cut_view(nested=False) share that loop and give the oracle's cut; at 65 levels both refuse a cut that has to go
    all the way down (a clean invalid-argument return), still answer one that stops at the root, and the single-pass
    routes give the oracle's cut whatever the depth."""
    import ctypes as C
    from hgs import _lib, frustum
    ERR_INVALID = 1                                        # HGS_ERR_INVALID (include/hgs.h)
    nodes_np, boxes_np = _chain(n)
    nodes, boxes = torch.from_numpy(nodes_np).to(gpu), torch.from_numpy(boxes_np).to(gpu)
    bounds = torch.zeros(n, 4, device=gpu)
    planes = torch.tensor([[0.0, 0.0, 1.0, 1e30]] * 5)     # every ball is inside
    vp = np.array([0.0, 0.0, 10.0], dtype=np.float32)
    lib, p = _lib.lib(), _lib.ptr
    ri = torch.zeros(n, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    tmp = torch.empty(lib.hgs_expand_tmp_bytes(n), dtype=torch.uint8, device=gpu)
    v3 = lambda t: (C.c_float * 3)(*[float(x) for x in t])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for tau, rows in ((1.0, (n - 1, n - 2)), (1e9, (0, 0))):
        r_o, p_o, n_o = lo.expand_to_size(nodes_np, boxes_np, tau, vp)
        w_o, k_o = lo.get_interpolation_weights(n_o, tau, nodes_np, boxes_np, vp)
        assert (r_o.tolist(), p_o.tolist(), w_o.tolist(), k_o.tolist()) == ([rows[0]], [rows[1]], [1.0], [1])
        too_deep = n > 64 and tau == 1.0
        for fn, fails in ((lib.hgs_expand_to_size, too_deep), (lib.hgs_expand_to_size_nested, False)):
            cnt = C.c_int32(0)
            ri.fill_(-7); pi.fill_(-7); ni.fill_(-7)
            rc = fn(p(nodes), p(boxes), n, tau, v3(vp), v3((0, 0, 0)), p(ri), p(pi), p(ni), n, p(tmp), C.byref(cnt),
                    stream, 0)
            if fails:
                assert rc == ERR_INVALID and b"deeper than 64 levels" in lib.hgs_last_error()
                continue
            _lib.check(rc, "expand")
            assert cnt.value == 1
            assert (ri[:1].tolist(), pi[:1].tolist(), ni[:1].tolist()) == (r_o.tolist(), p_o.tolist(), n_o.tolist())
        for nested, fails in ((False, too_deep), (True, False)):
            if fails:
                with pytest.raises(_lib.HgsError, match="deeper than 64 levels") as e:
                    frustum.cut_view(nodes, boxes, bounds, tau, vp, planes, 1.0, nested=nested)
                assert e.value.code == ERR_INVALID
                continue
            cv = frustum.cut_view(nodes, boxes, bounds, tau, vp, planes, 1.0, nested=nested)
            assert (cv.n, cv.n_unculled) == (1, 1)
            assert (cv.render_indices.tolist(), cv.parent_indices.tolist(), cv.node_indices.tolist()) == \
                (r_o.tolist(), p_o.tolist(), n_o.tolist())
            assert np.array_equal(cv.weights.cpu().numpy().view(np.uint32), w_o.view(np.uint32))
            assert cv.kids.tolist() == k_o.tolist()
