"""Generates the boundary fixtures tests/golden/boundary_*.npz by running the REFERENCE'S OWN code -- the render glue
gaussian_renderer/__init__.py and GaussianModel.create_from_pcd (scene/gaussian_model.py:146-205), imported from the
checkout HGS_REFERENCE names -- on the oracle-backed CPU stand-ins of tests/harness/cpu_backends.py, while
tests/harness/recorder.py records what crosses into this repository's packages.  Build machine only, like
make_golden.py:

    HGS_REFERENCE=<checkout> python tests/golden/make_boundary_golden.py

The reference's functions are called, never copied; the files hold numbers only (``np.load(..., allow_pickle=False)``),
every seed is fixed, and a second run reproduces every array of the direct-call files (tests/test_boundary_fixtures_cpu.py
checks it; the chain file depends on training, which drifts across BLAS builds).

Files
  boundary_direct.npz        op0 ``render`` (do_depth, trained exposure, the four empty "cuda" LOD tensors of :39-42);
                             op1 ``render`` at active SH degree 0 with 16 stored coefficients (train_single.py before its
                             first oneupSHdegree); op2 ``render_coarse`` (debug forced, :331);
                             knn0 / knn1 ``distCUDA2`` as create_from_pcd hands it the point cloud (:190), without and
                             with a skybox (:169-184)
  boundary_lod_<case>.npz    one ``render_post`` call each (:138, interp_python=True): op0 + lod0, and for the cases on a
                             real cut (hgs.hierarchy.build_hierarchy on a synth scene) cut0, the cut and weights calls
                             made as train_post.py:91-113 makes them.  Cases: ``cut`` (n > 300 entries, so sibling runs
                             cross 256-row workgroups), ``cut_skybox`` (skybox_points > 0), ``cut_deg1`` (16 -> 4 stored
                             coefficients, SH degree 1), ``edges`` (hand-placed entries: weights exactly 0 and 1, a root
                             that is its own parent, quaternion pairs with a dot of exactly 0, clearly < 0 and clearly > 0)
  boundary_chain.npz         samples of the reference's three scripts run unmodified and chained (see build_chain):
                             op0 first render of train_single.py (active SH degree 0, 16 stored coefficients), op1 the
                             first render after densify-and-prune changed P, op2 / op3 first / last render_post of
                             train_post.py, op4 / op5 first view of render_hierarchy.py at tau 0 / 15 (no backward);
                             cut0..cut3 the cut and weights calls of op2..op5; knn0 the initial distCUDA2.  Upstream
                             gradients are what the scripts' exposure, clamp and L1 + SSIM losses sent back.
Every LOD case keeps the precondition that no drawn row is another entry's parent row, and the generator asserts
that the oracle flags no knife-edge pixel in it (the recorded leaf gradients would be ambiguous otherwise).

Key schema (<op> = op<j>, <lod> = lod<j>, <cut> = cut<j>, <knn> = knn<j>; scalars are 0-d arrays)
  <op>__site                     0 render (:20), 1 render_post (:138), 2 render_coarse (:296)
  <op>__fragile                  pixels the oracle flagged as knife edges
  <op>__set__<field>             the 17 GaussianRasterizationSettings fields as passed
  <op>__arg__<name>              the call arguments as passed (means3D, means2D, shs, colors_precomp, opacities, scales,
                                 rotations, cov3D_precomp); an absent key is a None argument
  <op>__out__{color,radii,invdepth}   the op's outputs (oracle)
  <op>__gin__{color,invdepth}    the upstream gradients that reached them (no key: none reached it)
  <op>__gout__<name>             the gradients the op returned for its inputs, means2D included
                                 (no gin / gout keys at all: no backward ran, e.g. render_hierarchy.py's no_grad)
  <lod>__op                      the index j of the op record of this render_post call
  <lod>__skybox                  pc.skybox_points
  <lod>__full__<attr>            the full arrays render_post read: xyz, scaling, rotation, opacity, features
  <lod>__render_indices, __parent_indices, __weights, __kids     as passed in (before the edit of :232-234)
  <lod>__leafgrad__<attr>        gradient of the loss w.r.t. each full array: the reference's own autograd through
                                 its lerp (:199-234) of the op's gradients
  <lod>__viewspace_grad          gradient on the screen-space tensor render_post returns (:158; rows [:n + skybox])
  <cut>__nodes, __boxes, __size, __viewpoint, __viewdir, __capacity (numel of the three output tensors), __count,
  __render_indices, __parent_indices, __nodes_for_render_indices   an expand_to_size call and its outputs
  <cut>__w_size, __w_viewpoint, __w_capacity, __weights, __kids     the get_interpolation_weights call after it
  <knn>__points, __dist          distCUDA2's input and output (float64 brute force rounded to float32)
Where a GPU replay puts each tensor is what the cited lines do: everything on the GPU except the render_post LOD
fields that are empty (:145-148, :244-245), the viewdir of both cut calls (``torch.zeros((3))``) and the viewpoint of
get_interpolation_weights (``.cpu()``, train_post.py:109).
"""
import contextlib
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (TESTS, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H = 64, 48
LOD_CASES = ("cut", "cut_skybox", "cut_deg1", "edges")
MAX_FILE, MAX_TOTAL = 1 << 20, 4 << 20
FULL = ("xyz", "scaling", "rotation", "opacity", "features")
_REF_MODS = ("gaussian_renderer", "scene", "utils", "arguments", "lpipsPyTorch")


@contextlib.contextmanager
def reference(ref):
    """The reference's glue, imported from ``ref``, on the CPU stand-ins with the recorder on; restored on exit."""
    from harness import cpu_backends, recorder
    from harness.run_reference_script import CudaToCpu, _is_cuda
    import diff_gaussian_rasterization as dgr
    import gaussian_hierarchy._C as gh
    import simple_knn._C as knn
    saved = (dgr._C, gh.expand_to_size, gh.get_interpolation_weights, knn.distCUDA2)
    stubs = []
    for name in ("plyfile", "cv2"):                 # imported at load time, not used by what is called here
        if name not in sys.modules:
            m = types.ModuleType(name)
            if name == "plyfile":
                m.PlyData = type("PlyData", (), {})
                m.PlyElement = type("PlyElement", (), {})
            sys.modules[name] = m
            stubs.append(name)
    drop = lambda: [sys.modules.pop(m) for m in [m for m in sys.modules if m.split(".")[0] in _REF_MODS]]
    drop()
    sys.path.insert(0, ref)
    cpu_backends.install()
    rec = recorder.Recorder().install()
    rng = torch.range                               # (deprecated; does not consult the torch-function mode)
    torch.range = lambda *a, **k: rng(*a, **{**k, "device": "cpu"} if _is_cuda(k.get("device")) else k)
    try:
        with CudaToCpu():
            import gaussian_renderer
            from scene.gaussian_model import GaussianModel
            from utils.graphics_utils import BasicPointCloud
            yield types.SimpleNamespace(glue=gaussian_renderer, GaussianModel=GaussianModel,
                                        BasicPointCloud=BasicPointCloud, rec=rec)
    finally:
        torch.range = rng
        rec.uninstall()
        dgr._C, gh.expand_to_size, gh.get_interpolation_weights, knn.distCUDA2 = saved
        sys.path.remove(ref)
        drop()
        for name in stubs:
            sys.modules.pop(name, None)


class LeafModel:
    """Duck-typed GaussianModel: what gaussian_renderer reads (scene/gaussian_model.py:108-139), with the get_*
    properties returning LEAF tensors -- after backward their .grad is the reference's own autograd through its glue."""

    def __init__(self, full, active_sh_degree, skybox_points=0, exposure=None):
        self.leaves = {k: full[k].detach().clone().contiguous().requires_grad_(True) for k in FULL}
        self._xyz = self.leaves["xyz"]
        self.max_sh_degree = int(round(math.sqrt(full["features"].shape[1]))) - 1
        self.active_sh_degree = active_sh_degree
        self.skybox_points = skybox_points
        self.pretrained_exposures = None
        self._exposure = exposure

    get_xyz = property(lambda s: s.leaves["xyz"])
    get_scaling = property(lambda s: s.leaves["scaling"])
    get_rotation = property(lambda s: s.leaves["rotation"])
    get_opacity = property(lambda s: s.leaves["opacity"])
    get_features = property(lambda s: s.leaves["features"])

    def get_exposure_from_name(self, name):
        return self._exposure


def _viewpoint(cam):
    return types.SimpleNamespace(FoVx=cam.FoVx, FoVy=cam.FoVy, image_height=cam.image_height, image_width=cam.image_width,
                                 world_view_transform=cam.world_view_transform,
                                 full_proj_transform=cam.full_proj_transform, camera_center=cam.camera_center,
                                 image_name="v0")


_PIPE = dict(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


def _scene_full(s):
    return dict(xyz=s.means3D, scaling=s.scales, rotation=s.rotations, opacity=s.opacities, features=s.shs)


def direct(R):
    from hgs import synth
    cam = synth.make_camera(W, H)
    full = _scene_full(synth.make_scene(200, cam, seed=31))
    gc, gd = synth.upstream_grads(H, W, seed=32)
    pipe = types.SimpleNamespace(**_PIPE)
    exposure = torch.tensor([[0.9, 0.05, 0.0, 0.02], [0.0, 1.1, 0.05, -0.01], [0.03, 0.0, 0.95, 0.0]])
    i0 = len(R.rec.ops)
    pkg = R.glue.render(_viewpoint(cam), LeafModel(full, 3, exposure=exposure), pipe, torch.tensor([0.1, 0.2, 0.3]),
                        use_trained_exp=True)
    ((pkg["render"] * gc).sum() + (pkg["depth"] * gd).sum()).backward()
    pkg = R.glue.render(_viewpoint(cam), LeafModel(full, 0), pipe, torch.zeros(3))
    ((pkg["render"] * gc).sum() + (pkg["depth"] * gd).sum()).backward()
    pkg = R.glue.render_coarse(_viewpoint(cam), LeafModel(full, 3), pipe, torch.tensor([0.0, 0.3, 0.1]))
    (pkg["render"] * gc).sum().backward()
    assert len(R.rec.ops) == i0 + 3 and [R.rec.ops[i]["site"] for i in range(i0, i0 + 3)] == [0, 0, 2]
    # the SfM cloud create_from_pcd hands distCUDA2: a synthetic scene's centres with clusters and exact duplicates
    k0 = len(R.rec.knn)
    pts = synth.make_scene(1500, cam, seed=33, z_range=(2.0, 12.0)).means3D.double()
    pts[:150] = (pts[:150] * 8).round() / 8
    pts[150:180] = pts[:30]
    g = torch.Generator().manual_seed(34)
    for sky in (0, 64):
        torch.manual_seed(35)                            # the skybox directions (:173-174) come from torch.rand
        pcd = R.BasicPointCloud(points=pts.numpy(), colors=torch.rand(pts.shape[0], 3, generator=g).double().numpy(),
                                normals=np.zeros((pts.shape[0], 3)))
        R.GaussianModel(3).create_from_pcd(pcd, [types.SimpleNamespace(image_name="v0")], 1.0, sky, "", "", True)
    return R.rec.arrays(ops=range(i0, i0 + 3), cuts=[], knn=range(k0, len(R.rec.knn)))


def _edge_entries(full):
    """Hand-placed cut entries on 48 rows: (render row, parent row, weight); drawn rows 0..14 and 20, parents 30..39."""
    rot = full["rotation"].clone()
    nrm = lambda v: v / v.norm()
    rot[10], rot[34] = torch.tensor([1.0, 0.0, 0.0, 0.0]), torch.tensor([0.0, 0.0, 1.0, 0.0])      # dot exactly 0
    rot[11], rot[35] = torch.tensor([0.6, 0.8, 0.0, 0.0]), torch.tensor([0.0, 0.0, -0.8, 0.6])     # dot exactly 0
    rot[12] = nrm(rot[12])
    rot[36] = -nrm(rot[12] + 0.1 * rot[40])                                                          # clearly < 0
    rot[37] = nrm(rot[37])
    rot[13] = nrm(rot[37] + 0.2 * rot[41])                                                           # clearly > 0
    rot[14] = nrm(-rot[37] + 0.3 * rot[42])                                                          # < 0, same parent
    entries = [(20, 20, 0.7),                                               # a root: its own parent
               (0, 30, 0.0), (1, 30, 1.0), (2, 30, 0.375), (3, 31, 0.0), (4, 31, 0.5),
               (10, 34, 0.6), (11, 35, 0.25), (12, 36, 0.45), (13, 37, 0.8), (14, 37, 0.3),
               (5, 38, 1.0), (6, 38, 0.9), (7, 38, 0.2), (8, 39, 0.65), (9, 39, 0.0)]
    for r, p, _ in entries:                     # the random pairs: away from a dot of 0 (no flip within rounding)
        if r < 10 and abs(float(torch.dot(rot[r], rot[p]))) < 0.2:
            rot[r] = nrm(rot[r] + (2.0 if r % 2 else -2.0) * rot[p])
    full = dict(full, rotation=rot.contiguous())
    dots = {r: float(torch.dot(rot[r], rot[p])) for r, p, _ in entries if r != p}
    assert dots[10] == 0.0 and dots[11] == 0.0
    assert all(abs(d) > 0.1 for r, d in dots.items() if r not in (10, 11)) and dots[12] < 0 < dots[13] and dots[14] < 0
    return full, entries


def lod_case(R, name):
    import gaussian_hierarchy._C as gh
    from hgs import hierarchy, synth
    from oracle import lod_oracle as lo
    cam = synth.make_camera(W, H)
    gc, _ = synth.upstream_grads(H, W, seed=41)
    pipe = types.SimpleNamespace(**_PIPE)
    deg = 1 if name == "cut_deg1" else 3
    M = (deg + 1) ** 2
    sky = 24 if name == "cut_skybox" else 0
    base = 50 + 10 * LOD_CASES.index(name)          # (another scene, hence another cut, per case)
    for seed in range(base, base + 10):
        c0 = len(R.rec.cuts)
        if name == "edges":
            full, entries = _edge_entries(_scene_full(synth.make_scene(48, cam, seed=seed)))
            G, n = 48, len(entries)
            ri = torch.tensor([e[0] for e in entries], dtype=torch.int32)
            pi = torch.zeros(G, dtype=torch.int32)
            pi[:n] = torch.tensor([e[1] for e in entries], dtype=torch.int32)
            w = torch.zeros(G)
            w[:n] = torch.tensor([e[2] for e in entries])
            kids = torch.zeros(G, dtype=torch.int32)
            kids[:n] = torch.tensor([1 if r == p else sum(e[1] == p for e in entries) for r, p, _ in entries],
                                    dtype=torch.int32)
        else:
            h = hierarchy.build_hierarchy(synth.make_scene(420, cam, seed=seed))
            full = dict(xyz=h.xyz, scaling=torch.exp(h.log_scales), rotation=torch.nn.functional.normalize(h.rots),
                        opacity=h.alpha.abs(), features=h.shs[:, :M].contiguous())
            if sky:
                s = synth.make_scene(sky, cam, seed=seed + 1000, sh_degree=deg, s_px=(6.0, 20.0), z_range=(25.0, 40.0))
                full = {k: torch.cat((full[k], v)).contiguous() for k, v in _scene_full(s).items()}
            G = full["xyz"].shape[0]
            for tau_px in (4.0, 3.0, 2.0, 1.5, 1.0, 0.5, 0.0):
                tau = (2 * (tau_px + 0.5)) * cam.tanfovx / (0.5 * W)            # render_hierarchy.py:55-56
                if len(lo.expand_to_size(h.nodes.numpy(), h.boxes.numpy(), tau, cam.camera_center.numpy())[0]) > 300:
                    break
            # the cut and weights calls as train_post.py:91-113 makes them (capacity: all rows of the model)
            ri_buf, pi, ni_buf = (torch.zeros(G, dtype=torch.int32) for _ in range(3))
            w, kids = torch.zeros(G), torch.zeros(G, dtype=torch.int32)
            n = gh.expand_to_size(h.nodes, h.boxes, tau, cam.camera_center, torch.zeros((3)), ri_buf, pi, ni_buf)
            ri = ri_buf[:n].int()
            gh.get_interpolation_weights(ni_buf[:n], tau, h.nodes, h.boxes, cam.camera_center.cpu(), torch.zeros((3)),
                                         w, kids)
            assert n > 300 and int(((w[:n] > 0) & (w[:n] < 1)).sum()) >= 20, (name, n)
        drawn = set(ri.tolist())
        assert not drawn & {p for r, p in zip(ri.tolist(), pi[:n].tolist()) if p != r}, "a drawn row is a parent"
        model = LeafModel(full, deg, skybox_points=sky)
        w_in, kids_in = w.clone(), kids.clone()
        i0 = len(R.rec.ops)
        pkg = R.glue.render_post(_viewpoint(cam), model, pipe, torch.zeros(3), render_indices=ri, parent_indices=pi,
                                 interpolation_weights=w, num_node_kids=kids)
        (pkg["render"] * gc).sum().backward()
        rec = R.rec.ops[i0]
        assert rec["site"] == 1 and rec["args"]["means3D"].shape[0] == n + sky
        if rec["fragile"] != 0:                     # knife-edge pixels: the leaf gradients would be ambiguous
            continue
        out = R.rec.arrays(ops=[i0], cuts=range(c0, len(R.rec.cuts)), knn=[])
        out.update({"lod0__op": np.asarray(0, np.int64), "lod0__skybox": np.asarray(sky, np.int64),
                    "lod0__render_indices": ri.numpy(), "lod0__parent_indices": pi.numpy(),
                    "lod0__weights": w_in.numpy(), "lod0__kids": kids_in.numpy(),
                    "lod0__viewspace_grad": pkg["viewspace_points"].grad.numpy()})
        for k in FULL:
            out[f"lod0__full__{k}"] = full[k].detach().numpy()
            out[f"lod0__leafgrad__{k}"] = model.leaves[k].grad.numpy()
        if sky:
            assert int((rec["out"]["radii"][n:] > 0).sum()) > 0, "the skybox must be on screen"
        return out
    raise RuntimeError(f"{name}: every seed put a pixel on a knife edge")


def _take(z, kind, i, j):
    """Record ``<kind><i>`` of a recorder file, renamed ``<kind><j>``."""
    return {f"{kind}{j}__{k.split('__', 1)[1]}": v for k, v in z.items() if k.split("__")[0] == f"{kind}{i}"}


def _count(z, kind):
    return len({k.split("__")[0] for k in z if k.startswith(kind)})


def build_chain(ref, tmp):
    """{"boundary_chain.npz": arrays}: the reference's three scripts, unmodified, chained on the synthetic COLMAP scene
    of tests/harness/make_scene.py with the recorder on (HGS_RECORD of tests/harness/run_reference_script.py):
    train_single.py (densify-and-prune every 2nd iteration,
    opacities fast enough that it prunes) -> hierarchy of the trained chunk (tests/harness/ply_to_hier.py)
    -> train_post.py -> render_hierarchy.py at tau 0 and 15.  Kept: the first render (active SH degree 0, 16 stored
    coefficients), the first render after densification changed P, the first and the last render_post of train_post.py
    with their cut / weights calls (train_post.py:91-113), the first view of render_hierarchy.py at tau 0 and at tau 15
    with theirs (render_hierarchy.py:58-80), and the initial distCUDA2 (scene/gaussian_model.py:190).  Training on the
    oracle depends on the BLAS build, so these are not expected to regenerate bit for bit elsewhere."""
    import subprocess
    from harness import make_scene, ply_to_hier
    n_views = 4
    scene, out = os.path.join(tmp, "scene"), os.path.join(tmp, "chunk")
    make_scene.make(scene, n_points=240, n_views=n_views, W=W, H=H, radius=1.5, look_at_depth=5.5, hier=False)

    def run(script, *args):
        rec = os.path.join(tmp, script.replace(".py", ".npz"))
        cp = subprocess.run([sys.executable, os.path.join(TESTS, "harness", "run_reference_script.py"), "--backend", "cpu",
                             script, *args], env=dict(os.environ, HGS_RECORD=rec, HGS_REFERENCE=ref),
                            capture_output=True, text=True, timeout=3000)
        assert cp.returncode == 0 and os.path.isfile(rec), f"{script}:\n{cp.stdout[-2000:]}\n{cp.stderr[-4000:]}"
        with np.load(rec, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}

    single = run("train_single.py", "-s", scene, "--model_path", out, "--iterations", "6", "--disable_viewer", "-r", "1",
                 "--skip_scale_big_gauss", "--densify_from_iter", "1", "--densification_interval", "2",
                 "--densify_grad_threshold", "1e-7", "--opacity_lr", "1.0")
    rows = [single[f"op{i}__arg__means3D"].shape[0] for i in range(_count(single, "op"))]
    changed = next(i for i, r in enumerate(rows) if r != rows[0])
    hier = os.path.join(out, "hierarchy.hier")
    ply_to_hier.hier_from_ply(os.path.join(out, "point_cloud", "iteration_6", "point_cloud.ply"), hier)
    post = run("train_post.py", "-s", scene, "--model_path", out, "--hierarchy", hier, "--iterations", "3",
               "--disable_viewer", "-r", "1")
    last = _count(post, "op") - 1
    rh = run("render_hierarchy.py", "-s", scene, "--model_path", out, "--hierarchy", hier + "_opt", "--out_dir",
             os.path.join(tmp, "renders"), "--taus", "0", "15", "-r", "1")
    assert _count(rh, "op") == 2 * n_views and _count(rh, "cut") == 2 * n_views
    assert _count(post, "cut") == _count(post, "op")
    arrs = {}
    for j, (z, i) in enumerate(((single, 0), (single, changed), (post, 0), (post, last), (rh, 0), (rh, n_views))):
        arrs.update(_take(z, "op", i, j))
    for j, (z, i) in enumerate(((post, 0), (post, last), (rh, 0), (rh, n_views))):
        arrs.update(_take(z, "cut", i, j))
    arrs.update(_take(single, "knn", 0, 0))
    assert int(arrs["op0__set__sh_degree"]) == 0 and arrs["op0__arg__shs"].shape[1] == 16
    assert [int(arrs[f"op{j}__site"]) for j in range(6)] == [0, 0, 1, 1, 1, 1]
    return {"boundary_chain.npz": arrs}


def build(ref):
    """{file name: {key: array}} of the direct-call fixtures."""
    files = {}
    with reference(ref) as R:
        files["boundary_direct.npz"] = direct(R)
        for name in LOD_CASES:
            files[f"boundary_lod_{name}.npz"] = lod_case(R, name)
    for arrs in files.values():
        for k, v in arrs.items():
            assert v.dtype != object, k
    return files


def main():
    import tempfile
    ref = os.environ["HGS_REFERENCE"]
    files = build(ref)
    with tempfile.TemporaryDirectory() as tmp:
        files.update(build_chain(ref, tmp))
    total = 0
    for name, arrs in files.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        total += size
        print(f"{name}: {size} bytes, {len(arrs)} arrays")
        assert size <= MAX_FILE, name
    print(f"total {total} bytes")
    assert total <= MAX_TOTAL


if __name__ == "__main__":
    main()
