"""Generates tests/golden/ref_step_golden.npz by running the REFERENCE's own train_single.py and train_post.py, UNMODIFIED,
for a few iterations on the CPU harness (tests/harness/run_reference_script.py's CudaToCpu mode over the stand-ins of
tests/harness/cpu_backends.py, a synthetic scene of tests/harness/make_scene.py), with a locked skybox so that the
gradient-lock lines run, and with ``anchors`` for train_post.py.  Run in the build container:

    HGS_REFERENCE=<checkout> python tests/golden/make_step_golden.py

Nothing of the reference is edited; two calls are wrapped.  ``Tensor.backward``: right after it returns, the BEFORE
state of one case is taken -- the six parameters, their gradients, Adam moments and step, max_radii2D /
xyz_gradient_accum / denom, and the calling frame's ``radii``, ``visibility_filter`` and
``viewspace_point_tensor.grad``.  ``GaussianModel.update_learning_rate``: the next iteration's call takes the AFTER
state.  Everything between the two is the block hgs.step replaces (train_single.py:144-186, train_post.py:164-192).

Stored per case (numbers only): both states, the learning rates of the step, the lock configuration and the clamp
threshold.  The maker asserts that every case has visible and invisible rows and locked rows with non-zero raw
gradients, that the train_single.py cases have clamped and unclamped rows, and that every row is at least 1e-4
(relative) away from the clamp threshold before and after the step.
"""
import os
import runpy
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["HGS_REFERENCE"]
sys.path[:0] = [REF, os.path.join(ROOT, "tests", "shims"), os.path.join(ROOT, "hierarchical-3d-gaussians_amd"), ROOT,
                os.path.join(ROOT, "tests")]

from harness import cpu_backends, make_scene            # noqa: E402
from harness import run_reference_script as rrs         # noqa: E402

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
             rotation="_rotation")
SKYBOX = 24
MIN_DISTANCE = 1e-4
RADIUS = 40.0                      # of the camera ellipse: sets cameras_extent, hence the clamp threshold
ITERATIONS = 3                     # 2 complete iterations per script: the last one returns before its optimizer step

cases = []                         # dicts of numpy arrays, in the order they were taken
pending = {}


def np_(t):
    return t.detach().clone().numpy()


def snapshot(g, prefix, out):
    for n in NAMES:
        p = getattr(g, ATTRS[n])
        out[f"{prefix}.{n}"] = np_(p)
        st = g.optimizer.state.get(p, {})
        if "exp_avg" in st:
            out[f"{prefix}.{n}.exp_avg"], out[f"{prefix}.{n}.exp_avg_sq"] = np_(st["exp_avg"]), np_(st["exp_avg_sq"])
            out[f"{prefix}.{n}.step"] = np.array(float(st["step"]))
        else:
            out[f"{prefix}.{n}.exp_avg"] = out[f"{prefix}.{n}.exp_avg_sq"] = np.zeros_like(out[f"{prefix}.{n}"])
            out[f"{prefix}.{n}.step"] = np.array(0.0)
    out[f"{prefix}.max_radii2D"] = np_(g.max_radii2D)
    if getattr(g, "xyz_gradient_accum", None) is not None and g.xyz_gradient_accum.numel():
        out[f"{prefix}.accum"], out[f"{prefix}.denom"] = np_(g.xyz_gradient_accum), np_(g.denom)


def install_wrappers(GaussianModel):
    real_backward = torch.Tensor.backward
    real_ulr = GaussianModel.update_learning_rate

    def backward(self, *a, **k):
        real_backward(self, *a, **k)
        f = sys._getframe(1).f_locals
        g = f.get("gaussians")
        if g is None or "viewspace_point_tensor" not in f or g._xyz.grad is None:
            return
        c = {"script": os.path.basename(sys.argv[0]), "iteration": int(f["iteration"])}
        snapshot(g, "before", c)
        for n in NAMES:
            c[f"grad.{n}"] = np_(getattr(g, ATTRS[n]).grad)
            c[f"lr.{n}"] = np.array(float(next(gr["lr"] for gr in g.optimizer.param_groups if gr["name"] == n)))
        c["radii"] = np_(f["radii"]).astype(np.int32)
        vf = f["visibility_filter"]
        c["visible"] = np_(vf.nonzero().flatten() if vf.dtype == torch.bool else vf).astype(np.int64)
        c["means2D_grad"] = np_(f["viewspace_point_tensor"].grad)
        c["skybox_points"] = np.array(int(g.skybox_points))
        c["anchors"] = np_(g.anchors).astype(np.int64) if getattr(g, "anchors", None) is not None else np.zeros(0, np.int64)
        if c["script"] == "train_single.py":
            c["clamp_threshold"] = np.array(float(f["scene"].cameras_extent) * 0.02)
            assert g.scaffold_points is None
        pending["case"] = c

    def update_learning_rate(self, iteration):
        c = pending.pop("case", None)
        if c is not None:
            snapshot(self, "after", c)
            cases.append(c)
        return real_ulr(self, iteration)

    torch.Tensor.backward = backward
    GaussianModel.update_learning_rate = update_learning_rate

    def restore():
        torch.Tensor.backward = real_backward
        GaussianModel.update_learning_rate = real_ulr
    return restore


def run(script, *args):
    argv = sys.argv
    sys.argv = [os.path.join(REF, script)] + list(args)
    try:
        with rrs.CudaToCpu():
            runpy.run_path(os.path.join(REF, script), run_name="__main__")
    except SystemExit as e:
        assert not e.code, e
    finally:
        sys.argv = argv
        pending.clear()               # the last iteration returns before its optimizer step


def degree1_scaffold(src, dst):
    """create_from_hier reads its skybox from a scaffold saved with SH degree 1 (train_coarse.py's output): the chunk
    train_single.py just saved, with the first nine f_rest columns kept."""
    from plyfile import PlyData, PlyElement
    el = PlyData.read(os.path.join(src, "point_cloud.ply")).elements[0].data
    keep = [n for n in el.dtype.names if not n.startswith("f_rest_") or int(n[len("f_rest_"):]) < 9]
    cut = np.empty(len(el), dtype=[(n, el.dtype[n]) for n in keep])
    for n in keep:
        cut[n] = el[n]
    os.makedirs(dst)
    PlyData([PlyElement.describe(cut, "vertex")]).write(os.path.join(dst, "point_cloud.ply"))
    with open(os.path.join(src, "pc_info.txt")) as f, open(os.path.join(dst, "pc_info.txt"), "w") as g:
        g.write(f.read())
    return dst


def rel_distance(scaling, thr):
    m = np.exp(scaling.astype(np.float64)).max(axis=1)
    return np.abs(m - thr) / thr


def check_case(c, name):
    P = c["before.xyz"].shape[0]
    vis = np.zeros(P, bool)
    vis[c["visible"]] = True
    assert vis.any() and not vis.all(), (name, int(vis.sum()), P)
    locked = np.zeros(P, bool)
    sky = int(c["skybox_points"])
    if c["script"] == "train_single.py":
        locked[:sky] = True
    else:
        locked[P - sky:] = True
        locked[c["anchors"]] = True
        assert c["anchors"].size > 0
    assert sky > 0 and any(np.abs(c[f"grad.{n}"][locked]).max() > 0 for n in NAMES), name
    info = f"{name}: P {P}, visible {int(vis.sum())}, locked {int(locked.sum())}"
    if "clamp_threshold" in c:
        thr = float(np.float32(c["clamp_threshold"]))
        d = min(rel_distance(c["before.scaling"], thr).min(), rel_distance(c["after.scaling"], thr).min())
        changed = (c["after.scaling"] != c["before.scaling"]).any(axis=1)
        big = np.exp(c["after.scaling"].astype(np.float64)).max(axis=1) * (1 / 0.8) > thr
        n_clamped = int((changed & locked).sum())       # locked rows change by the clamp alone
        assert d >= MIN_DISTANCE, (name, d)
        assert n_clamped >= 1 and int((~big).sum()) >= 1, (name, n_clamped, thr, np.quantile(np.exp(c["before.scaling"]).max(axis=1), [0, 0.25, 0.5, 0.75, 1]))
        info += f", clamp threshold {thr:.6g}, locked rows clamped {n_clamped}, distance {d:.2e}"
    print(info)


def main():
    cpu_backends.install()
    torch.cuda.Event = rrs._Event
    torch.cuda.max_memory_allocated = lambda *a, **k: 0
    torch.cuda.empty_cache = lambda: None
    torch.cuda.set_device = lambda *a, **k: None
    torch.cuda.synchronize = lambda *a, **k: None
    # the deprecated torch.range (render_post's skybox rows) does not pass through the torch-function mode
    real_range = torch.range
    torch.range = lambda *a, **k: real_range(*a, **dict(k, device="cpu"))
    with rrs.CudaToCpu():
        from scene.gaussian_model import GaussianModel
    restore = install_wrappers(GaussianModel)
    torch.manual_seed(0)
    np.random.seed(0)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            scene = os.path.join(tmp, "scene")
            hier = make_scene.make(scene, n_points=160, radius=RADIUS, look_at_depth=5.5)
            out = os.path.join(tmp, "chunk")
            run("train_single.py", "-s", scene, "--model_path", out, "--iterations", str(ITERATIONS), "--disable_viewer",
                "-r", "1", "--skybox_num", str(SKYBOX), "--skybox_locked")
            n_single = len(cases)
            hier_in = os.path.join(out, "hierarchy.hier")
            os.replace(hier, hier_in)
            anchors = np.arange(3, 160, 7, dtype=np.int32)
            with open(os.path.join(out, "anchors.bin"), "wb") as f:
                f.write(int(anchors.size).to_bytes(4, "little"))
                f.write(anchors.tobytes())
            scaffold = degree1_scaffold(os.path.join(out, "point_cloud", f"iteration_{ITERATIONS}"), os.path.join(tmp, "scaffold"))
            run("train_post.py", "-s", scene, "--model_path", out, "--hierarchy", hier_in, "--iterations", str(ITERATIONS),
                "--disable_viewer", "-r", "1", "--scaffold_file", scaffold, "--skybox_locked")
    finally:
        restore()
    assert n_single == ITERATIONS - 1 and len(cases) == 2 * (ITERATIONS - 1), (n_single, len(cases))
    arrays = {}
    names = []
    for c in cases:
        name = f"{c['script'][len('train_'):-len('.py')]}_{c['iteration']}"
        names.append(name)
        check_case(c, name)
        for k, v in c.items():
            if k not in ("script", "iteration"):
                arrays[f"{name}.{k}"] = v
    arrays["case_names"] = np.array(names)
    path = os.path.join(HERE, "ref_step_golden.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
