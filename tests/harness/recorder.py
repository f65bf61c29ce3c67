"""Recorder of the calls the reference's own code makes across this repository's drop-in boundary, while that code runs
on the oracle-backed CPU stand-ins (tests/harness/cpu_backends.py).  TEST INFRASTRUCTURE ONLY.

What is recorded, by ``detach().clone()`` so that the run is not perturbed:
  * every ``GaussianRasterizer`` call: the 17 settings fields as they arrive, the eight call arguments as they are
    passed (``None`` and empty tensors included), the op's outputs, the upstream gradients that reach them and the
    gradients the op returns for its inputs (``means2D`` included), the call site in gaussian_renderer/__init__.py
    and the oracle's count of knife-edge ("fragile") pixels;
  * every ``expand_to_size`` / ``get_interpolation_weights`` call: arguments, capacity of the output tensors, outputs;
  * every ``distCUDA2`` call: input points and output.

``install()`` wraps whatever the drop-in packages hold at that moment (call it after ``cpu_backends.install()``),
``uninstall()`` puts it back; ``arrays()`` flattens what was recorded into the key schema of
tests/golden/make_boundary_golden.py.  tests/harness/run_reference_script.py ``--backend cpu`` turns it on when
HGS_RECORD names an output file."""
import inspect
import sys

import numpy as np
import torch

SETTINGS = ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
            "sh_degree", "campos", "prefiltered", "debug", "render_indices", "parent_indices", "interpolation_weights",
            "num_node_kids", "do_depth")
ARGS = ("means3D", "means2D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")
SITES = ("render", "render_post", "render_coarse")          # gaussian_renderer/__init__.py:20, :138, :296
LOD_FIELDS = ("render_indices", "parent_indices", "interpolation_weights", "num_node_kids")
# order of the tuple the extension layer's backward returns (diff_gaussian_rasterization/__init__.py:191)
_BWD = ("means2D", "colors_precomp", "opacities", "means3D", "cov3D_precomp", "shs", "scales", "rotations")


def _snap(v):
    return v.detach().clone() if torch.is_tensor(v) else v


def _site():
    f = sys._getframe(2)
    while f is not None:
        if f.f_code.co_name in SITES and f.f_code.co_filename.replace("\\", "/").endswith("gaussian_renderer/__init__.py"):
            return SITES.index(f.f_code.co_name)
        f = f.f_back
    return -1


class _Proxy:
    """The extension module with two entry points replaced (everything else delegates)."""

    def __init__(self, inner, **over):
        self.__dict__.update(over)
        self._inner = inner

    def __getattr__(self, k):
        return getattr(self._inner, k)


class Recorder:
    def __init__(self):
        self.ops, self.cuts, self.weights, self.knn = [], [], [], []
        self._pending = None
        self._saved = None

    def install(self):
        import diff_gaussian_rasterization as dgr
        import gaussian_hierarchy._C as gh
        import simple_knn._C as knn
        rec = self
        C = dgr._C
        self._saved = (C, dgr.GaussianRasterizer.forward, gh.expand_to_size, gh.get_interpolation_weights,
                       knn.distCUDA2)
        c_fwd, c_bwd = C.rasterize_gaussians, C.rasterize_gaussians_backward

        def fwd(*a, **k):
            res = c_fwd(*a, **k)
            call, r = res[-1], rec._pending
            if r is not None:
                call._hgs_record = r
                out = getattr(call, "out", None)
                if out is not None and getattr(out, "fragile", None) is not None:
                    r["fragile"] = int(np.asarray(out.fragile).sum())
            return res

        def bwd(call, color, invdepth, dL_dcolor, dL_dinvdepth, *a, **k):
            g = c_bwd(call, color, invdepth, dL_dcolor, dL_dinvdepth, *a, **k)
            r = getattr(call, "_hgs_record", None)
            if r is not None:
                r["grad_in"] = dict(color=_snap(dL_dcolor), invdepth=_snap(dL_dinvdepth))
                r["grad_out"] = {n: _snap(t) for n, t in zip(_BWD, g) if t is not None}
            return g

        dgr._C = _Proxy(C, rasterize_gaussians=fwd, rasterize_gaussians_backward=bwd)
        orig = dgr.GaussianRasterizer.forward
        sig = inspect.signature(orig)

        def forward(mod, *a, **k):
            ba = sig.bind(mod, *a, **k)
            ba.apply_defaults()
            rs = mod.raster_settings
            r = dict(site=_site(), settings={f: _snap(getattr(rs, f)) for f in SETTINGS},
                     args={n: _snap(ba.arguments[n]) for n in ARGS})
            rec._pending = r
            try:
                out = orig(*ba.args, **ba.kwargs)
            finally:
                rec._pending = None
            r["out"] = dict(color=_snap(out[0]), radii=_snap(out[1]), invdepth=_snap(out[2]))
            rec.ops.append(r)
            return out

        dgr.GaussianRasterizer.forward = forward
        e_fn, w_fn, k_fn = gh.expand_to_size, gh.get_interpolation_weights, knn.distCUDA2

        def expand_to_size(nodes, boxes, size, viewpoint, viewdir, render_indices, parent_indices, nodes_for_render):
            r = dict(nodes=_snap(nodes), boxes=_snap(boxes), size=float(size), viewpoint=_snap(viewpoint),
                     viewdir=_snap(viewdir), capacity=np.array([render_indices.numel(), parent_indices.numel(),
                                                                nodes_for_render.numel()], np.int64))
            n = e_fn(nodes, boxes, size, viewpoint, viewdir, render_indices, parent_indices, nodes_for_render)
            r.update(count=int(n), render_indices=_snap(render_indices[:n]), parent_indices=_snap(parent_indices[:n]),
                     nodes_for_render_indices=_snap(nodes_for_render[:n]))
            rec.cuts.append(r)
            return n

        def get_interpolation_weights(node_indices, size, nodes, boxes, viewpoint, viewdir, weights, kids):
            r = dict(node_indices=_snap(node_indices), size=float(size), viewpoint=_snap(viewpoint),
                     capacity=np.array([weights.numel(), kids.numel()], np.int64))
            res = w_fn(node_indices, size, nodes, boxes, viewpoint, viewdir, weights, kids)
            n = node_indices.numel()
            r.update(weights=_snap(weights[:n]), kids=_snap(kids[:n]))
            rec.weights.append(r)
            # paired with the cut whose nodes it weighs (the scripts call it right after expand_to_size)
            cut = rec.cuts[-1] if rec.cuts else None
            if cut is not None and "weights" not in cut and torch.equal(
                    cut["nodes_for_render_indices"].cpu(), r["node_indices"].cpu().to(cut["nodes_for_render_indices"].dtype)):
                cut["weights"] = r
            return res

        def distCUDA2(points):
            out = k_fn(points)
            rec.knn.append(dict(points=_snap(points), dist=_snap(out)))
            return out

        gh.expand_to_size, gh.get_interpolation_weights, knn.distCUDA2 = expand_to_size, get_interpolation_weights, \
            distCUDA2
        return self

    def uninstall(self):
        import diff_gaussian_rasterization as dgr
        import gaussian_hierarchy._C as gh
        import simple_knn._C as knn
        if self._saved is not None:
            dgr._C, dgr.GaussianRasterizer.forward, gh.expand_to_size, gh.get_interpolation_weights, knn.distCUDA2 = \
                self._saved
            self._saved = None

    def arrays(self, ops=None, cuts=None, knn=None):
        """{key: numpy array} of the selected records (indices into ops / cuts / knn; None = all, cuts: every cut that
        was followed by its weights call) in the key schema of tests/golden/make_boundary_golden.py.  A cut record is an
        ``expand_to_size`` call together with the ``get_interpolation_weights`` call on its nodes that followed it."""
        out = {}
        ops = range(len(self.ops)) if ops is None else ops
        cuts = [i for i, c in enumerate(self.cuts) if "weights" in c] if cuts is None else cuts
        knn = range(len(self.knn)) if knn is None else knn
        for j, i in enumerate(ops):
            out.update(op_arrays(f"op{j}", self.ops[i]))
        for j, i in enumerate(cuts):
            out.update(cut_arrays(f"cut{j}", self.cuts[i], self.cuts[i]["weights"]))
        for j, i in enumerate(knn):
            out[f"knn{j}__points"] = _np(self.knn[i]["points"])
            out[f"knn{j}__dist"] = _np(self.knn[i]["dist"])
        return out


def _np(v):
    if torch.is_tensor(v):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def op_arrays(pre, r):
    out = {f"{pre}__site": np.asarray(r["site"], np.int64), f"{pre}__fragile": np.asarray(r.get("fragile", -1), np.int64)}
    for f, v in r["settings"].items():
        out[f"{pre}__set__{f}"] = _np(v)
    for n, v in r["args"].items():
        if v is not None:
            out[f"{pre}__arg__{n}"] = _np(v)
    for n, v in r["out"].items():
        out[f"{pre}__out__{n}"] = _np(v)
    for n, v in r.get("grad_in", {}).items():
        if v is not None:
            out[f"{pre}__gin__{n}"] = _np(v)
    for n, v in r.get("grad_out", {}).items():
        out[f"{pre}__gout__{n}"] = _np(v)
    return out


def cut_arrays(pre, e, w):
    out = {f"{pre}__nodes": _np(e["nodes"]), f"{pre}__boxes": _np(e["boxes"]),
           f"{pre}__size": np.asarray(e["size"], np.float64), f"{pre}__viewpoint": _np(e["viewpoint"]),
           f"{pre}__viewdir": _np(e["viewdir"]), f"{pre}__capacity": e["capacity"],
           f"{pre}__count": np.asarray(e["count"], np.int64)}
    for k in ("render_indices", "parent_indices", "nodes_for_render_indices"):
        out[f"{pre}__{k}"] = _np(e[k])
    assert np.array_equal(_np(w["node_indices"]), out[f"{pre}__nodes_for_render_indices"]), "weights of another cut"
    out[f"{pre}__w_size"] = np.asarray(w["size"], np.float64)
    out[f"{pre}__w_viewpoint"] = _np(w["viewpoint"])
    out[f"{pre}__w_capacity"] = w["capacity"]
    out[f"{pre}__weights"] = _np(w["weights"])
    out[f"{pre}__kids"] = _np(w["kids"])
    return out
