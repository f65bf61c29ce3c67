"""Adaptive density control on the GPU: the reference's ``GaussianModel.densify_and_prune``
(scene/gaussian_model.py:528-685, called from train_single.py:150-151) as one stream compaction -- a plan launch that
decides every row's class and rank, one host wait for the four totals, and apply launches that write every output row
of the six parameter tensors and their twelve Adam moment tensors once (``csrc/densify.hip``; one launch for all of
them at tensor level, one per parameter group at model level so that each group's old tensors can be released).

    import hgs.densify
    hgs.densify.install(GaussianModel)        # binds the method densify_and_prune(max_grad, min_opacity, extent)

or ``hgs.densify.densify_and_prune(gaussians, max_grad, min_opacity, extent, noise=..., generator=...)``.

The rule is the reference's (include/hgs.h states it); what differs on purpose: the noise of the split children is an
ARGUMENT (``noise`` [2S,3] standard normal samples, or drawn with ``generator`` after the plan), so the result does not
depend on the process's RNG stream position; ``torch.cuda.empty_cache()`` is not called; max_grad <= 0 is refused.
GPU only, float32 only; there is no torch fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch import nn

from . import _lib

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
_ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
              rotation="_rotation")
_TAIL = dict(xyz=(3,), f_dc=(1, 3), opacity=(1,), scaling=(3,), rotation=(4,))
_KIND = dict(xyz=_lib.DENSIFY_XYZ, scaling=_lib.DENSIFY_SCALING)

_totals_host = {}       # device index -> (ctypes int64[4] over pinned, device-mapped memory, address)


def _fail(msg):
    raise ValueError("hgs.densify: " + msg)


def _check_tensor(name, t, P=None, shape_tail=None):
    if not isinstance(t, torch.Tensor):
        _fail(f"{name} must be a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        _fail(f"{name} is on {t.device}; a GPU tensor is needed (no CPU fallback)")
    if t.dtype != torch.float32:
        _fail(f"{name} has dtype {t.dtype}; only float32 is supported")
    if not t.is_contiguous():
        _fail(f"{name} is not contiguous")
    if P is not None and (t.dim() < 1 or t.shape[0] != P):
        _fail(f"{name} has shape {tuple(t.shape)}; {P} rows expected")
    if shape_tail is not None and tuple(t.shape[1:]) != tuple(shape_tail):
        _fail(f"{name} has shape {tuple(t.shape)}; (P,{','.join(map(str, shape_tail))}) expected")


def _validate(tensors, moments, accum, radii, F, max_grad, min_opacity, d, noise):
    if not isinstance(tensors, dict) or set(tensors) != set(NAMES):
        _fail(f"tensors must be a dict with the keys {NAMES}")
    moments = moments or {}
    if not set(moments) <= set(NAMES):
        _fail(f"moments has unknown keys {sorted(set(moments) - set(NAMES))}")
    _check_tensor("xyz", tensors["xyz"])
    if tensors["xyz"].dim() != 2:
        _fail(f"xyz has shape {tuple(tensors['xyz'].shape)}; (P,3) expected")
    P = tensors["xyz"].shape[0]
    dev = tensors["xyz"].device
    for n in NAMES:
        t = tensors[n]
        if n == "f_rest":
            _check_tensor(n, t, P)
            if t.dim() != 3 or t.shape[2] != 3:
                _fail(f"f_rest has shape {tuple(t.shape)}; (P,K,3) expected")
        else:
            _check_tensor(n, t, P, _TAIL[n])
        mv = moments.get(n)
        if mv is not None:
            if not isinstance(mv, (tuple, list)) or len(mv) != 2:
                _fail(f"moments[{n!r}] must be (exp_avg, exp_avg_sq) or None")
            for what, m in zip(("exp_avg", "exp_avg_sq"), mv):
                _check_tensor(f"{n}.{what}", m)
                if m.shape != t.shape:
                    _fail(f"{n}.{what} has shape {tuple(m.shape)}; the parameter has {tuple(t.shape)}")
    _check_tensor("accum", accum, P)
    _check_tensor("radii", radii, P)
    if accum.numel() != P or radii.numel() != P:
        _fail(f"accum / radii must hold one value per row ({P}), got {tuple(accum.shape)} / {tuple(radii.shape)}")
    every = [tensors[n] for n in NAMES] + [m for mv in moments.values() if mv is not None for m in mv] + [accum, radii]
    if any(t.device != dev for t in every):
        _fail("all tensors must live on one device")
    F = 0 if F is None else F
    if not isinstance(F, int) or isinstance(F, bool) or not 0 <= F <= P:
        _fail(f"F (protected leading rows) must be an integer in [0, {P}], got {F!r}")
    for what, x in (("max_grad", max_grad), ("min_opacity", min_opacity), ("d", d)):
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            _fail(f"{what} must be a number, got {x!r}")
    if not (max_grad > 0 and math.isfinite(max_grad)):
        _fail(f"max_grad must be positive and finite, got {max_grad!r}")
    if math.isnan(min_opacity) or math.isnan(d):
        _fail("min_opacity / d is NaN")
    if noise is not None:
        _check_tensor("noise", noise)
        if noise.dim() != 2 or noise.shape[1] != 3 or noise.shape[0] % 2:
            _fail(f"noise has shape {tuple(noise.shape)}; (2S,3) expected")
        if noise.device != dev:
            _fail("noise must live on the device of the parameters")
    return P, F, dev, moments


def _totals_buffer(index):
    if index not in _totals_host:
        p = _lib.lib().hgs_host_alloc(4 * 8)
        if not p:
            raise RuntimeError("cannot allocate pinned host memory for the densification totals")
        _totals_host[index] = ((C.c_int64 * 4).from_address(p), p)
    return _totals_host[index]


class _Plan:
    """The plan of one call: classes and ranks of the P source rows in ``tmp`` on the device, the four totals on the
    host.  ``apply(names)`` builds the outputs of those tensors (one launch per <= ADAM_MAX_TENSORS of them)."""

    def __init__(self, tensors, moments, accum, radii, F, max_grad, min_opacity, d, noise, generator):
        self.P, F, self.dev, self.moments = _validate(tensors, moments, accum, radii, F, max_grad, min_opacity, d, noise)
        self.tensors = dict(tensors)
        # xyz's children read the SOURCE scaling and rotation: they outlive their own groups' release
        self.scaling, self.rotation = tensors["scaling"], tensors["rotation"]
        l = self.l = _lib.lib()
        dev = self.dev
        self.index = dev.index if dev.index is not None else torch.cuda.current_device()
        self.stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        tmp_bytes = l.hgs_densify_tmp_bytes(self.P)
        if tmp_bytes == 0:
            raise _lib.HgsError(f"hgs_densify_tmp_bytes: {l.hgs_last_error().decode()}", 1)
        self.tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
        host, host_addr = _totals_buffer(self.index)
        _lib.check(l.hgs_densify_plan(_lib.ptr(accum), _lib.ptr(radii), _lib.ptr(tensors["opacity"]),
                                      _lib.ptr(tensors["scaling"]), self.P, F, max_grad, min_opacity, d,
                                      _lib.ptr(self.tmp), C.c_void_p(host_addr), 1, self.stream, self.index),
                   "hgs_densify_plan")
        self.totals = tuple(int(host[i]) for i in range(4))
        n_orig, n_clone, S, n_kept = self.totals
        if noise is None:
            noise = torch.randn((2 * S, 3), generator=generator, device=dev, dtype=torch.float32)
        elif noise.shape[0] != 2 * S:
            _fail(f"noise has shape {tuple(noise.shape)}; {S} rows split, so ({2 * S},3) is expected")
        self.noise = noise
        self.P_new = n_orig + n_clone + 2 * n_kept

    def apply(self, names):
        out, out_m, descs = {}, {}, []
        for n in names:
            t = self.tensors[n]
            out[n] = torch.empty((self.P_new,) + tuple(t.shape[1:]), dtype=torch.float32, device=self.dev)
            mv = self.moments.get(n)
            out_m[n] = None if mv is None else (torch.empty_like(out[n]), torch.empty_like(out[n]))
            row_len = int(math.prod(t.shape[1:]))
            if row_len == 0:            # f_rest of zero width (K = 0): nothing to launch on
                continue
            descs.append(_lib.DensifyTensor(
                src=t.data_ptr(), exp_avg=None if mv is None else mv[0].data_ptr(),
                exp_avg_sq=None if mv is None else mv[1].data_ptr(), dst=out[n].data_ptr(),
                dst_exp_avg=None if mv is None else out_m[n][0].data_ptr(),
                dst_exp_avg_sq=None if mv is None else out_m[n][1].data_ptr(), row_len=row_len,
                kind=_KIND.get(n, _lib.DENSIFY_COPY)))
        if self.P and self.P_new:
            tot = (C.c_int64 * 4)(*self.totals)
            for i in range(0, len(descs), _lib.ADAM_MAX_TENSORS):
                chunk = descs[i:i + _lib.ADAM_MAX_TENSORS]
                arr = (_lib.DensifyTensor * len(chunk))(*chunk)
                _lib.check(self.l.hgs_densify_apply(arr, len(chunk), self.P, tot, _lib.ptr(self.scaling),
                                                    _lib.ptr(self.rotation), _lib.ptr(self.noise) if self.totals[2] else None,
                                                    _lib.ptr(self.tmp), self.stream, self.index), "hgs_densify_apply")
        return out, out_m

    def release(self, name):
        """Drop the plan's references to a source tensor and its moments (scaling and rotation stay until the end)."""
        self.tensors.pop(name, None)
        self.moments.pop(name, None)


def densify_and_prune_tensors(tensors, moments, accum, radii, F, max_grad, min_opacity, d, noise=None, generator=None):
    """tensors: dict xyz [P,3], f_dc [P,1,3], f_rest [P,K,3], opacity [P,1], scaling [P,3], rotation [P,4] (raw);
    moments: dict name -> (exp_avg, exp_avg_sq) or None (a missing name: no moments); accum [P,1] or [P], radii [P];
    F: protected leading rows (None = 0); d = percent_dense * extent; noise: [2S,3] standard normal samples (None: drawn
    with ``generator`` after the plan).  -> (new tensors, new moments, (kept originals, kept clones, split rows S, kept
    split rows)).  The inputs are not modified."""
    plan = _Plan(tensors, moments, accum, radii, F, max_grad, min_opacity, d, noise, generator)
    out, out_m = plan.apply(NAMES)
    return out, out_m, plan.totals


# the order in which the model's groups are rebuilt and released: the widest first, while every other source is still
# alive (the peak above the inputs is then f_rest's outputs, 3K of 14 + 3K floats per row, not the outputs of
# everything); xyz before scaling and rotation, whose source rows its children read
_ORDER = ("f_rest", "f_dc", "opacity", "xyz", "scaling", "rotation")


def densify_and_prune(gaussians, max_grad, min_opacity, extent, *, noise=None, generator=None):
    """The reference's ``GaussianModel.densify_and_prune(max_grad, min_opacity, extent)`` on a model of its shape (duck
    typed: _xyz .. _rotation, optimizer.param_groups named xyz .. rotation with one parameter each,
    xyz_gradient_accum, denom, max_radii2D, percent_dense, scaffold_points).  Every argument is checked, the plan is
    made and the noise is fixed before anything is touched: a ``ValueError`` leaves model and optimizer exactly as they
    were.  Then the groups are rebuilt and switched over one by one, each one's old tensors released as soon as its new
    ones exist (as the reference's ``cat_tensors_to_optimizer`` / ``_prune_optimizer`` walk the groups): only a failed
    allocation or launch can interrupt that walk.  Returns the four totals."""
    groups = {}
    for group in gaussians.optimizer.param_groups:
        if group.get("name") in NAMES:
            if len(group["params"]) != 1:
                _fail(f"param group {group['name']!r} holds {len(group['params'])} parameters; one expected")
            groups[group["name"]] = group
    if set(groups) != set(NAMES):
        _fail(f"the optimizer needs one param group per name of {NAMES}; found {sorted(groups)}")
    tensors, moments = {}, {}
    state = gaussians.optimizer.state
    for n in NAMES:
        p = groups[n]["params"][0]
        if p is not getattr(gaussians, _ATTRS[n]):
            _fail(f"param group {n!r} does not hold the model's {_ATTRS[n]}")
        tensors[n] = p.data
        st = state.get(p, None)
        moments[n] = (st["exp_avg"], st["exp_avg_sq"]) if st is not None and "exp_avg" in st else None
    if isinstance(extent, bool) or not isinstance(extent, (int, float)):
        _fail(f"extent must be a number, got {extent!r}")
    plan = _Plan(tensors, moments, gaussians.xyz_gradient_accum, gaussians.max_radii2D, gaussians.scaffold_points,
                 max_grad, min_opacity, gaussians.percent_dense * extent, noise, generator)
    del tensors, moments
    dev, P_new = plan.dev, plan.P_new
    for n in _ORDER:
        out, out_m = plan.apply((n,))
        new = nn.Parameter(out[n].requires_grad_(True))
        old = groups[n]["params"][0]
        st = state.get(old, None)
        if st is not None:
            if out_m[n] is not None:
                st["exp_avg"], st["exp_avg_sq"] = out_m[n]
            del state[old]
            state[new] = st
        groups[n]["params"][0] = new
        setattr(gaussians, _ATTRS[n], new)
        plan.release(n)
        del old, st, out, out_m, new
    gaussians.xyz_gradient_accum = torch.zeros((P_new, 1), device=dev)
    gaussians.denom = torch.zeros((P_new, 1), device=dev)
    gaussians.max_radii2D = torch.zeros((P_new,), device=dev)
    return plan.totals


def install(model_class):
    """Bind the fused pass as ``model_class.densify_and_prune`` (the reference's GaussianModel): the one-line opt-in of
    train_single.py, like ``hgs.optim`` and ``hgs.loss``."""
    def method(self, max_grad, min_opacity, extent, *, noise=None, generator=None):
        return densify_and_prune(self, max_grad, min_opacity, extent, noise=noise, generator=generator)
    method.__name__ = "densify_and_prune"
    method.__doc__ = densify_and_prune.__doc__
    model_class.densify_and_prune = method
    return model_class
