"""The bookkeeping between ``loss.backward()`` and the next render on the GPU: the
densification statistics, the gradient locks, ``relevant = (opacity.grad != 0).nonzero()``, the optimizer step and the
big-Gaussian scale clamp of train_single.py:144-186, train_post.py:164-192 and train_coarse.py:110-145 as two HIP
launches (``csrc/train_step.hip``) with no device-to-host wait, instead of about twenty torch launches and four waits.

    import hgs.step
    hgs.step.install(GaussianModel)           # binds the method post_backward(...)
    gaussians.post_backward(radii=radii, visible=visibility_filter, viewspace_points=viewspace_point_tensor,
                            lock_head=gaussians.skybox_points, clamp=(0.02 * extent, gaussians.scaffold_points))

or ``hgs.step.post_backward_tensors(params, optimizer, ...)`` on the six tensors.  include/hgs.h states the rule.  The
optimizer must be an ``hgs.optim.Adam``; its state layout is not changed, so ``hgs.densify`` keeps working on it.
GPU only, float32 only; there is no torch fallback.

Not reproduced, on purpose: the [k,2] ``relevant`` of train_coarse.py:133 (express the coarse configuration as
``lock_names=("scaling",), lock_head=skybox_points, clamp=(0.1 * extent, skybox_points)``), the exposure optimizer
(12 floats per camera, stays torch), ``reset_opacity``, and the zeroed slices of the ``.grad`` tensors themselves.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .optim import Adam

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
_ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
              rotation="_rotation")
SELECT = ("opacity_grad", "all")


def _fail(msg):
    raise ValueError("hgs.step: " + msg)


def _check(name, t, dtype, dev=None, rows=None, contiguous=True):
    if not isinstance(t, torch.Tensor):
        _fail(f"{name} must be a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        _fail(f"{name} is on {t.device}; a GPU tensor is needed (no CPU fallback)")
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if t.dtype not in dtypes:
        _fail(f"{name} has dtype {t.dtype}; {' or '.join(str(d) for d in dtypes)} expected")
    if contiguous and not t.is_contiguous():
        _fail(f"{name} is not contiguous")
    if dev is not None and t.device != dev:
        _fail(f"{name} is on {t.device}; the parameters are on {dev}")
    if rows is not None and (t.dim() < 1 or t.shape[0] != rows):
        _fail(f"{name} has shape {tuple(t.shape)}; {rows} rows expected")


def _int(name, x, lo, hi):
    if isinstance(x, bool) or not isinstance(x, int) or not lo <= x <= hi:
        _fail(f"{name} must be an integer in [{lo}, {hi}], got {x!r}")
    return x


def row_mask(P, rows, device=None):
    """A ``lock_mask`` [P] uint8 with the listed rows set (``anchors`` of train_post.py:176-181): build it once."""
    if not isinstance(rows, torch.Tensor):
        rows = torch.as_tensor(rows, dtype=torch.int64, device=device)
    mask = torch.zeros(_int("P", P, 0, 2 ** 31 - 1), dtype=torch.uint8, device=rows.device if device is None else device)
    if rows.numel():
        mask[rows.reshape(-1).to(device=mask.device, dtype=torch.int64)] = 1
    return mask


def _validate(params, optimizer, radii, indices, visible, means2D_grad, max_radii2D, accum, denom, select, lock_head,
              lock_tail, lock_mask, lock_names, clamp, optimize):
    if not isinstance(params, dict) or set(params) != set(NAMES):
        _fail(f"params must be a dict with the keys {NAMES}")
    if not isinstance(optimizer, Adam):
        _fail(f"the optimizer must be an hgs.optim.Adam, got {type(optimizer).__name__}")
    _check("xyz", params["xyz"], torch.float32)
    P, dev = params["xyz"].shape[0] if params["xyz"].dim() else _fail("xyz has no rows"), params["xyz"].device
    owned = {id(p) for g in optimizer.param_groups for p in g["params"]}
    for n in NAMES:
        _check(n, params[n], torch.float32, dev, P)
    for n, width in (("xyz", 3), ("opacity", 1), ("scaling", 3), ("rotation", 4)):
        if params[n].numel() != P * width:
            _fail(f"{n} has shape {tuple(params[n].shape)}; {width} floats per row expected")
    for n in NAMES:
        if id(params[n]) not in owned:
            _fail(f"{n} is not a parameter of the optimizer")
    if select not in SELECT:
        _fail(f"select must be one of {SELECT}, got {select!r}")
    lock_names = tuple(lock_names)
    if not set(lock_names) <= set(NAMES):
        _fail(f"lock_names has unknown names {sorted(set(lock_names) - set(NAMES))}")
    _int("lock_head", lock_head, 0, P)
    _int("lock_tail", lock_tail, 0, P)
    if lock_head + lock_tail > P:
        _fail(f"lock_head {lock_head} + lock_tail {lock_tail} exceed {P} rows")
    if lock_mask is not None:
        _check("lock_mask", lock_mask, (torch.bool, torch.uint8), dev, P)
        if lock_mask.dim() != 1:
            _fail(f"lock_mask has shape {tuple(lock_mask.shape)}; ({P},) expected")
    thr = None
    if clamp is not None:
        if not isinstance(clamp, (tuple, list)) or len(clamp) != 2:
            _fail("clamp must be None or (threshold, protect_head)")
        thr, head = clamp
        if isinstance(thr, bool) or not isinstance(thr, (int, float)) or not (thr > 0 and math.isfinite(thr)):
            _fail(f"the clamp threshold must be positive and finite, got {thr!r}")
        if float(thr) > 3.4028234663852886e38 or C.c_float(thr).value <= 0.0:
            _fail(f"the clamp threshold {thr!r} is not a positive finite float32")
        clamp = (float(thr), _int("clamp's protect_head", 0 if head is None else head, 0, P))
    # statistics
    stats = any(t is not None for t in (radii, indices, visible, max_radii2D, accum, denom))
    if stats:
        if radii is None:
            _fail("statistics need radii: raw [n] (with optional indices) or compacted [m] with visible")
        if indices is not None and visible is not None:
            _fail("pass raw radii with indices, or compacted radii with visible, not both forms")
        _check("radii", radii, torch.int32, dev)
        if radii.dim() != 1:
            _fail(f"radii has shape {tuple(radii.shape)}; one dimension expected")
        n = radii.shape[0]
        if visible is not None:
            _check("visible", visible, torch.int64, dev, n)
            if visible.dim() != 1:
                _fail(f"visible has shape {tuple(visible.shape)}; ({n},) expected")
        elif indices is not None:
            _check("indices", indices, torch.int32, dev, n)
            if indices.dim() != 1:
                _fail(f"indices has shape {tuple(indices.shape)}; ({n},) expected")
        elif n != P:
            _fail(f"radii has {n} rows; {P} expected without indices or visible")
        if max_radii2D is None:
            _fail("statistics need max_radii2D")
        _check("max_radii2D", max_radii2D, torch.float32, dev, P)
        if max_radii2D.numel() != P:
            _fail(f"max_radii2D has shape {tuple(max_radii2D.shape)}; one value per row expected")
        if (accum is None) != (denom is None):
            _fail("accum and denom come together")
        if accum is not None:
            for what, t in (("accum", accum), ("denom", denom)):
                _check(what, t, torch.float32, dev, P)
                if t.numel() != P:
                    _fail(f"{what} has shape {tuple(t.shape)}; one value per row expected")
            if means2D_grad is None:
                _fail("accum needs means2D_grad (the gradient of the screen-space means, [P,3])")
            _check("means2D_grad", means2D_grad, torch.float32, dev, P)
            if means2D_grad.dim() != 2 or means2D_grad.shape[1] != 3:
                _fail(f"means2D_grad has shape {tuple(means2D_grad.shape)}; ({P},3) expected")
    # gradients: all or none
    step = False
    if optimize:
        have = [params[n].grad is not None for n in NAMES]
        if any(have) and not all(have):
            _fail("some parameters have a gradient and some have none")
        step = all(have)
        if step:
            for n in NAMES:
                g = params[n].grad
                if g.is_sparse or not g.is_cuda or g.dtype != torch.float32 or g.shape != params[n].shape:
                    _fail(f"the gradient of {n} must be a dense float32 GPU tensor of the parameter's shape")
    return P, dev, lock_names, clamp, stats, step


@torch.no_grad()
def post_backward_tensors(params, optimizer, *, radii=None, indices=None, visible=None, means2D_grad=None,
                          max_radii2D=None, accum=None, denom=None, select="opacity_grad", lock_head=0, lock_tail=0,
                          lock_mask=None, lock_names=NAMES, clamp=None, optimize=True):
    """params: dict xyz [P,3], f_dc [P,1,3], f_rest [P,K,3], opacity [P,1], scaling [P,3], rotation [P,4] -- the
    parameters of ``optimizer`` (an ``hgs.optim.Adam``), with their gradients.  Statistics (if any of radii / visible /
    max_radii2D is given): raw ``radii`` [n] int32 with optional ``indices`` [n] int32, or ``visible`` [m] int64 with
    compacted ``radii`` [m]; ``max_radii2D`` [P]; ``accum`` / ``denom`` [P,1] with ``means2D_grad`` [P,3].  Optimizer
    step (if ``optimize`` and the parameters have gradients): rows ``< lock_head``, ``>= P - lock_tail`` or set in
    ``lock_mask`` take gradient 0 in the tensors of ``lock_names``; ``select``: "opacity_grad" (rows whose effective
    opacity gradient is non-zero; all rows if there is none) or "all"; afterwards every ``.grad`` is None.  ``clamp``:
    None or (threshold, protect_head).  Everything is checked before anything is touched: a ``ValueError`` leaves
    parameters, optimizer and statistics as they were.  Nothing waits for the device."""
    P, dev, lock_names, clamp, stats, step = _validate(params, optimizer, radii, indices, visible, means2D_grad,
                                                       max_radii2D, accum, denom, select, lock_head, lock_tail,
                                                       lock_mask, lock_names, clamp, optimize)
    if not (stats or step or clamp is not None):
        return
    l = _lib.lib()
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    descs, keep, opacity_grad = [], [], None
    if step:
        by_ptr = {params[n].data_ptr(): n for n in NAMES if params[n].numel()}
        for rows, _, t, grad in optimizer._collect([params[n] for n in NAMES]):
            n = by_ptr.get(t.param)
            if n is None:               # zero-width f_rest (K = 0): stepped, nothing to launch on
                continue
            flags = (_lib.STEP_LOCKABLE if n in lock_names else 0) | (_lib.STEP_SCALING if n == "scaling" else 0)
            descs.append(_lib.StepTensor(adam=t, flags=flags))
            keep.append(grad)
            if n == "opacity":
                opacity_grad = grad
    elif clamp is not None:
        descs.append(_lib.StepTensor(adam=_lib.AdamTensor(param=params["scaling"].data_ptr(), row_len=3),
                                     flags=_lib.STEP_SCALING))
    if P == 0:
        if step:
            for n in NAMES:
                params[n].grad = None
        return
    if lock_mask is not None and lock_mask.dtype == torch.bool:
        lock_mask = lock_mask.view(torch.uint8)
    a = _lib.StepArgs(P=P, n=radii.shape[0] if stats else 0, radii=_lib.ptr(radii) if stats else None,
                      indices=_lib.ptr(indices), visible=_lib.ptr(visible), means2D_grad=_lib.ptr(means2D_grad),
                      max_radii2D=_lib.ptr(max_radii2D), accum=_lib.ptr(accum), denom=_lib.ptr(denom),
                      opacity_grad=_lib.ptr(opacity_grad), lock_mask=_lib.ptr(lock_mask), lock_head=lock_head,
                      lock_tail=lock_tail, protect_head=clamp[1] if clamp else 0,
                      select_all=1 if select == "all" else 0, lock_opacity=1 if "opacity" in lock_names else 0,
                      clamp=1 if clamp else 0, clamp_threshold=clamp[0] if clamp else 0.0)
    tmp_bytes = l.hgs_step_tmp_bytes(P)
    if tmp_bytes == 0:
        raise _lib.HgsError(f"hgs_step_tmp_bytes: {l.hgs_last_error().decode()}", 1)
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
    _lib.check(l.hgs_step_select(C.byref(a), _lib.ptr(tmp), stream, index), "hgs_step_select")
    for i in range(0, len(descs), _lib.ADAM_MAX_TENSORS):
        chunk = descs[i:i + _lib.ADAM_MAX_TENSORS]
        arr = (_lib.StepTensor * len(chunk))(*chunk)
        _lib.check(l.hgs_step_apply(C.byref(a), arr, len(chunk), _lib.ptr(tmp), stream, index), "hgs_step_apply")
    if step:
        for n in NAMES:
            params[n].grad = None


def post_backward(gaussians, *, radii=None, indices=None, visible=None, viewspace_points=None, means2D_grad=None,
                  select="opacity_grad", lock_head=0, lock_tail=0, lock_mask=None, lock_names=NAMES, clamp=None,
                  optimize=True):
    """``post_backward_tensors`` on a model of the reference's shape (duck typed: _xyz .. _rotation, optimizer,
    max_radii2D, xyz_gradient_accum, denom).  Statistics are kept iff ``radii`` is given (then ``viewspace_points``, the
    tensor render() returns, or its gradient ``means2D_grad`` is needed)."""
    params = {n: getattr(gaussians, a) for n, a in _ATTRS.items()}
    if means2D_grad is None and viewspace_points is not None:
        means2D_grad = viewspace_points.grad
    stats = radii is not None or visible is not None or indices is not None
    if stats and means2D_grad is None:
        _fail("statistics need viewspace_points (with its gradient) or means2D_grad")
    return post_backward_tensors(
        params, gaussians.optimizer, radii=radii, indices=indices, visible=visible,
        means2D_grad=means2D_grad if stats else None, max_radii2D=gaussians.max_radii2D if stats else None,
        accum=gaussians.xyz_gradient_accum if stats else None, denom=gaussians.denom if stats else None, select=select,
        lock_head=lock_head, lock_tail=lock_tail, lock_mask=lock_mask, lock_names=lock_names, clamp=clamp,
        optimize=optimize)


def install(model_class):
    """Bind the fused pass as ``model_class.post_backward`` (the reference's GaussianModel), like ``hgs.densify.install``."""
    def method(self, **kw):
        return post_backward(self, **kw)
    method.__name__ = "post_backward"
    method.__doc__ = post_backward.__doc__
    model_class.post_backward = method
    return model_class
