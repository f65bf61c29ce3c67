"""The yardstick of hgs.step (test infrastructure; the product never imports it): the bookkeeping between
``loss.backward()`` and the next render stated in whole-array torch ops, device- and dtype-generic (float32 on the GPU,
where it is the reference's call shape and the opponent of scripts/bench_step.py; float64 on the CPU, where
tests/golden/ref_step_golden.npz pins it to the reference's own scripts).  Written from the rule of include/hgs.h /
DESIGN.md section 7 f-10.

    1. statistics: for every visible row r: max_radii2D[r] = max(max_radii2D[r], radius); accum[r] = max(|g[r,:2]|,
       accum[r]); denom[r] += 1
    2. step: rows < lock_head, >= P - lock_tail or in lock_mask take gradient 0 in the tensors of lock_names; the rows
       whose (effective) opacity gradient is != 0 -- all rows if there is none, or with select="all" -- take Adam
    3. clamp: rows >= protect_head with max_k exp(scaling) > threshold: scaling = log(exp(scaling) * 0.8)
"""
import math

import torch

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def statistics(max_radii2D, accum, denom, means2D_grad, radii, indices=None, visible=None):
    """In place.  radii: raw [n] (rendered row i is model row indices[i], or i) or compacted [m] with visible [m]."""
    if visible is None:
        sub = radii > 0
        rows = sub.nonzero().flatten() if indices is None else indices.long()[sub]
        radii = radii[sub]
    else:
        rows = visible.long()
    max_radii2D[rows] = torch.max(max_radii2D[rows], radii.to(max_radii2D.dtype))
    if accum is not None:
        norm = torch.sqrt((means2D_grad[rows, :2] ** 2).sum(dim=-1, keepdim=True)).to(accum.dtype)
        accum[rows] = torch.max(norm, accum[rows].reshape(-1, 1)).reshape(accum[rows].shape)
        denom[rows] += 1
    return rows


def locked_rows(P, lock_head=0, lock_tail=0, lock_mask=None, device="cpu"):
    r = torch.arange(P, device=device)
    locked = (r < lock_head) | (r >= P - lock_tail)
    if lock_mask is not None:
        locked |= lock_mask.bool()
    return locked


def zero_locked(grads, locked, lock_names=NAMES):
    """In place: the torch lock zeroing (train_single.py:163-168, train_post.py:169-181)."""
    rows = locked.nonzero().flatten()
    for n in lock_names:
        grads[n][rows] = 0


def relevant_rows(opacity_grad):
    """train_single.py:171-172."""
    return (opacity_grad.flatten() != 0).nonzero().flatten().long()


def adam_rows(p, g, m, v, rows, lr, step, betas=(0.9, 0.999), eps=1e-15):
    """In place, in the dtype of the tensors: torch's _single_tensor_adam on the listed rows (None: all)."""
    b1, b2 = betas
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    sel = slice(None) if rows is None else rows
    gg = g[sel]
    mm = m[sel] * b1 + (1 - b1) * gg
    vv = v[sel] * b2 + (1 - b2) * gg * gg
    m[sel], v[sel] = mm, vv
    p[sel] = p[sel] - (lr / bc1) * (mm / (vv.sqrt() / math.sqrt(bc2) + eps))


def clamp_rows(scaling, threshold, protect_head=0):
    """The boolean [P] mask of the rows the clamp acts on (train_single.py:182-185)."""
    P = scaling.shape[0]
    big = torch.exp(scaling).max(dim=1).values > threshold if P else torch.zeros(0, dtype=torch.bool, device=scaling.device)
    big[:protect_head] = False
    return big


def clamp(scaling, threshold, protect_head=0):
    """In place; -> the mask."""
    big = clamp_rows(scaling, threshold, protect_head)
    scaling[big] = torch.log(torch.exp(scaling[big]) * 0.8)
    return big


def post_backward_spec(params, grads, *, optimizer=None, state=None, lrs=None, betas=(0.9, 0.999), eps=1e-15,
                       radii=None, indices=None, visible=None, means2D_grad=None, max_radii2D=None, accum=None,
                       denom=None, select="opacity_grad", lock_head=0, lock_tail=0, lock_mask=None, lock_names=NAMES,
                       clamp_args=None):
    """params: dict name -> tensor (updated in place); grads: dict name -> tensor (locked rows are zeroed in place) or
    None (no step).  The step is either ``optimizer.step(relevant)`` of an hgs.optim.Adam whose parameters carry
    ``grads`` as .grad (the float32 call shape of the reference), or the restatement ``adam_rows`` on ``state``: dict
    name -> [exp_avg, exp_avg_sq, step] (step is incremented) with ``lrs``: dict name -> lr.
    -> dict(relevant=rows or None, clamped=mask or None)."""
    out = dict(relevant=None, clamped=None)
    P = params["xyz"].shape[0]
    dev = params["xyz"].device
    if radii is not None:
        statistics(max_radii2D, accum, denom, means2D_grad, radii, indices, visible)
    if grads is not None:
        locked = locked_rows(P, lock_head, lock_tail, lock_mask, dev)
        zero_locked(grads, locked, lock_names)
        relevant = relevant_rows(grads["opacity"]) if select == "opacity_grad" else torch.empty(0, dtype=torch.int64, device=dev)
        out["relevant"] = relevant
        if optimizer is not None:
            optimizer.step(relevant)
            optimizer.zero_grad(set_to_none=True)
        else:
            for n in NAMES:
                st = state[n]
                st[2] += 1
                adam_rows(params[n], grads[n], st[0], st[1], relevant if relevant.numel() else None, lrs[n], st[2],
                          betas, eps)
    if clamp_args is not None:
        out["clamped"] = clamp(params["scaling"], clamp_args[0], clamp_args[1] or 0)
    return out
