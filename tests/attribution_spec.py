"""Float64 statement of the image attribution, folded from the CPU oracle's own per-pixel
rows through ``contribution_spec.oracle_view``: for every Gaussian and channel ``A[i, c] = sum_p w_i(p) f_c(p)`` over the
counted pixels at which the row is blended, ``w = alpha * T_before``; beside it the same fold of ``|f|`` (the scale an
error bound on a signed image needs) and the weights' own sum."""
import numpy as np
import torch

from contribution_spec import oracle_view  # noqa: F401  (the one oracle forward both specs are folded from)


def fold_image(view, image, pixel_mask=None, slot_of_row=None, n_slots=None):
    """(A float64 [S, C], Aabs float64 [S, C], wsum float64 [S]) of one view: ``image`` [C, H, W] (or [H, W]) under
    ``pixel_mask`` (bool / uint8 [H*W] or [H, W], default all) and ``slot_of_row`` (int [P], default identity; negative
    or >= n_slots: ignored).  The image is SELECTED, not multiplied: its values at pixels that are not counted or at
    which a row is not blended never enter a sum, whatever they are."""
    f = np.asarray(image, dtype=np.float64)
    f = f.reshape(-1, view.H * view.W) if f.ndim == 3 else f.reshape(1, view.H * view.W)
    C = f.shape[0]
    S = view.P if n_slots is None else int(n_slots)
    A, Aabs, wsum = np.zeros((S, C)), np.zeros((S, C)), np.zeros(S)
    m = np.ones(view.W * view.H, dtype=bool) if pixel_mask is None else np.asarray(pixel_mask).reshape(-1) != 0
    slot = np.arange(view.P, dtype=np.int64) if slot_of_row is None else np.asarray(slot_of_row, dtype=np.int64)
    for flat, ids, w, keep in view.pix:
        sel = m[flat]
        if not sel.any():
            continue
        w, keep, fp = w[sel], keep[sel], f[:, flat[sel]]
        s = slot[ids]
        ok = (s >= 0) & (s < S) & keep.any(axis=0)
        for j in np.nonzero(ok)[0]:
            k = keep[:, j]
            wk, fk = w[k, j], fp[:, k]
            A[s[j]] += (fk * wk).sum(axis=1)            # (row by row: a channel's sum does not depend on the others)
            Aabs[s[j]] += (np.abs(fk) * wk).sum(axis=1)
            wsum[s[j]] += wk.sum()
    return A, Aabs, wsum


def autograd_attribution(view, image, pixel_mask=None):
    """d(sum_c sum over the counted pixels of f_c(p) color_c(p)) / d colors_precomp, [P, 3]: the oracle's own autograd
    says what ``A`` is for a three-channel image (identity slots)."""
    f = torch.as_tensor(np.asarray(image, dtype=np.float64)).reshape(3, view.H, view.W)
    if pixel_mask is not None:
        f = f * torch.as_tensor(np.asarray(pixel_mask).reshape(view.H, view.W) != 0, dtype=torch.float64)
    leaf = view.run.leaves["colors_precomp"]
    leaf.grad = None
    (view.out.color * f).sum().backward(retain_graph=True)
    return leaf.grad.detach().numpy().copy()
