"""Float64 statement of the value painting, folded from ``contribution_spec.oracle_view``: per
pixel p the rows the oracle blended, front to back, with their weights ``w_k = alpha_k * T_{k-1}`` and the transmittance
``T_n`` behind the last of them,

    out[p, c]  = sum_k (w * keep)[p, k] * v[slot(ids[k]), c] + T_n * bg[c]
    wsum[p]    = sum over the NAMED rows (those whose slot lies in [0, n_slots)) of (w * keep)[p, k]
    Aabs[p, c] = the same sum as ``out`` over |v| (and |bg|): the size of the terms, which the bound of the GPU test is
                 relative to -- signed values cancel in ``out``.

A row the map ignores still occludes (its weight stays in T) and adds nothing.  A pixel of a tile without a list shows
the background."""
import numpy as np


def fold_values(view, values, slot_of_row=None, n_slots=None, background=None):
    """-> (out [H*W, C], wsum [H*W], Aabs [H*W, C]) in float64.  ``values``: [S, C] (or [S]); ``slot_of_row``: int [P],
    default the identity; ``n_slots``: default S; ``background``: C values, default zeros."""
    v = np.asarray(values, dtype=np.float64)
    v = v.reshape(-1, 1) if v.ndim == 1 else v
    S, C = v.shape
    n_slots = S if n_slots is None else int(n_slots)
    slot = np.arange(view.P, dtype=np.int64) if slot_of_row is None else np.asarray(slot_of_row, dtype=np.int64)
    bg = np.zeros(C) if background is None else np.asarray(background, dtype=np.float64).reshape(C)
    HW = view.W * view.H
    out = np.tile(bg, (HW, 1))                     # T = 1 where no row is blended
    aabs = np.tile(np.abs(bg), (HW, 1))
    wsum = np.zeros(HW)
    for flat, ids, w, keep in view.pix:
        wk = w * keep
        s = slot[ids]
        named = (s >= 0) & (s < n_slots)
        rows = np.where(named[:, None], v[np.clip(s, 0, S - 1)], 0.0)          # [n, C]; an ignored row: zeros
        T_n = 1.0 - wk.sum(axis=1)
        out[flat] = wk @ rows + T_n[:, None] * bg[None, :]
        aabs[flat] = wk @ np.abs(rows) + T_n[:, None] * np.abs(bg)[None, :]
        wsum[flat] = wk[:, named].sum(axis=1)
    return out, wsum, aabs
