"""Float64 statement of the contribution statistics, folded from the CPU oracle's own
per-pixel rows: for every Gaussian the largest blending weight ``w = alpha * T_before`` it reaches at a counted pixel,
the sum of those weights and the number of counted pixels it is blended at.

The oracle runs with ``colors_precomp`` (no SH evaluation is needed for the weights) and ``positive_power="clamp"`` (what
the HIP kernels do), keeps every tile's blended sets (``return_keep``) and every pixel's ``PixelRow`` (``capture``)."""
from dataclasses import dataclass

import numpy as np
import torch

import parity as pa


@dataclass
class SpecView:
    out: object                # the OracleOut (fragile, final_T, geom, binning, ...)
    run: object                # the OracleRun (leaves: colors_precomp, ...)
    W: int
    H: int
    P: int
    pix: list                  # per tile with a list: (flat pixels [npx], ids [n], w [npx, n] float64, keep [npx, n])


def oracle_view(scene, cam, bg=None, colors_precomp=None, **kw) -> SpecView:
    """One oracle forward of ``scene`` with every pixel captured; ``w`` of every (pixel, list entry) in float64."""
    bg = torch.zeros(3) if bg is None else bg
    W, H = cam.image_width, cam.image_height
    if colors_precomp is None:
        colors_precomp = torch.full((scene.P, 3), 0.5, dtype=torch.float64)     # (float64: so is its gradient)
    run = pa.oracle_run(scene, cam, bg, colors_precomp=colors_precomp, positive_power="clamp", **kw)
    out = run(return_keep=True, capture=range(H * W))
    pix = []
    for t, keep in out.keep.items():
        flat = np.asarray(pa.tile_pixels(t, W, H), dtype=np.int64)
        rows = [out.rows[int(f)] for f in flat]
        ids = np.asarray(rows[0].ids, dtype=np.int64)
        a = np.stack([r.alpha for r in rows]).astype(np.float64) * keep
        T_after = np.cumprod(1.0 - a, axis=1)
        T_before = np.concatenate([np.ones((a.shape[0], 1)), T_after[:, :-1]], axis=1)
        pix.append((flat, ids, a * T_before, keep.astype(bool)))
    return SpecView(out=out, run=run, W=W, H=H, P=scene.P, pix=pix)


def fold(view: SpecView, pixel_mask=None, slot_of_row=None, n_slots=None, into=None):
    """(wmax float64 [S], wsum float64 [S], count int64 [S]) of one view under ``pixel_mask`` (bool / uint8 [H*W] or
    [H,W], default all) and ``slot_of_row`` (int [P], default identity; negative or >= n_slots: ignored), accumulated
    into ``into`` (the same triple) when given."""
    S = view.P if n_slots is None else int(n_slots)
    wmax, wsum, count = into if into is not None else (np.zeros(S), np.zeros(S), np.zeros(S, dtype=np.int64))
    m = np.ones(view.W * view.H, dtype=bool) if pixel_mask is None else np.asarray(pixel_mask).reshape(-1) != 0
    slot = np.arange(view.P, dtype=np.int64) if slot_of_row is None else np.asarray(slot_of_row, dtype=np.int64)
    for flat, ids, w, keep in view.pix:
        sel = m[flat]
        if not sel.any():
            continue
        w, keep = w[sel], keep[sel]
        s = slot[ids]
        ok = (s >= 0) & (s < S) & keep.any(axis=0)
        if not ok.any():
            continue
        # a row appears once per tile list, the slots are distinct: plain indexed updates
        np.maximum.at(wmax, s[ok], (w * keep).max(axis=0)[ok])
        np.add.at(wsum, s[ok], w.sum(axis=0)[ok])
        np.add.at(count, s[ok], keep.sum(axis=0)[ok])
    return wmax, wsum, count


def autograd_wsum(view: SpecView, pixel_mask=None):
    """d(sum over the counted pixels of image channel 0) / d colors_precomp[:, 0]: the oracle's own autograd says what
    ``wsum`` is (the identity row is the only map this form has)."""
    m = torch.ones(view.H, view.W, dtype=torch.float64) if pixel_mask is None else \
        torch.as_tensor(np.asarray(pixel_mask).reshape(view.H, view.W) != 0, dtype=torch.float64)
    leaf = view.run.leaves["colors_precomp"]
    leaf.grad = None
    (view.out.color[0] * m).sum().backward(retain_graph=True)
    return leaf.grad[:, 0].detach().numpy().copy()
