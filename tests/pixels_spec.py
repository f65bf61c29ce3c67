"""Float64 statement of the per-pixel readout, folded from ``contribution_spec.oracle_view``:
per pixel the rows the oracle blended, front to back, their weights ``w_k = alpha_k * T_{k-1}`` and ``T_k = 1 - cumsum(w)``,
hence ``n``, the front and the back row, the heaviest row (front-most on a tie) with its weight and the runner-up's, the
median row (the first ``k`` with ``T_k < 0.5``) -- and, for the near-tie checks of the GPU tests, what the spec says
about ANY row at a pixel: its weight, and ``T`` before and after it.

The case builders stand here too (copies of those in tests/test_contribution_gpu.py: a test file is not imported)."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

import contribution_spec as cs
import parity as pa

NONE, IGNORED = -1, -2


# ---- cases -------------------------------------------------------------------------------------------------------------
def _opaque_stack():
    cam, scene, _, _ = pa.default_case(200, 40, 24, 6)
    k = torch.arange(40, dtype=torch.float32)
    scene.means3D[:40] = torch.stack([torch.zeros(40), torch.zeros(40), 3.0 + 0.01 * k], 1)
    scene.scales[:40] = 0.15
    scene.opacities[:40] = 0.9
    scene.opacities[:8] = 1.0
    return cam, scene


def _centred_row():
    """Row 0: opacity 1, in front of everything (z = 1), centred on the centre of pixel (10, 12) of a 32 x 32 image."""
    cam, scene, _, _ = pa.default_case(50, 32, 32, 4)
    ndc = lambda p, n: (2.0 * p + 1.0) / n - 1.0
    scene.means3D[0] = torch.tensor([ndc(10, 32) * cam.tanfovx, ndc(12, 32) * cam.tanfovy, 1.0])
    scene.scales[0] = 0.05
    scene.opacities[0] = 1.0
    return cam, scene


def _big_rows():
    """Three rows that cover the whole 10 x 9 tile grid."""
    cam, scene, _, _ = pa.default_case(100, 160, 144, 7)
    scene.means3D[:3] = torch.tensor([[0.0, 0.0, 6.0], [0.5, -0.3, 9.0], [-0.4, 0.2, 12.0]])
    scene.scales[:3] = torch.tensor([[2.0, 1.5, 1.0], [3.0, 3.0, 3.0], [2.5, 4.0, 1.0]])
    scene.opacities[:3] = torch.tensor([[0.3], [0.5], [0.9]])
    return cam, scene


CASES = {
    "one_tile": lambda: pa.default_case(64, 16, 16, 3)[:2],
    "edge_tiles_a": lambda: pa.default_case(300, 70, 45, 0)[:2],
    "edge_tiles_b": lambda: pa.default_case(600, 130, 50, 2)[:2],
    "long_lists": lambda: pa.default_case(4000, 64, 64, 5)[:2],
    "opaque_stack": _opaque_stack,
    "1x1": lambda: pa.default_case(30, 1, 1, 9)[:2],
    "5x3": lambda: pa.default_case(40, 5, 3, 1)[:2],
    "big_rows": _big_rows,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(cam, scene, SpecView, PixelSpec): the oracle runs once per case and is shared, unchanged, by every test."""
    cam, scene = (_centred_row if name == "centred_row" else CASES[name])()
    view = cs.oracle_view(scene, cam)
    return cam, scene, view, fold_pixels(view)


# ---- the statement -----------------------------------------------------------------------------------------------------
@dataclass
class PixelSpec:
    """Flat [H*W] arrays; ids are op rows (``map_ids`` applies a slot map), NONE where there is none."""
    W: int
    H: int
    P: int
    n: np.ndarray              # int64   rows blended
    alpha: np.ndarray          # float64 1 - T_n
    front: np.ndarray          # int64
    back: np.ndarray           # int64
    heaviest: np.ndarray       # int64   front-most row of the largest weight
    wmax: np.ndarray           # float64 that weight (0: no row)
    second: np.ndarray         # float64 the runner-up's weight (0: fewer than two rows)
    median: np.ndarray         # int64   first k with T_k < 0.5
    t_gap: np.ndarray          # float64 min over the blended k of |T_k - 0.5| (inf: no row)
    tiles: list                # per tile with a list: (flat [npx], ids [n], w [npx, n], keep [npx, n], T_after [npx, n])

    def of_row(self, rows):
        """What the spec says about row ``rows[p]`` at pixel p: (w, T_before, T_after) float64 [H*W]; NaN where the row
        is not blended at the pixel (not in the tile's list, or not kept)."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        w, tb, ta = (np.full(self.W * self.H, np.nan) for _ in range(3))
        for flat, ids, ww, keep, T_after in self.tiles:
            r = rows[flat]
            hit = r[:, None] == ids[None, :]                      # a row appears once per tile list
            hit &= keep
            has = hit.any(axis=1)
            col = hit.argmax(axis=1)
            px = np.arange(flat.size)
            w[flat[has]] = ww[px, col][has]
            ta[flat[has]] = T_after[px, col][has]
            tb[flat[has]] = (T_after[px, col] + ww[px, col])[has]
        return w, tb, ta


def fold_pixels(view) -> PixelSpec:
    HW = view.W * view.H
    n = np.zeros(HW, dtype=np.int64)
    alpha, wmax, second = np.zeros(HW), np.zeros(HW), np.zeros(HW)
    t_gap = np.full(HW, np.inf)
    front, back, heaviest, median = (np.full(HW, NONE, dtype=np.int64) for _ in range(4))
    tiles = []
    for flat, ids, w, keep in view.pix:
        npx, L = w.shape
        px = np.arange(npx)
        wk = w * keep                                             # (w is zero off the kept set already)
        T_after = 1.0 - np.cumsum(wk, axis=1)
        tiles.append((flat, ids, wk, keep, T_after))
        if L == 0:
            continue
        cnt = keep.sum(axis=1)
        has = cnt > 0
        n[flat] = cnt
        alpha[flat] = 1.0 - T_after[:, -1]
        first = keep.argmax(axis=1)
        last = L - 1 - keep[:, ::-1].argmax(axis=1)
        front[flat[has]] = ids[first[has]]
        back[flat[has]] = ids[last[has]]
        top = wk.argmax(axis=1)                                   # the first of equal maxima: the front-most
        heaviest[flat[has]] = ids[top[has]]
        wmax[flat] = wk[px, top]
        rest = wk.copy()
        rest[px, top] = 0.0
        second[flat] = rest.max(axis=1)
        below = keep & (T_after < 0.5)
        hm = below.any(axis=1)
        median[flat[hm]] = ids[below.argmax(axis=1)[hm]]
        gap = np.where(keep, np.abs(T_after - 0.5), np.inf)
        t_gap[flat] = gap.min(axis=1)
    return PixelSpec(W=view.W, H=view.H, P=view.P, n=n, alpha=alpha, front=front, back=back, heaviest=heaviest, wmax=wmax,
                     second=second, median=median, t_gap=t_gap, tiles=tiles)


def map_ids(ids, slot_of_row=None, n_slots=None):
    """Row ids -> what the call reports under a slot map: the slot when it lies in [0, n_slots), IGNORED when it does
    not, NONE kept."""
    ids = np.asarray(ids, dtype=np.int64)
    if slot_of_row is None:
        return ids.copy()
    slot = np.asarray(slot_of_row, dtype=np.int64)
    s = slot[np.clip(ids, 0, None)]
    ok = (s >= 0) & (s < (np.iinfo(np.int64).max if n_slots is None else int(n_slots)))
    return np.where(ids < 0, ids, np.where(ok, s, IGNORED))
