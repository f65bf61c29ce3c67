"""Scenes whose blend decisions sit on their knife edges ON PURPOSE (tests/test_knife_edges_cpu.py, _gpu.py).

A 200 x 120 image (ragged: 12.5 x 7.5 tiles) holds
  * alpha edges: Gaussians whose opacity is solved, from the float64 oracle's exponent at one chosen target pixel,
    so that alpha there is 1/255 (1 +- 0.5 .. 3e-7) -- float32 rounding of the opacity adds 6e-8, far inside the 1e-5 band.
    Targets sit on 16 px tile edges, 8 px quadrant edges and 4 px cell edges, on the last row and column, with the
    Gaussian's centre several pixels away (across such an edge, often): isotropic, slanted (anisotropic, rotated) and
    elongated conics (a needle 8 .. 12 px by 0.5 px, the target along its axis: M in the hundreds, where the band's
    footprint term decides);
  * T edges: three stacks of two Gaussians whose alpha is capped at 0.99 over a disc of some 150 pixels each
    (T (1 - alpha) = 0.01^2 = 1e-4 up to rounding: float64 continues, float32 stops), one of them across the
    last row and column; and chains of three whose last opacity is solved so that the product lands within a few
    1e-7 of 1e-4;
  * both kinds in one pixel: alpha-edge Gaussians in front of a stack, aimed at a pixel of its capped disc.
Depth order, front to back: those combined ones, the alpha edges, the chains, the stacks.  Nothing else is live in
front of a stack's disc (candidates are redrawn until they stay clear of it).

Route variants: ``lod`` = "opacity" (interpolation_weights / num_node_kids through ``lod_opacity``, what the kernels
do) or "alpha" (the per-pixel remap, ``lod_alpha``); ``precomp`` = colours handed in.
"""
import math

import numpy as np
import torch

from hgs import synth
from oracle import raster_oracle as ro

W, H = 200, 120
STACKS = ((32.3, 63.6), (104.4, 24.3), (189.6, 111.7))      # centres (px): across a tile edge, a quadrant edge, the corner
# opacity 1.9 caps alpha where G >= 0.52 (a disc of radius 1.14 sigma) and stays below 2 x 0.99, where the oracle's
# straight-through cap araw + (0.99 - araw) is exact in float32 as well (Sterbenz): its float32 stand-in keeps 0.99
STACK_SIGMA, STACK_OPACITY, CORE_R = 6.0, 1.9, 7.0


def _edge_coords(rng, n, size):
    """Pixel coordinates on a 16 px tile edge, an 8 px quadrant edge, a 4 px cell edge or the last row / column."""
    kind = rng.integers(0, 4, n)
    base = rng.integers(0, size // 16 + 1, n) * 16
    side = rng.integers(0, 2, n)                   # the pixel before or after the boundary
    off = np.choose(kind, [np.zeros(n, int), np.full(n, 8), 4 * rng.integers(1, 4, n), np.zeros(n, int)])
    v = base + off - side
    v = np.where(kind == 3, size - 1, v)
    return np.clip(v, 0, size - 1)


def _to_world(px, py, z, cam):
    tx, ty = cam.tanfovx, cam.tanfovy
    return np.stack([((2 * px + 1) / W - 1) * z * tx, ((2 * py + 1) / H - 1) * z * ty, z], 1)


def _conic_px(s1, s2, th):
    """Approximate screen-space inverse covariance of a Gaussian with pixel sigmas s1, s2 rotated by th (+ the 0.3 blur)."""
    c, s = np.cos(th), np.sin(th)
    a = c * c * s1 ** 2 + s * s * s2 ** 2 + 0.3
    b = c * s * (s1 ** 2 - s2 ** 2)
    d = s * s * s1 ** 2 + c * c * s2 ** 2 + 0.3
    det = a * d - b * b
    return d / det, -b / det, a / det


def _core_pixels():
    ys, xs = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for cx, cy in STACKS:
        m |= (xs - cx) ** 2 + (ys - cy) ** 2 <= (CORE_R + 4.0) ** 2
    return np.stack([xs[m], ys[m]], 1).astype(np.float64)


def _solve(f, target, hi):
    """Monotone f: [0, hi] -> ..., the x with f(x) = target (float64 bisection, vectorised)."""
    lo_, hi_ = torch.zeros_like(target), torch.full_like(target, hi)
    for _ in range(80):
        mid = 0.5 * (lo_ + hi_)
        up = f(mid) < target
        lo_, hi_ = torch.where(up, mid, lo_), torch.where(up, hi_, mid)
    return 0.5 * (lo_ + hi_)


def build(seed=0, *, lod=None, precomp=False, n_alpha=330, n_chain=24, n_combo=6):
    rng = np.random.default_rng(seed)
    cam = synth.make_camera(W, H, 60.0)
    fx = W / (2 * cam.tanfovx)
    core = _core_pixels()
    rows = []          # (kind, target (x, y) or None, centre (x, y) px, z, s1 px, s2 px, theta, opacity)
    used = set()       # one aimed Gaussian per target pixel

    def clear_of_stacks(cx, cy, s1, s2, th):
        A, B, C = _conic_px(s1, s2, th)
        dx, dy = core[:, 0] - cx, core[:, 1] - cy
        return bool((-0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy).max() < -8.0)

    def place(kind, n, z_lo, z_hi, keep_clear=True):
        got = 0
        while got < n:
            tx, ty = _edge_coords(rng, 1, W)[0], _edge_coords(rng, 1, H)[0]
            shape = got % 3
            if shape == 0:                                          # isotropic
                s1 = s2 = rng.uniform(1.5, 4.0); th = 0.0
            elif shape == 1:                                        # slanted
                s1, s2, th = rng.uniform(2.5, 5.0), rng.uniform(1.0, 2.0), rng.uniform(0, math.pi)
            else:                                                   # elongated
                s1, s2, th = rng.uniform(8.0, 12.0), 0.5, rng.uniform(0, math.pi)
            if kind == "combo":
                cx0, cy0 = STACKS[got % len(STACKS)]
                ang = rng.uniform(0, 2 * math.pi)
                tx, ty = int(round(cx0 + 6 * math.cos(ang))), int(round(cy0 + 6 * math.sin(ang)))
                s1 = s2 = 1.5; th = 0.0
            r = math.sqrt(rng.uniform(3.0, 7.0))                  # exponent -1.5 .. -3.5 at the target
            phi = rng.uniform(-0.25, 0.25) if shape == 2 else rng.uniform(0, 2 * math.pi)
            u = np.array([r * s1 * math.cos(phi), r * s2 * math.sin(phi)])
            c, s = math.cos(th), math.sin(th)
            cx, cy = tx - (c * u[0] - s * u[1]), ty - (s * u[0] + c * u[1])
            if not (-8 < cx < W + 8 and -8 < cy < H + 8):
                continue
            if (tx, ty) in used or (kind != "combo" and keep_clear and not clear_of_stacks(cx, cy, s1, s2, th)):
                continue
            used.add((tx, ty))
            rows.append((kind, (int(tx), int(ty)), (cx, cy), rng.uniform(z_lo, z_hi), s1, s2, th, 0.5))
            got += 1

    place("combo", n_combo, 2.0, 2.5)
    place("alpha", n_alpha, 3.0, 6.0)
    got = 0
    while got < n_chain:                         # two near-opaque Gaussians on the target, a third solved behind them
        tx, ty = _edge_coords(rng, 1, W)[0], _edge_coords(rng, 1, H)[0]
        ok = all(clear_of_stacks(tx + dx, ty + dy, 2.5, 2.5, 0.0) for dx, dy in ((0.3, 0.0), (0.0, -0.3), (0.1, 0.1)))
        if not ok or (tx, ty) in used:
            continue
        used.add((tx, ty))
        z0 = rng.uniform(6.5, 7.0)
        rows.append(("chain0", (int(tx), int(ty)), (tx + 0.3, ty), z0, 2.5, 2.5, 0.0, 0.95))
        rows.append(("chain1", (int(tx), int(ty)), (tx, ty - 0.3), z0 + 0.05, 2.5, 2.5, 0.0, 0.95))
        rows.append(("chain2", (int(tx), int(ty)), (tx + 0.1, ty + 0.1), 7.5, 2.5, 2.5, 0.0, 0.5))
        got += 1
    for cx, cy in STACKS:
        for dz in (0.0, 0.05):
            rows.append(("stack", None, (cx, cy), 8.0 + dz, STACK_SIGMA, STACK_SIGMA, 0.0, STACK_OPACITY))

    P = len(rows)
    kind = np.array([r[0] for r in rows])
    cxy = np.array([r[2] for r in rows])
    z = np.array([r[3] for r in rows])
    means = _to_world(cxy[:, 0], cxy[:, 1], z, cam)
    s1 = np.array([r[4] for r in rows]) * z / fx
    s2 = np.array([r[5] for r in rows]) * z / fx
    th = np.array([r[6] for r in rows])
    scales = np.stack([s1, s2, s2], 1)
    rots = np.stack([np.cos(th / 2), np.zeros(P), np.zeros(P), np.sin(th / 2)], 1)
    g = torch.Generator().manual_seed(seed)
    shs = torch.randn(P, 16, 3, generator=g) * 0.25
    scene = synth.Scene(torch.tensor(means, dtype=torch.float32), torch.tensor(scales, dtype=torch.float32),
                        torch.tensor(rots, dtype=torch.float32),
                        torch.tensor([[r[7]] for r in rows], dtype=torch.float32), shs, 3)
    colors = torch.rand(P, 3, generator=g) if precomp else None
    w = kids = None
    if lod is not None:                          # the edge Gaussians in transition, everything else not (identity)
        w = torch.ones(P + 7)
        kids = torch.ones(P + 7, dtype=torch.int32)
        sel = torch.from_numpy(np.isin(kind, ("alpha", "combo")))
        w[:P][sel] = torch.rand(int(sel.sum()), generator=g) * 0.9
        kids[:P][sel] = torch.randint(2, 9, (int(sel.sum()),), generator=g, dtype=torch.int32)

    targets = np.array([r[1][1] * W + r[1][0] if r[1] is not None else -1 for r in rows])
    eff = {}

    def oracle(capture):
        with torch.no_grad():
            return ro.rasterize(scene.means3D, None, None if precomp else scene.shs, colors, scene.opacities,
                                scene.scales, scene.rotations, None, image_height=H, image_width=W,
                                tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3), scale_modifier=1.0,
                                viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=3,
                                campos=cam.camera_center, interpolation_weights=w, num_node_kids=kids,
                                lod_mode=lod or "opacity", capture=capture)

    def power_at(out, i):
        row = out.rows[int(targets[i])]
        j = np.flatnonzero(row.ids == i)
        return float(row.power[j[0]]) if len(j) else None, row, (j[0] if len(j) else None)

    # pass 1: alpha edges (the exponent does not depend on the opacity)
    edge = np.flatnonzero(np.isin(kind, ("alpha", "combo")))
    out = oracle(targets[edge])
    op = scene.opacities[:, 0].double().clone()
    sgn = rng.choice([-1.0, 1.0], P) * rng.uniform(0.5, 3.0, P) * 1e-7
    for i in edge:
        p, _, _ = power_at(out, i)
        if p is None:
            op[i] = 0.0                          # (target outside its rectangle: drop it)
            continue
        a = torch.tensor([ro.ALPHA_MIN * (1.0 + sgn[i])], dtype=torch.float64)
        G = math.exp(p)
        if lod is None:
            o = a / G
        elif lod == "opacity":
            wi, ki = w[i:i + 1].double(), kids[i:i + 1]
            o = _solve(lambda x: ro.lod_opacity(x, wi, ki), a / G, 1.0)
        else:
            wi, ki = w[i:i + 1].double(), kids[i:i + 1]
            o = _solve(lambda x: ro.lod_alpha(x, wi, ki), a, 1.0) / G
        op[i] = float(o)
    scene.opacities = op.float()[:, None].contiguous()
    # pass 2: the chains' last opacity, from the transmittance in front of it
    last = np.flatnonzero(kind == "chain2")
    out = oracle(targets[last])
    for i in last:
        p, row, j = power_at(out, i)
        T = 1.0
        for k in range(j if j is not None else 0):
            a = float(row.alpha[k])
            if row.power[k] <= 0 and a >= ro.ALPHA_MIN:
                T *= 1.0 - a
        o = (1.0 - ro.T_EPS * (1.0 + sgn[i]) / T) / math.exp(p) if p is not None and T > 0 else 0.0
        op[i] = o if 0.0 < o * math.exp(p if p is not None else 0.0) < 0.985 and o <= 1.0 else 0.3
    scene.opacities = op.float()[:, None].contiguous()
    return dict(cam=cam, scene=scene, colors_precomp=colors, interpolation_weights=w, num_node_kids=kids,
                lod_mode=lod or "opacity", kind=kind, targets=targets)
