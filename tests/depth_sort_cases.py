"""Hand-built frames for the per-tile depth sort (csrc/binning.hip: launch_tile_depth_sort, tile_depth_sort_wave_body).

A frame is a small image and a list of (tile, n, depth pattern) entries: ``n`` Gaussians sit at the centre pixel of that
tile, each with a footprint of radius 3, so that the tile's instance list holds exactly those ``n`` and nothing else.  The
camera is ``synth.make_camera``'s default (identity view), so a Gaussian's depth is the float32 ``z`` it was given, bit for
bit.  The Gaussians of all tiles are shuffled together: ids carry no depth order.

The host rule of launch_tile_depth_sort is restated here (``route``), together with the size classes of the kernels, so
that every frame can say which kernels sort which of its tiles -- and the tests can check that the frames, taken together,
stand on every edge (``EDGES``).  The builder and the reference are numpy only; ``render`` at the end is the one function
that needs a GPU, and it imports what it needs itself.
"""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from hgs import synth

F = np.float32
TILE = 16

# ---- csrc/binning.hip, restated -------------------------------------------------------------------------------------------
K_NETWORK = 128          # wave_sort_tile<2>
K_LIGHT_SAMPLE = 512     # light kernel: the sample sort up to here, wave_sort_tile<16> up to K_WAVE
K_WAVE = 1024            # one wave
K_QUAD = 4096            # the workgroup's four waves
K_MID = 8192             # coop_sort_tile<8> (heavy frames)
K_LARGE = 16384          # coop_sort_tile<16>; above: radix_sort_tile<16>
K_MAX_BUCKET = 64        # kSsMaxBucket
ONE_WAVE_EDGES = (192, 256, 384, 512, 768, 1024)            # KPL 3, 4, 6, 8, 12, 16
FOUR_WAVE_EDGES = (1280, 1536, 2048, 2560, 3072, 4096)      # KPL 5, 6, 8, 10, 12, 16


def route(lengths):
    """What launch_tile_depth_sort does with a frame of these per-tile list lengths when it is handed the exact L."""
    lengths = np.asarray(lengths, dtype=np.int64)
    L, T = int(lengths.sum()), int(lengths.shape[0])
    quad = L > 512 * T
    heavy = L > 1024 * T
    large = int(((lengths > K_QUAD) & (lengths <= K_LARGE)).sum()) if quad else 0       # (a light frame files nothing)
    huge = int((lengths > K_LARGE).sum()) if quad else 0
    return dict(L=L, T=T, quad=bool(quad), heavy=bool(heavy), large=large, huge=huge,
                name="heavy" if heavy else ("quad" if quad else "light"))


def sample_sort_class(n, quad):
    """Does the tile go to sample_sort_tile first (and to the network only when a fine bucket overflows)?"""
    return K_NETWORK < n <= (K_QUAD if quad else K_LIGHT_SAMPLE)


def sorter(n, r):
    """Name of the code that sorts a list of ``n`` under route ``r`` (for the coverage table and the messages)."""
    if n <= 1:
        return "none"
    if n <= K_NETWORK:
        return "network2"
    if not r["quad"]:
        if n <= K_LIGHT_SAMPLE:
            return "sample1/kpl%d" % (3, 4, 6, 8)[sum(n > e for e in ONE_WAVE_EDGES[:4])]
        return "network16" if n <= K_WAVE else "radix4"
    if n <= K_WAVE:
        return "sample1/kpl%d" % (3, 4, 6, 8, 12, 16)[sum(n > e for e in ONE_WAVE_EDGES)]
    if n <= K_QUAD:
        return "sample4/kpl%d" % (5, 6, 8, 10, 12, 16)[sum(n > e for e in FOUR_WAVE_EDGES)]
    if n <= K_LARGE:
        return "coop8" if r["heavy"] and n <= K_MID else "coop16"
    return "radix16"


# ---- depth patterns: (n, rng) -> float32[n], every value > NEAR_Z = 0.2 ------------------------------------------------------
def _distinct(draw, n, exclude=()):
    out = np.empty(0, dtype=F)
    while out.shape[0] < n:
        more = np.concatenate([out, draw(2 * (n - out.shape[0]) + 8).astype(F)])
        _, first = np.unique(more, return_index=True)
        more = more[np.sort(first)]
        for v in exclude:
            more = more[more != F(v)]
        out = more[:n]
    return out


def smooth(n, rng):
    """Distinct, uniform in [1, 50]."""
    return _distinct(lambda m: rng.uniform(1.0, 50.0, m), n)


def wide(n, rng):
    """Distinct, log-uniform in [0.25, 8192]: 15 octaves, a span of 15 * 2^23 bit patterns -- the (float)(kd - l) of the
    fine-bucket interpolation rounds."""
    return _distinct(lambda m: np.exp(rng.uniform(math.log(0.25), math.log(8192.0), m)), n)


def ulps(n, rng):
    """n consecutive bit patterns, shuffled: h - l is tiny."""
    bits = np.array([3.0], dtype=F).view(np.uint32)[0] + np.arange(n, dtype=np.uint32)
    return rng.permutation(bits).view(F)


def outlier(n, rng):
    """n - 1 distinct values within a relative 1e-3 of 5, one at 1000."""
    lo, hi = (np.array([5.0, 5.005], dtype=F).view(np.uint32)).astype(np.int64)
    bits = (lo + rng.choice(hi - lo, size=n - 1, replace=False)).astype(np.uint32)
    z = np.concatenate([bits.view(F), np.array([1000.0], dtype=F)])
    return rng.permutation(z)


def all_equal(n, rng):
    """One value: the sorted list is the ascending ids."""
    return np.full(n, 7.25, dtype=F)


def two_values(n, rng):
    z = np.full(n, 9.75, dtype=F)
    z[: n // 2] = F(4.5)
    return rng.permutation(z)


def _block(k):
    def pattern(n, rng):
        rest = _distinct(lambda m: rng.uniform(1.0, 50.0, m), n - k, exclude=(12.5,))
        return rng.permutation(np.concatenate([np.full(k, 12.5, dtype=F), rest]))
    pattern.__doc__ = f"{k} copies of one value among otherwise smooth depths (kSsMaxBucket = {K_MAX_BUCKET})."
    return pattern


PATTERNS = dict(smooth=smooth, wide=wide, ulps=ulps, outlier=outlier, all_equal=all_equal, two_values=two_values,
                block65=_block(65), block64=_block(64))
# largest number of equal depths a pattern puts into a list of n
MULTIPLICITY = dict(smooth=lambda n: 1, wide=lambda n: 1, ulps=lambda n: 1, outlier=lambda n: 1, all_equal=lambda n: n,
                    two_values=lambda n: n - n // 2, block65=lambda n: 65, block64=lambda n: 64)
# equal depths share a fine bucket (fb is a function of the depth bits alone): more than kSsMaxBucket of them MUST send a
# sample-sort-class tile to the network
MUST_FALL_BACK = ("all_equal", "two_values", "block65")
ADVERSARIAL = ("wide", "ulps", "outlier", "all_equal", "two_values", "block65", "block64")


# ---- frames -------------------------------------------------------------------------------------------------------------------
def _s(*ns):
    return [(n, "smooth") for n in ns]


def _each(patterns, *ns):
    return [(n, p) for p in patterns for n in ns]


_SIX = tuple(p for p in ADVERSARIAL if p != "wide")

# name -> (family, W, H, [(n, pattern) for tile 0, 1, ...]; the remaining tiles are empty)
FRAME_SPECS = {
    # T = 18 (not a multiple of 4: the last workgroup's `tile < T` guard), every length up to the one-wave cap
    "light_tiers": ("light", 96, 48, _s(0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 1024)),
    "light_t3": ("light", 48, 16, _s(300, 0, 77)),
    # a crowded tile (radix fallback inside the one-wave kernel), not a multiple of the radix chunk of 256
    "light_crowded_1500": ("light", 64, 32, _s(1500, 40, 0, 200, 130, 3, 513, 100)),
    "light_crowded_4500": ("light", 64, 64, _s(70, 4500, 0, 257, 1, 129, 512, 33)),
    # two crowded tiles in one workgroup (tiles 0 and 2): the radix fallback runs twice over the same LDS
    "light_two_crowded": ("light", 64, 32, _s(1100, 5, 1301, 0, 200, 64, 0, 129)),
    # tiles 0 .. 3: two quad-class tiles and an empty one in one workgroup; 4097 and 8193: the big kernel, large_lo = 0
    "quad_tiers": ("quad", 128, 96, _s(1025, 0, 2049, 300, 768, 769, 1024, 1280, 1281, 1536, 1537, 2048, 2560, 2561, 3072,
                                       3073, 4096, 4097, 8193, 130, 200, 513, 600, 1, 100)),
    # the mid kernel (<= 8192), the big kernel above, the huge class, a few quad-class tiles
    "heavy_classes": ("heavy", 64, 64, _s(4097, 1100, 8192, 0, 8193, 2500, 16384, 4096, 16385, 300, 2)),
    # one wave, KPL 3 (180) and KPL 16 (1000); the network size 100
    "adv_one_wave": ("adversarial", 112, 32, _each(_SIX, 180, 1000) + [(100, "all_equal"), (500, "all_equal")]),
    # four waves, KPL 5 (1200) and KPL 16 (4000); all_equal in the large class (both kernels) and the huge class
    "adv_four_waves": ("adversarial", 64, 64, _each(_SIX, 1200, 4000) +
                       [(5000, "all_equal"), (9000, "all_equal"), (16500, "all_equal")]),
    "adv_wide": ("adversarial", 64, 32, [(n, "wide") for n in (180, 1000, 1200, 4000, 100)]),
    # the light kernel's own instantiations: KPL 3, KPL 8, the 16-key network, the radix fallback
    "adv_light": ("adversarial", 64, 48, _each(ADVERSARIAL, 180) +
                  [(100, "all_equal"), (500, "all_equal"), (1000, "all_equal"), (1500, "all_equal")]),
}
FAMILIES = ("light", "quad", "heavy", "adversarial")
# the route each frame is built for
FRAME_ROUTES = dict(light_tiers="light", light_t3="light", light_crowded_1500="light", light_crowded_4500="light",
                    light_two_crowded="light", quad_tiers="quad", heavy_classes="heavy", adv_one_wave="quad",
                    adv_four_waves="heavy", adv_wide="quad", adv_light="light")

# Every edge the frames must stand on: (route, n, pattern).  tests/test_depth_sort_cases_cpu.py walks this table.
EDGES = (
    [("light", n, "smooth") for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 1024)] +
    [("quad", n, "smooth") for n in (768, 769, 1024, 1025, 1280, 1281, 1536, 1537, 2048, 2049, 2560, 2561, 3072, 3073,
                                     4096, 4097, 8193)] +
    [("heavy", n, "smooth") for n in (4097, 8192, 8193, 16384, 16385)] +
    [("quad", n, p) for p in ADVERSARIAL for n in (180, 1000)] +                     # one wave: KPL 3, KPL 16
    [("quad|heavy", n, p) for p in ADVERSARIAL for n in (1200, 4000)] +              # four waves: KPL 5, KPL 16
    [("light", 180, p) for p in ADVERSARIAL] +
    [("quad", 100, "all_equal"), ("light", 100, "all_equal"), ("heavy", 5000, "all_equal"), ("heavy", 9000, "all_equal"),
     ("heavy", 16500, "all_equal"), ("light", 1500, "all_equal")]
)


@dataclass
class Frame:
    name: str
    family: str
    W: int
    H: int
    entries: list                 # [(tile, n, pattern)]
    lengths: np.ndarray           # [T] designed list length per tile
    route: dict                   # route(lengths)
    z: np.ndarray                 # [P] float32 designed depth per Gaussian
    tile_of: np.ndarray           # [P] tile each Gaussian sits in
    means3D: np.ndarray
    scales: np.ndarray
    rotations: np.ndarray
    opacities: np.ndarray
    shs: np.ndarray               # [P,1,3]
    cam: object = field(repr=False, default=None)

    @property
    def P(self):
        return int(self.z.shape[0])

    @property
    def min_fallbacks(self):
        """Lower bound on big[2]: sample-sort-class tiles that hold more than kSsMaxBucket equal depths."""
        return sum(1 for _, n, p in self.entries
                   if p in MUST_FALL_BACK and sample_sort_class(n, self.route["quad"]) and MULTIPLICITY[p](n) > K_MAX_BUCKET)

    @property
    def zero_fallbacks(self):
        """Distinct, spread depths only: the design claim that fine buckets hold a few keys says no tile falls back."""
        return all(p in ("smooth", "wide") for _, _, p in self.entries)


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (1 << 31)


@functools.lru_cache(maxsize=None)
def build(name) -> Frame:
    family, W, H, spec = FRAME_SPECS[name]
    assert W % TILE == 0 and H % TILE == 0
    gx, gy = W // TILE, H // TILE
    T = gx * gy
    assert len(spec) <= T, name
    cam = synth.make_camera(W, H)
    rng = np.random.default_rng(_seed(name))
    entries = [(tile, n, p) for tile, (n, p) in enumerate(spec)]
    lengths = np.zeros(T, dtype=np.int64)
    zs, tiles = [], []
    for tile, n, p in entries:
        lengths[tile] = n
        if n:
            z = PATTERNS[p](n, rng)
            assert z.dtype == np.float32 and z.shape == (n,) and float(z.min()) > 0.2
            zs.append(z)
            tiles.append(np.full(n, tile, dtype=np.int64))
    z = np.concatenate(zs)
    tile_of = np.concatenate(tiles)
    perm = rng.permutation(z.shape[0])                   # ids carry no depth (and no tile) order
    z, tile_of = z[perm], tile_of[perm]
    # centre pixel of the tile; px = ((ndc + 1) W - 1) / 2 and x = ndc z tanfovx, inverted (the same for y)
    px = (tile_of % gx) * TILE + TILE // 2
    py = (tile_of // gx) * TILE + TILE // 2
    ndcx = (2.0 * px + 1.0) / W - 1.0
    ndcy = (2.0 * py + 1.0) / H - 1.0
    zd = z.astype(np.float64)
    means = np.stack([ndcx * zd * cam.tanfovx, ndcy * zd * cam.tanfovy, zd], 1).astype(F)
    assert np.array_equal(means[:, 2].view(np.uint32), z.view(np.uint32))
    P = z.shape[0]
    scales = np.repeat((F(1e-4) * z)[:, None], 3, axis=1).astype(F)
    rot = np.zeros((P, 4), dtype=F)
    rot[:, 0] = 1.0
    fr = Frame(name=name, family=family, W=W, H=H, entries=entries, lengths=lengths, route=route(lengths), z=z,
               tile_of=tile_of, means3D=means, scales=scales, rotations=rot, opacities=np.full((P, 1), 0.02, dtype=F),
               shs=np.full((P, 1, 3), 0.5, dtype=F), cam=cam)
    for a in (fr.lengths, fr.z, fr.tile_of, fr.means3D, fr.scales, fr.rotations, fr.opacities, fr.shs):
        a.setflags(write=False)
    return fr


def family_frames(family):
    return [n for n, s in FRAME_SPECS.items() if s[0] == family]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(Geometry, Binning) of the frame from the CPU oracle: numpy's stable argsort over (tile << 32 | depth bits) with ids
    in ascending emission order -- the (depth bits, id) order.  Computed once, shared, read-only."""
    from oracle import raster_oracle as ro
    fr = build(name)
    geom = ro.geometry_spec(fr.means3D, fr.scales, fr.rotations, None, fr.cam.world_view_transform.numpy(),
                            fr.cam.full_proj_transform.numpy(), fr.W, fr.H, fr.cam.tanfovx, fr.cam.tanfovy, 1.0)
    binning = ro.binning_spec(geom)
    for a in (binning.point_list, binning.ranges, binning.keys_sorted):
        a.setflags(write=False)
    return geom, binning


# ---- the GPU side (torch and the extension are imported here, not above: the module stays importable without them) ---
def render(name, device, debug=False):
    """One forward of the frame through ``dgr._C.rasterize_gaussians``.  Returns (call, L, ranges [T,2], point_list [L]),
    the two arrays as numpy copies of ``raster_views``."""
    import torch
    import diff_gaussian_rasterization as dgr
    import parity as pa
    fr = build(name)
    t = lambda a: torch.from_numpy(np.array(a)).to(device)             # (a copy: the frame's arrays are read-only)
    rs = dgr.GaussianRasterizationSettings(**pa.settings_kwargs(fr.cam, torch.zeros(3), 0, do_depth=False, debug=debug,
                                                                device=device))
    L, color, radii, _, _, _, invd, call = dgr._C.rasterize_gaussians(
        rs.bg, t(fr.means3D), None, t(fr.opacities), t(fr.scales), t(fr.rotations), 1.0, None, rs.viewmatrix,
        rs.projmatrix, rs.tanfovx, rs.tanfovy, fr.H, fr.W, t(fr.shs), 0, rs.campos, False, debug, rs.render_indices,
        rs.parent_indices, rs.interpolation_weights, rs.num_node_kids, False)
    v = dgr._C.raster_views(call)
    ranges, plist = v["ranges"].cpu().numpy().copy(), v["point_list"].cpu().numpy().copy()
    return call, int(L), ranges, plist


def mismatches(name, L, ranges, plist):
    """Exact comparison with the oracle: no tolerance, no entry left out.  Returns the counts and, for the message, the
    tiles whose lists differ with their length, pattern and sorter."""
    fr = build(name)
    _, ref = reference(name)
    out = dict(frame=name, L=int(L), L_ref=int(ref.num_rendered),
               ranges_bad=int((ranges.astype(np.int64) != ref.ranges.astype(np.int64)).sum()) if ranges.shape == ref.ranges.shape else -1,
               list_bad=-1, tiles_bad=[])
    if L == ref.num_rendered and plist.shape == ref.point_list.shape:
        bad = plist.astype(np.int64) != ref.point_list.astype(np.int64)
        out["list_bad"] = int(bad.sum())
        for tile, n, p in fr.entries:
            r0, r1 = ref.ranges[tile]
            if bad[r0:r1].any():
                out["tiles_bad"].append(dict(tile=tile, n=n, pattern=p, sorter=sorter(n, fr.route), bad=int(bad[r0:r1].sum())))
    return out


def clean(m):
    return m["L"] == m["L_ref"] and m["ranges_bad"] == 0 and m["list_bad"] == 0
