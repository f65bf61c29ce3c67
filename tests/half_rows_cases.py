"""Shared cases of the half-row tests (test_half_rows_cpu.py, test_half_rows_kernels_gpu.py, test_half_rows_gpu.py): a
helper module, not a test.

NARROW_CASES is the narrowing rule of include/hgs.h (HGS_RESID_HOST_ROW_BYTES_HALF) by example: (float32 value, IEEE half
bits).  The bits are written out by hand from the format -- 1 sign, 5 exponent (bias 15), 10 mantissa bits; the subnormal
unit is 2^-24; the largest finite half is 0x7bff = 65504 -- and are not produced by any function under test."""
import numpy as np

NARROW_CASES = [
    (0.0, 0x0000), (-0.0, 0x8000),
    (2.0 ** -24, 0x0001),                  # the smallest subnormal half
    (2.0 ** -25, 0x0000),                  # half of it: a tie between 0 and 0x0001, to even
    (-(2.0 ** -25), 0x8000),
    (1.5 * 2.0 ** -24, 0x0002),            # a tie between 0x0001 and 0x0002
    (2.5 * 2.0 ** -24, 0x0002),            # a tie between 0x0002 and 0x0003
    (1.0 + 2.0 ** -11, 0x3C00),            # midway between 1 (0x3c00, even) and 1 + 2^-10 (0x3c01)
    (1.0 + 3 * 2.0 ** -11, 0x3C02),        # midway between 0x3c01 and 0x3c02 (even)
    (2049.0, 0x6800),                      # halves step by 2 above 2048 = 0x6800: midway to 2050 = 0x6801
    (2051.0, 0x6802),                      # midway between 2050 and 2052
    (-2049.0, 0xE800),
    (65504.0, 0x7BFF),
    (65519.9, 0x7BFF),                     # rounds down to 65504 by itself
    (65520.0, 0x7BFF),                     # would round to infinity: saturates
    (1e9, 0x7BFF), (-1e9, 0xFBFF),
    (6.1e-5, 0x03FF),                      # just below 2^-14: 6.1e-5 / 2^-24 = 1023.41 -> subnormal 1023
    (float("nan"), 0x7E00),
    (float("inf"), 0x7C00), (float("-inf"), 0xFC00),
]
NARROW_VALUES = np.array([v for v, _ in NARROW_CASES], np.float32)
NARROW_BITS = np.array([b for _, b in NARROW_CASES], np.uint16)

# IEEE half -> float32 by the format's definition, for every bit pattern (a table: 65 536 entries)
_b = np.arange(1 << 16, dtype=np.int64)
_e, _m = (_b >> 10) & 31, (_b & 1023).astype(np.float64)
_mag = np.where(_e == 0, _m * 2.0 ** -24, np.where(_e == 31, np.where(_m == 0, np.inf, np.nan), (1024 + _m) * 2.0 ** (_e - 25.0)))
WIDEN_TABLE = (np.where(_b >> 15, -1.0, 1.0) * _mag).astype(np.float32)


def widen(bits):
    """IEEE half bits -> float32 through the table above."""
    return WIDEN_TABLE[np.asarray(bits, np.int64)]


def attribute_arrays(G, M, seed, with_cases=True):
    """Five float32 numpy arrays of G rows ([G,3], [G,M,3], [G,1], [G,3], [G,4]) of mixed magnitudes and signs (values
    up to ~1e5, down to ~1e-8); with_cases: NARROW_VALUES, its NaN and infinities included, strewn over every field."""
    rng = np.random.default_rng(seed)
    shapes = dict(means3D=(G, 3), shs=(G, M, 3), opacities=(G, 1), scales=(G, 3), rotations=(G, 4))
    out = []
    for k, shape in shapes.items():
        a = (rng.standard_normal(shape) * 10.0 ** rng.integers(-8, 6, shape)).astype(np.float32)
        if with_cases:                                   # (a field with fewer elements than cases takes a window of them)
            flat = a.reshape(-1)
            at = rng.permutation(flat.size)[:len(NARROW_VALUES)]
            flat[at] = np.roll(NARROW_VALUES, -int(rng.integers(len(NARROW_VALUES))))[:len(at)]
        out.append(a)
    return tuple(out)


def half_pattern_rows(G, M):
    """Half host rows uint8 [G, 128] for the fetch tests: every useful half is a function of (id, column) that runs
    through normal values of both signs, +-0, subnormal halves and 65504; the padding halves [3 M, 48) are the NaN 0x7e01,
    bytes 124..127 the float32 NaN 0x7fc00001; the mean is id * 4 + component (float32).  -> (rows, float rows [G, 64] in
    the float layout of HGS_RESID_HOST_ROW_FLOATS holding the exact widening, NaN in its padding)."""
    ids, col = np.arange(G, dtype=np.int64)[:, None], np.arange(56, dtype=np.int64)[None, :]
    k = ids * 56 + col
    bits = ((k * 37 + 11) % 0x7C00).astype(np.uint16)                  # finite magnitudes: exponent fields 0 .. 30
    bits |= ((k % 3 == 0).astype(np.uint16) << 15)                      # both signs
    special = np.array([0x0000, 0x8000, 0x0001, 0x83FF, 0x7BFF, 0xFBFF, 0x0400], np.uint16)
    pick = k % 5 == 0
    bits[pick] = special[(k[pick] // 5) % len(special)]
    bits[:, 3 * M:48] = 0x7E01
    rows = np.zeros((G, 128), np.uint8)
    rows[:, :112] = bits.view(np.uint8)
    means = (np.arange(G, dtype=np.float32)[:, None] * 4 + np.arange(3, dtype=np.float32)[None, :]).astype(np.float32)
    rows[:, 112:124] = means.view(np.uint8)
    rows[:, 124:128] = np.array([0x7FC00001], np.uint32).view(np.uint8)
    wide = np.full((G, 64), np.nan, np.float32)
    f = widen(bits)
    wide[:, :3 * M] = f[:, :3 * M]
    wide[:, 48:52] = f[:, 48:52]          # rotation
    wide[:, 52:55] = means
    wide[:, 55:58] = f[:, 52:55]          # scale
    wide[:, 58] = f[:, 55]                # opacity
    return rows, wide
