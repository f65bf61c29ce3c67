"""The float32 rule of the fused Adam (csrc/adam_update.h) in numpy -- TEST INFRASTRUCTURE, a helper module.

The header's five lines are `fmaf`, `* / +` and `sqrtf` on float32; every one of them is correctly rounded on the host
and on gfx950 (adam.hip's code object keeps float32 denormals and uses the refined divide and square root), so the result
is a function of the inputs alone and this restatement gives its BITS.  tests/test_adam_update_on_host.py pins it to the
header compiled for the host; the GPU tests compare the kernels with it and need no compiler.

`fmaf32` is exact: the product of two float32 is exact in float64, `c` is added with a TwoSum, and an inexact sum with an
even last mantissa bit is moved one ulp towards its error (round to odd: 53 >= 2 * 24 + 2 bits, so the second rounding
to float32 sees what the exact sum would show it).  A plain float64 `a * b + c` rounds twice.

Preconditions of `step`, as of hgs_adam_step: every listed row is in [0, P) (anything else is undefined by contract: the
kernel would read and write out of bounds) and no row is listed twice (two threads would race on it)."""
import math
from collections import namedtuple

import numpy as np

F = np.float32
# the float32 scalars of hgs_adam_tensor (include/hgs.h) between row_len and reserved, in their order
Consts = namedtuple("Consts", "step_size beta1 one_minus_beta1 beta2 one_minus_beta2 eps weight_decay "
                              "bias_correction2_sqrt")


def fmaf32(a, b, c):
    """fmaf(a, b, c) on float32 arrays (broadcast), one rounding."""
    a, b, c = (np.asarray(x, dtype=F).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                     # exact: 48 bits, exponents far inside float64's range
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                 # TwoSum: s + e == p + c exactly wherever s is finite
        bits = np.array(s, dtype=np.float64, ndmin=1).view(np.int64)
        fix = (np.isfinite(s) & np.isfinite(e) & (e != 0)).reshape(bits.shape) & ((bits & 1) == 0)
        grow = ((e > 0) == (s > 0)).reshape(bits.shape)            # the error points away from zero
        bits = np.where(fix, np.where(grow, bits + 1, bits - 1), bits)
        return bits.view(np.float64).reshape(np.shape(s)).astype(F)


def tensor_constants(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1):
    """What include/hgs.h tells the caller to pass at step count `step` (after its increment): every value computed in
    Python double and rounded to float32 once."""
    beta1, beta2 = betas
    return Consts(step_size=F(lr / (1 - beta1 ** step)), beta1=F(beta1), one_minus_beta1=F(1 - beta1), beta2=F(beta2),
                  one_minus_beta2=F(1 - beta2), eps=F(eps), weight_decay=F(weight_decay),
                  bias_correction2_sqrt=F(math.sqrt(1 - beta2 ** step)))


def update(T, g, p, m, v):
    """adam_update.h line by line on float32 arrays of one shape -> (p, m, v)."""
    g, p, m, v = (np.asarray(x, dtype=F) for x in (g, p, m, v))
    with np.errstate(all="ignore"):
        if T.weight_decay != 0:
            g = fmaf32(T.weight_decay, p, g)
        m = fmaf32(T.one_minus_beta1, g, m * T.beta1)
        v = fmaf32(T.one_minus_beta2 * g, g, v * T.beta2)
        denom = np.sqrt(v) / T.bias_correction2_sqrt + T.eps
        p = fmaf32(-T.step_size, m / denom, p)
    assert p.dtype == F and m.dtype == F and v.dtype == F and denom.dtype == F
    return p, m, v


def selected(P, rows=None, mask=None):
    """The rows a call updates, as a bool [P]: the listed rows, the rows with mask != 0, or all."""
    assert rows is None or mask is None
    sel = np.zeros(P, dtype=bool)
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        assert ((rows >= 0) & (rows < P)).all() and np.unique(rows).size == rows.size
        sel[rows] = True
    elif mask is not None:
        mask = np.asarray(mask).reshape(-1)
        assert mask.size == P
        sel = mask != 0                               # -0.0 is skipped; subnormals, NaN and infinities are selected
    else:
        sel[:] = True
    return sel


def step(T, param, grad, m, v, rows=None, mask=None):
    """One call for one tensor [P, ...] -> new (param, m, v); unselected rows are copies."""
    param, grad, m, v = (np.array(x, dtype=F) for x in (param, grad, m, v))
    sel = selected(param.shape[0], rows, mask)
    p2, m2, v2 = update(T, grad[sel], param[sel], m[sel], v[sel])
    param[sel], m[sel], v[sel] = p2, m2, v2
    return param, m, v


def same_bits(a, b):
    """Element-wise: equal uint32 views, or both NaN (whatever the payload)."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same_bits(got, want, what, exact=False):
    """All elements of got [P, row_len] equal want (`exact`: NaN payloads too); the message names the first mismatch by
    tensor, row and column with both values as hex, and counts the rest."""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = got.view(np.uint32) == want.view(np.uint32) if exact else same_bits(got, want)
    if ok.all():
        return
    g2, w2, bad = (x.reshape(got.shape[0] if got.ndim else 1, -1) for x in (got, want, ~ok))
    r, c = (int(i[0]) for i in np.nonzero(bad))
    raise AssertionError(f"{what}: row {r} column {c}: got 0x{int(g2.view(np.uint32)[r, c]):08x} ({g2[r, c]!r}), want "
                         f"0x{int(w2.view(np.uint32)[r, c]):08x} ({w2[r, c]!r}); {int(bad.sum())} of {bad.size} "
                         f"elements differ")


# ---- inputs at the rule's edges, shared by the host and the GPU tests ----------------------------------------------
PLANTED_G = (0.0, -0.0, 1e-45, -1e-45, 3e19, -3e19, np.inf, -np.inf, np.nan, 3.4e38)


def log_uniform(rng, shape, lo=1e-24, hi=10.0, signed=True):
    x = 10.0 ** rng.uniform(math.log10(lo), math.log10(hi), size=shape)
    if signed:
        x = x * rng.choice([-1.0, 1.0], size=shape)
    return x.astype(F)


def edge_inputs(rng, shape, planted=PLANTED_G):
    """g, p, m, v of `shape`: |g|, |m| and sqrt(v) log-uniform over 1e-24..10 (so v reaches down through the
    subnormals to 0), p over 1e-6..10, a share of zero-moment elements (a parameter never stepped), zero gradients on
    zero and on non-zero moments, and the `planted` gradient values each in a few elements of their own."""
    n = int(np.prod(shape))
    g, m = log_uniform(rng, n), log_uniform(rng, n)
    with np.errstate(under="ignore"):
        v = (log_uniform(rng, n, signed=False).astype(np.float64) ** 2).astype(F)
    p = log_uniform(rng, n, 1e-6, 10.0)
    fresh = rng.random(n) < 0.15
    m[fresh], v[fresh] = 0, 0
    g[rng.random(n) < 0.1] = 0                        # on zero and on non-zero moments alike
    if planted and n >= 4:
        where = rng.choice(n, size=min(n // 2, max(n // 50, len(planted))), replace=False)
        g[where] = np.resize(np.array(planted, dtype=F), where.size)
    return tuple(x.reshape(shape) for x in (g, p, m, v))
