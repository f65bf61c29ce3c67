"""Model of the LOD gather / scatter and a builder of hand-made cuts (a helper module, no GPU).

Row i of a hierarchy render is  w_i * attr[r_i] + (1 - w_i) * attr[p_i]  with the parent quaternion flipped into the
node's hemisphere first; the backward sends  w_i g_i  to the node row and  (1 - w_i) g_i  to the parent row, summed over
the siblings.  Three pieces of device code implement that (csrc/lod_gather.hip stand-alone, the LOD instantiations of
csrc/preprocess.hip in-op); this module is what they are compared with:

``build_cut``       cuts with chosen run geometry (runs of siblings = rows sharing a parent), emitted or shuffled
``make_rotations``  unit quaternions whose node / parent dot product is forced negative, exactly 0 or -0.0 where asked
``gather_f32``      the forward in float32 with every operation rounded on its own: what lod_gather.hip promises, so
                    the stand-alone gather is held to bit equality
``scatter_f64``     the float64 adjoint with, per output element, the number of products added and their absolute mass
``scatter_bound``   (terms + 2) * 2**-24 * mass: each product carries at most two roundings (1 - w, the product), a sum
                    of ``terms`` values at most terms - 1 more, in ANY order (atomics included)
``check_scatter``   the bound per element, bit-zero per untouched row
``check_rows``      the rule for gradients that went through the rasterizer's float32 chain first: per touched row
                    |got - ref|_inf <= rel * sum_j |coef_j| |g_j|_inf, so a wrong small row cannot hide behind a large one
"""
from dataclasses import dataclass

import numpy as np

GROUPS = ("means3D", "scales", "rotations", "shs", "opacities")     # the order of the C entry points
U = 2.0 ** -24                                                      # unit roundoff of float32
SPECIAL_WEIGHTS = (1.0, 0.0, 0.5, 1.0 - 2.0 ** -24)
BLOCK = 256                                                         # rows per workgroup of every LOD kernel


@dataclass
class Cut:
    ri: np.ndarray       # int32 [n] node rows (unique)
    pi: np.ndarray       # int32 [n] parent rows
    w: np.ndarray        # float32 [n]
    G: int               # rows of the attribute arrays
    order: str

    @property
    def n(self):
        return len(self.ri)

    def runs(self):
        """[(first, end)] of the maximal runs of equal parents, in row order."""
        cuts = np.flatnonzero(np.diff(self.pi)) + 1
        edges = np.concatenate(([0], cuts, [self.n]))
        return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def build_cut(runs, extra_rows=0, order="emitted", seed=0, self_parent=False, w1_runs=(), weights=None):
    """``runs``: lengths of the sibling runs.  Parent rows distinct and ascending, node rows distinct, ascending and
    disjoint from the parent rows -- the way expand_to_size emits a cut (children contiguous, parents non-decreasing);
    ``extra_rows`` more rows that the cut does not name lie between them.  ``order="shuffled"`` cuts runs into pieces and
    permutes the pieces: the parents are no longer sorted and at least one parent owns two separate runs.
    ``self_parent``: a one-entry cut with p == r (a root).  ``w1_runs``: runs whose entries all get weight exactly 1 (their
    parent then has no weight in any row).  Weights: one each of exactly 1, exactly 0, 0.5 and 1 - 2**-24 (all four from
    eight entries on, never more than half the entries), the rest uniform in [0.05, 0.95] -- no ordinary term is
    negligible; ``weights`` overrides them."""
    rng = np.random.default_rng(seed)
    if self_parent:
        G = 1 + extra_rows
        row = int(rng.integers(0, G))
        w = np.array([1.0 if weights is None else weights[0]], dtype=np.float32)
        return Cut(np.array([row], np.int32), np.array([row], np.int32), w, G, "emitted")
    runs = [int(k) for k in runs]
    assert runs and min(runs) >= 1
    R, n = len(runs), sum(runs)
    e_par = extra_rows // 2
    par_rows = np.sort(rng.choice(R + e_par, size=R, replace=False))
    node_rows = R + e_par + np.sort(rng.choice(n + extra_rows - e_par, size=n, replace=False))
    G = R + n + extra_rows
    ri = node_rows.astype(np.int32)
    pi = np.repeat(par_rows, runs).astype(np.int32)
    first = np.concatenate(([0], np.cumsum(runs)))
    w = rng.uniform(0.05, 0.95, size=n).astype(np.float32)
    in_w1 = np.zeros(n, dtype=bool)
    for k in w1_runs:
        in_w1[first[k]:first[k + 1]] = True
    free = np.flatnonzero(~in_w1)
    spots = rng.permutation(free)[:min(len(SPECIAL_WEIGHTS), max(1, len(free) // 2))]    # (at most half the entries)
    special = np.roll(np.array(SPECIAL_WEIGHTS, dtype=np.float32), seed)
    w[spots] = special[:len(spots)]
    w[in_w1] = 1.0
    if weights is not None:
        w = np.asarray(weights, dtype=np.float32).copy()
        assert w.shape == (n,)
    if order == "shuffled":
        pieces = []
        for a, b in zip(first[:-1], first[1:]):
            if b - a >= 2:
                m = int(rng.integers(a + 1, b))
                pieces += [(a, m), (m, b)]
            else:
                pieces.append((a, b))
        assert len(pieces) > len(runs), "a shuffled cut needs a run of two or more"
        for _ in range(64):
            perm = rng.permutation(len(pieces))
            idx = np.concatenate([np.arange(*pieces[k]) for k in perm])
            c = Cut(ri[idx], pi[idx], w[idx], G, "shuffled")
            starts = [c.pi[a] for a, _ in c.runs()]
            if bool((np.diff(c.pi) < 0).any()) and len(starts) > len(set(starts)):
                return c
        raise AssertionError("no permutation with a parent that owns two runs")
    assert order == "emitted"
    return Cut(ri, pi, w, G, "emitted")


def check_cut(cut):
    """Validity of a built cut: unique node rows, node and parent rows disjoint (except a self-parent root), in range,
    monotone when emitted."""
    assert len(np.unique(cut.ri)) == cut.n
    if not (cut.n == 1 and cut.ri[0] == cut.pi[0]):
        assert not set(cut.ri.tolist()) & set(cut.pi.tolist())
    assert cut.ri.min() >= 0 and cut.pi.min() >= 0 and max(cut.ri.max(), cut.pi.max()) < cut.G
    mono = not bool((np.diff(cut.pi) < 0).any())
    assert mono == (cut.order == "emitted")
    if mono:
        assert bool((np.diff(cut.ri) > 0).all())
        assert len(cut.runs()) == len(np.unique(cut.pi))
    else:
        assert len(cut.runs()) > len(np.unique(cut.pi))


def dot_f64(q, qp):
    return (q.astype(np.float64) * qp.astype(np.float64)).sum(-1)


def make_rotations(cut, negative=(), zero=(), neg_zero=(), seed=0):
    """[G, 4] float32 unit quaternions.  For the cut entries listed in ``negative`` the node . parent dot product is below
    -1e-3; for those in ``zero`` it is exactly 0 ((1,0,0,0) against (0,1,0,0)), for those in ``neg_zero`` every product is
    a zero and the first is -0.0 ((1,0,0,0) against (-0.0,1,0,0)) -- neither may flip.  Every other pair has
    |dot| > 1e-3 in float64, so its sign is never a rounding question.  Forcing an entry rewrites its NODE row (unique to
    the entry); ``zero`` / ``neg_zero`` also rewrite the parent row, so at most one of them per run."""
    rng = np.random.default_rng(seed + 1000)
    q = rng.standard_normal((cut.G, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    forced = {}
    for i in zero:
        forced[int(i)] = "zero"
    for i in neg_zero:
        forced[int(i)] = "neg_zero"
    fixed_parents = set()
    for i, kind in forced.items():
        r, p = int(cut.ri[i]), int(cut.pi[i])
        assert r != p and p not in fixed_parents, "one exact-zero pair per run"
        fixed_parents.add(p)
        q[r] = (1.0, 0.0, 0.0, 0.0)
        q[p] = (0.0, 1.0, 0.0, 0.0) if kind == "zero" else (-0.0, 1.0, 0.0, 0.0)
    neg = {int(i) for i in negative}
    assert not neg & set(forced)
    for i in range(cut.n):
        if i in forced:
            continue
        r, p = int(cut.ri[i]), int(cut.pi[i])
        if r == p:
            continue
        for _ in range(100):
            d = float(dot_f64(q[r], q[p]))
            if abs(d) > 1e-3:
                break
            v = rng.standard_normal(4)
            q[r] = (v / np.linalg.norm(v)).astype(np.float32)
        else:
            raise AssertionError("no quaternion away from the parent's equator")
        if (i in neg) != (d < 0):
            q[r] = -q[r]
    for i in range(cut.n):
        r, p = int(cut.ri[i]), int(cut.pi[i])
        d = float(dot_f64(q[r], q[p]))
        if i in forced:
            assert d == 0.0 and np.signbit(q[r][0] * q[p][0]) == (forced[i] == "neg_zero")
        elif r != p:
            assert abs(d) > 1e-3 and (d < -1e-3) == (i in neg), (i, d)
    return q


def flip_signs(rotations, ri, pi):
    """+1 / -1 per entry: -1 where the float32 dot product, summed left to right, is strictly negative."""
    a, b = rotations[ri], rotations[pi]
    f = np.float32
    d = f(f(f(a[:, 0] * b[:, 0]) + f(a[:, 1] * b[:, 1])) + f(a[:, 2] * b[:, 2])) + f(a[:, 3] * b[:, 3])
    return np.where(d < 0, -1.0, 1.0).astype(np.float32)


def gather_f32(attrs, ri, pi, w, rot_key="rotations"):
    """{name: [G, ...] float32} -> {name: [n, ...] float32}: u = f32(1) - w, w * a, u * b and the sum each rounded to
    float32 on its own; the quaternion dot product summed left to right, the parent negated (exactly) where it is
    strictly negative.  Signed zeros come out as this evaluation makes them."""
    ri, pi = np.asarray(ri, dtype=np.int64), np.asarray(pi, dtype=np.int64)
    w = np.asarray(w, dtype=np.float32)
    u = (np.float32(1.0) - w).astype(np.float32)
    out = {}
    for k, a in attrs.items():
        assert a.dtype == np.float32
        node, par = a[ri], a[pi]
        if k == rot_key:
            par = par * flip_signs(a, ri, pi)[:, None]
        shape = (-1,) + (1,) * (a.ndim - 1)
        x = (w.reshape(shape) * node).astype(np.float32)
        y = (u.reshape(shape) * par).astype(np.float32)
        out[k] = (x + y).astype(np.float32)
    return out


@dataclass
class Model:
    ref: np.ndarray        # float64 [G, D]
    terms: np.ndarray      # int64 [G, D] products added into the element
    mass: np.ndarray       # float64 [G, D] sum |coef_j g_j|
    rowmass: np.ndarray    # float64 [G] sum |coef_j| |g_j|_inf
    shape: tuple           # of the full array

    @property
    def touched(self):
        return self.terms[:, 0] > 0


def scatter_f64(grads, ri, pi, w, G, rotations=None, shapes=None, rot_key="rotations"):
    """The adjoint of the gather in float64.  ``grads``: {name: [n, ...]} row gradients; ``rotations``: the full [G, 4]
    float32 array (the hemisphere signs), needed when ``grads`` has ``rot_key``.  A self-parent entry (p == r) is the
    identity: its gradient goes to the row once, with coefficient 1.  Returns {name: Model}."""
    ri, pi = np.asarray(ri, dtype=np.int64), np.asarray(pi, dtype=np.int64)
    wd = np.asarray(w, dtype=np.float32).astype(np.float64)
    self_par = ri == pi
    c_node = np.where(self_par, 1.0, wd)
    c_par = np.where(self_par, 0.0, 1.0 - wd)
    on_par = ~self_par
    out = {}
    for k, g in grads.items():
        g = np.asarray(g)
        n = g.shape[0]
        g2 = g.astype(np.float64).reshape(n, -1)
        D = g2.shape[1]
        sign = np.ones(n)
        if k == rot_key:
            sign = flip_signs(rotations, ri, pi).astype(np.float64)
        ref, mass = np.zeros((G, D)), np.zeros((G, D))
        terms, rowmass = np.zeros((G, D), dtype=np.int64), np.zeros(G)
        np.add.at(ref, ri, c_node[:, None] * g2)
        np.add.at(mass, ri, np.abs(c_node[:, None] * g2))
        np.add.at(terms, ri, 1)
        np.add.at(rowmass, ri, c_node * np.abs(g2).max(1))
        np.add.at(ref, pi[on_par], (c_par * sign)[on_par, None] * g2[on_par])
        np.add.at(mass, pi[on_par], np.abs(c_par[on_par, None] * g2[on_par]))
        np.add.at(terms, pi[on_par], 1)
        np.add.at(rowmass, pi[on_par], c_par[on_par] * np.abs(g2[on_par]).max(1))
        full = tuple(shapes[k]) if shapes is not None else (G,) + tuple(g.shape[1:])
        out[k] = Model(ref, terms, mass, rowmass, full)
    return out


def scatter_bound(terms, mass):
    return (terms + 2) * U * mass


def _bit_zero(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) == 0


def check_scatter(got, model):
    """``got``: {name: [G, ...] float32}, ``model``: scatter_f64's result.  Every element within scatter_bound of the
    float64 adjoint; every row nothing is added into holds +0.0 bits."""
    assert got.keys() == model.keys(), (sorted(got), sorted(model))
    for k, m in model.items():
        a = np.asarray(got[k])
        assert a.dtype == np.float32 and a.size == m.ref.size, (k, a.dtype, a.shape)
        a = a.reshape(m.ref.shape)
        assert np.isfinite(a).all(), (k, "non-finite gradient")
        zero_ok = _bit_zero(a[~m.touched]).all()
        assert zero_ok, (k, "rows outside the cut must stay +0.0", np.flatnonzero(~_bit_zero(a).all(1) & ~m.touched)[:8])
        err = np.abs(a.astype(np.float64) - m.ref)
        bad = err > scatter_bound(m.terms, m.mass)
        if bad.any():
            r, c = np.argwhere(bad)[0]
            raise AssertionError(f"{k}: {int(bad.sum())} elements outside (terms + 2) 2^-24 mass; first row {r} col {c}: "
                                 f"got {a[r, c]!r}, ref {m.ref[r, c]!r}, terms {m.terms[r, c]}, mass {m.mass[r, c]!r}")


def check_rows(got, model, rel=2e-5):
    """Per touched row |got - ref|_inf <= rel * sum_j |coef_j| |g_j|_inf over the terms the model adds into the row;
    rows outside the cut bit-zero."""
    assert got.keys() == model.keys(), (sorted(got), sorted(model))
    for k, m in model.items():
        a = np.asarray(got[k])
        assert a.dtype == np.float32 and a.size == m.ref.size, (k, a.dtype, a.shape)
        a = a.reshape(m.ref.shape)
        assert np.isfinite(a).all(), (k, "non-finite gradient")
        assert _bit_zero(a[~m.touched]).all(), (k, "rows outside the cut must stay +0.0")
        err = np.abs(a.astype(np.float64) - m.ref).max(1)
        bad = err > rel * m.rowmass
        if bad.any():
            r = int(np.flatnonzero(bad)[0])
            raise AssertionError(f"{k}: {int(bad.sum())} rows outside {rel:g} x row mass; first row {r}: err {err[r]!r}, "
                                 f"row mass {m.rowmass[r]!r}")


# ---- the cuts of the GPU tests ----------------------------------------------------------------------------------------
def _fill(total, rng):
    """Run lengths 1..8 mixed, summing to ``total``."""
    out, left = [], total
    while left > 0:
        k = min(int(rng.integers(1, 9)), left)
        out.append(k)
        left -= k
    return out


def _seams_runs():
    rng = np.random.default_rng(5)
    a = _fill(BLOCK - 5, rng) + [5]             # a run of five ends on row 255
    b = [3] + _fill(510 - BLOCK - 3, rng)       # a run of three starts on row 256; rows up to 509
    return a + b + [4, 1]                       # 510..513 straddles 511|512; a run of one on row 514 = n - 1


def _long_runs():
    return [3, 1, 5, 600, 2, 4, 1]              # the long run: rows 9..608, three workgroups (the middle one entirely its)


CUTS = {
    "pair": dict(runs=[2], extra_rows=3),
    "wave": dict(runs=[1, 2, 3, 4, 5, 6, 7, 8, 1, 3, 8, 2, 5], extra_rows=9, w1_runs=(2, 8)),      # n = 55
    "seams": dict(runs=_seams_runs(), extra_rows=21, w1_runs=(1, 3)),
    "long": dict(runs=_long_runs(), extra_rows=11, w1_runs=(1,)),
    "skybox": dict(runs=_fill(250, np.random.default_rng(9)), extra_rows=6, w1_runs=(2,)),
}


def named_cut(name, seed=0):
    """"root", "root_distinct", "root_w0", "root_w1", "pair", "pair_01", "wave", "seams", "long", "skybox" and
    "<name>_shuf".  The mixture cannot put an exact 0 and an exact 1 into one or two entries: "root_w0" / "root_w1" (one
    entry, distinct parent) and "pair_01" (weights 0 and 1) give the one-row and two-row parent sums those weights."""
    if name == "root":
        return build_cut([1], extra_rows=2, self_parent=True, seed=seed)
    if name in ("root_distinct", "root_w0", "root_w1"):
        return build_cut([1], extra_rows=2, weights=[dict(root_distinct=0.5, root_w0=0.0, root_w1=1.0)[name]], seed=seed)
    if name == "pair_01":
        return build_cut(weights=[0.0, 1.0], seed=seed, **CUTS["pair"])
    shuf = name.endswith("_shuf")
    cut = build_cut(order="shuffled" if shuf else "emitted", seed=seed, **CUTS[name[:-5] if shuf else name])
    if name == "seams":
        runs = cut.runs()
        assert cut.n == 515 and any(b == BLOCK for _, b in runs) and (510, 514) in runs and runs[-1] == (514, 515)
    if name == "long":
        assert (9, 609) in cut.runs()
    return cut


CUT_NAMES = ("root", "root_distinct", "root_w0", "root_w1", "pair", "pair_01", "wave", "seams", "long", "wave_shuf", "seams_shuf")


def forced_dots(cut, seed=0):
    """Which entries get a forced dot product: an exact 0 and a -0.0 in two different runs, negatives on the rows next to
    every workgroup boundary (their parent sum is partly another workgroup's) and on a fifth of the rest."""
    rng = np.random.default_rng(seed + 7)
    runs = [(a, b) for a, b in cut.runs() if cut.ri[a] != cut.pi[a]]
    by_parent = {}
    for a, b in runs:
        by_parent.setdefault(int(cut.pi[a]), (a, b))
    firsts = [a for a, _ in by_parent.values()]
    zero = firsts[:1]
    neg_zero = firsts[1:2]
    negative = []
    for i in range(cut.n):
        if cut.ri[i] == cut.pi[i] or i in zero + neg_zero:
            continue
        near_seam = i % BLOCK in (0, 1, BLOCK - 2, BLOCK - 1) and cut.n > BLOCK
        if near_seam or rng.random() < 0.2:
            negative.append(i)
    return dict(negative=negative, zero=zero, neg_zero=neg_zero)


def make_attrs(cut, M, seed=0):
    """Random finite attribute arrays for the C entry points, {name: [G, ...] float32}, with the forced rotations."""
    rng = np.random.default_rng(seed + 11)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(means3D=f(cut.G, 3), scales=np.abs(f(cut.G, 3)) + np.float32(0.01),
                rotations=make_rotations(cut, seed=seed, **forced_dots(cut, seed)), shs=f(cut.G, M, 3),
                opacities=np.abs(f(cut.G, 1)))


def make_row_grads(cut, M, seed=0):
    """Row gradients whose magnitude differs from row to row by up to 100 x: a small sibling next to a large one."""
    rng = np.random.default_rng(seed + 13)
    scale = (10.0 ** rng.uniform(-2.0, 0.0, size=cut.n)).astype(np.float32)
    inner = dict(means3D=(3,), scales=(3,), rotations=(4,), shs=(M, 3), opacities=(1,))
    return {k: (rng.standard_normal((cut.n,) + s).astype(np.float32) * scale.reshape((-1,) + (1,) * len(s)))
            for k, s in inner.items()}
