"""numpy restatement of the budget-exact hierarchy cut (include/hgs.h "Budget-exact cut", DESIGN.md section 4;
csrc/lod_budget.hip): the three cost formulas, the events they are sums of, the brute-force cost at any bit pattern,
the radix descent with the chosen digit split (11, 10, 10 bits: steps 2^20, 2^10, 1) and ``is_monotone``.  Everything
is float32 as ``oracle.lod_oracle.node_size`` computes it; counts are Python / int64 integers.  TEST INFRASTRUCTURE
ONLY."""
from __future__ import annotations

import numpy as np

import frustum_spec as fs
from oracle import lod_oracle as lo

F = np.float32
INF_BITS = 0x7F800000
SHIFTS = (20, 10, 0)


def bits(x) -> int:
    """Bit pattern of a non-negative float32 (-0 counts as +0)."""
    return int(np.asarray(F(x) + F(0.0), dtype=np.float32).view(np.uint32))


def value(t) -> np.float32:
    return np.asarray(int(t), dtype=np.uint32).view(np.float32)[()]


def prev(t: int) -> int:
    return t - 1


class View:
    """What the cost depends on, from one viewpoint: s [N] float32, s_par [N] (+inf at the root), kept [N] bool."""

    def __init__(self, nodes, boxes, viewpoint, bounds=None, planes=None, radius_scale=1.0):
        self.nodes = nodes = np.asarray(nodes)
        N = nodes.shape[0]
        self.boxes = boxes = np.asarray(boxes, dtype=np.float32).reshape(N, 2, 4)
        self.viewpoint = np.asarray(viewpoint, dtype=np.float32)
        self.s = lo.node_size(boxes, np.arange(N), viewpoint)
        par = nodes[:, 1].astype(np.int64)
        self.s_par = np.where(par >= 0, self.s[np.maximum(par, 0)], F(np.inf)).astype(np.float32)
        if planes is None:
            self.kept = np.ones(N, dtype=bool)
        else:
            self.kept = ~fs.culled_spec(nodes, bounds, np.arange(N), planes, radius_scale)
        self.L = nodes[:, 3].astype(np.int64)
        self.M = nodes[:, 4].astype(np.int64)
        # m_p: the smallest s_c over p's children c with kept_c and L_c + M_c > 0 (+inf: there is none)
        self.m = np.full(N, np.inf, dtype=np.float32)
        has = np.zeros(N, dtype=bool)
        ok = (par >= 0) & self.kept & (self.L + self.M > 0)
        np.minimum.at(self.m, par[ok], self.s[ok])
        has[par[ok]] = True
        self.has_child_rows = has

    def nested(self) -> bool:
        return bool(np.all(self.s <= self.s_par))


def entries_formula(v: View, tau) -> int:
    tau = F(tau)
    k = v.kept.astype(np.int64)
    return int(np.sum(k * ((v.s_par >= tau) * (v.L + v.M) - (v.s >= tau) * v.M)))


def parents_formula(v: View, tau) -> int:
    """Interior nodes p some kept child of which is in the cut with weight < 1: s_p >= tau, s_p < 2 tau, m_p < tau."""
    tau = F(tau)
    with np.errstate(over="ignore"):
        two_tau = F(2.0) * tau
    return int(np.sum(v.has_child_rows & (v.s >= tau) & (v.s < two_tau) & (v.m < tau)))


def rows_formula(v: View, tau) -> int:
    return entries_formula(v, tau) + parents_formula(v, tau)


class Events:
    """cost(t) = the sum of the values of the events with key >= t."""

    def __init__(self, v: View, cost: str):
        assert cost in ("entries", "rows")
        k = v.kept.astype(np.int64)
        keys = [v.s_par.view(np.uint32), v.s.view(np.uint32)]
        vals = [(v.L + v.M) * k, -v.M * k]
        if cost == "rows":
            e = np.maximum(F(0.5) * v.s, v.m)
            on = v.has_child_rows & (e < v.s)
            keys += [v.s[on].view(np.uint32), e[on].view(np.uint32)]
            vals += [np.ones(int(on.sum()), np.int64), -np.ones(int(on.sum()), np.int64)]
        keys = np.concatenate(keys).astype(np.int64)
        vals = np.concatenate(vals)
        keep = vals != 0
        order = np.argsort(keys[keep], kind="stable")
        self.keys = keys[keep][order]
        self.vals = vals[keep][order]
        # suffix[i] = sum of vals[i:]
        self.suffix = np.concatenate([np.cumsum(self.vals[::-1])[::-1], [0]]).astype(np.int64)

    def cost(self, t) -> int:
        """Brute force: add up every event at or above bit pattern ``t``."""
        return int(self.vals[self.keys >= int(t)].sum())

    def cost_fast(self, t):
        return self.suffix[np.searchsorted(self.keys, np.asarray(t, dtype=np.int64), side="left")]

    def is_monotone(self, tau_min) -> bool:
        """Does the cost never rise with tau on [tau_min, +inf)?"""
        lo_t = bits(tau_min)
        ts = np.unique(np.concatenate([[lo_t], self.keys[self.keys >= lo_t], self.keys[self.keys >= lo_t] + 1]))
        ts = ts[ts <= INF_BITS + 1]
        c = self.cost_fast(ts)
        return bool(np.all(np.diff(c) <= 0))

    def smallest_fit(self, tau_min, budget):
        """The smallest bit pattern t >= bits(tau_min) with cost(t) <= budget (None: there is none): the cost only
        changes just above a key."""
        lo_t = bits(tau_min)
        ts = np.unique(np.concatenate([[lo_t], self.keys[self.keys >= lo_t] + 1]))
        ts = ts[ts <= INF_BITS]
        fit = ts[self.cost_fast(ts) <= budget]
        return int(fit[0]) if fit.size else None


class Capacity(Exception):
    """The coarsest cut (tau = +inf) costs more than the budget; ``.cost`` is that cost."""

    def __init__(self, cost):
        super().__init__(f"the coarsest cut costs {cost}")
        self.cost = cost


def descent(ev: Events, tau_min, budget, shifts=SHIFTS):
    """-> (bit pattern of tau*, cost(tau*)).  Rule 3: the request fits -> tau_min.  Else the radix descent: the
    invariant cost(lo) > budget >= cost(hi) from lo = bits(tau_min), hi = bits(+inf); per digit (step 2^sh) the cost at
    the multiples of the step inside (lo, hi] -- hi is one -- lo to the highest that violates the budget (stays if none
    does), hi to the next multiple above the new lo."""
    lo_t, hi_t = bits(tau_min), INF_BITS
    c_lo = ev.cost(lo_t)
    if c_lo <= budget:
        return lo_t, c_lo
    c_inf = ev.cost(hi_t)
    if c_inf > budget:
        raise Capacity(c_inf)
    for sh in shifts:
        first = ((lo_t >> sh) + 1) << sh
        bounds = np.arange(first, hi_t + 1, 1 << sh, dtype=np.int64)
        assert bounds.size and bounds[-1] == hi_t, (lo_t, hi_t, sh)
        c = ev.cost_fast(bounds)
        bad = np.nonzero(c[:-1] > budget)[0]
        if bad.size:
            lo_t, hi_t = int(bounds[bad[-1]]), int(bounds[bad[-1] + 1])
        else:
            hi_t = int(bounds[0])
        assert ev.cost(lo_t) > budget >= ev.cost(hi_t)
    assert hi_t == lo_t + 1
    return hi_t, ev.cost(hi_t)


def oracle_counts(nodes, boxes, tau, viewpoint, bounds=None, planes=None, radius_scale=1.0):
    """(entries, distinct parent rows of entries with w < 1, distinct rows) of the oracle's cut at ``tau`` minus the
    culled entries: what the formulas must equal."""
    nodes = np.asarray(nodes)
    r, p, ni = lo.expand_to_size(nodes, boxes, tau, viewpoint)
    if len(ni) == 0:
        return 0, 0, 0
    with np.errstate(over="ignore"):            # (2 tau at tau = FLT_MAX)
        w, _ = lo.get_interpolation_weights(ni, tau, nodes, boxes, viewpoint)
    if planes is not None:
        keep = ~fs.culled_spec(nodes, bounds, ni, planes, radius_scale)
        r, p, w = r[keep], p[keep], w[keep]
    par_rows = np.unique(p[w < F(1.0)])
    return int(len(r)), int(len(par_rows)), int(len(np.unique(np.concatenate([r, par_rows]))))


def probe_taus(v: View, count=40, seed=0):
    """About ``count`` granularities: node sizes and the values one ulp either side of them, halves of sizes, the
    ends of the range and a few values in between."""
    g = np.random.default_rng(seed)
    s = v.s[np.isfinite(v.s) & (v.s < lo.FLT_MAX)]
    out = [F(0.0), F(np.inf), lo.FLT_MAX]
    if s.size:
        pick = g.choice(s, size=min(s.size, count // 4), replace=False)
        for x in pick:
            out += [x, np.nextafter(x, F(np.inf)), np.nextafter(x, F(0.0)), F(0.5) * x]
        out += list(np.exp(g.uniform(np.log(max(float(s.min()), 1e-6)), np.log(float(s.max()) * 2 + 1e-6), 6)).astype(F))
    return [F(x) for x in out]
