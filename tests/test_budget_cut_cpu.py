"""The budget-exact cut without a GPU (tests/budget_cut_spec.py restates it): the cost formulas against the LOD oracle
and the frustum spec, the radix descent against rules 1 to 3 of include/hgs.h and against the brute-force minimum where
the cost is monotone, and the static resources of the new kernels."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import budget_cut_cases as bc
import budget_cut_spec as bs
from hgs import frustum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _views(nodes, boxes, bounds, name):
    """(camera, [(label, View)]): the plain view and the culled one."""
    cam, planes, rs = bc.planes_of(name)
    vp = cam.camera_center.numpy()
    return cam, vp, planes, rs, (("plain", bs.View(nodes, boxes, vp)),
                                 ("culled", bs.View(nodes, boxes, vp, bounds, planes, rs)))


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("P", bc.CPU_LEAVES)
def test_formulas_equal_the_oracle_counts(P, name):
    nodes, boxes, bounds, _, _ = bc.built(P)
    cam, vp, planes, rs, views = _views(nodes, boxes, bounds, name)
    ups = 0
    for label, v in views:
        assert v.nested()
        kw = dict(bounds=bounds, planes=planes, radius_scale=rs) if label == "culled" else {}
        taus = bs.probe_taus(v, 40, seed=P)
        assert len(taus) >= 40 or P < 33
        ev_e, ev_r = bs.Events(v, "entries"), bs.Events(v, "rows")
        last = None
        for tau in sorted(taus):
            e, par, rows = bs.oracle_counts(nodes, boxes, tau, vp, **kw)
            assert (bs.entries_formula(v, tau), bs.parents_formula(v, tau), bs.rows_formula(v, tau)) == (e, par, rows), \
                (P, name, label, float(tau))
            assert (ev_e.cost(bs.bits(tau)), ev_r.cost(bs.bits(tau))) == (e, rows), (P, name, label, float(tau))
            ups += last is not None and rows > last
            last = rows
        if label == "plain":
            assert ev_e.is_monotone(0.0)                # nesting: s_par >= s_n in float32
    print(f"P {P} camera {name}: upward steps of rows(tau) over the samples: {ups}")


@pytest.mark.parametrize("name", ["A", "B"])
def test_formulas_on_nodes_of_several_rows(name):
    """Hand-built nested hierarchy: several rows per node, a node without rows, and a node with children that owns
    leaf rows -- there ``rows`` may count the parent row twice and is only required to be an upper bound."""
    nodes, boxes, bounds, _, _ = bc.multi_row()
    cam, vp, planes, rs, views = _views(nodes, boxes, bounds, name)
    strict = 0
    for label, v in views:
        assert v.nested()
        kw = dict(bounds=bounds, planes=planes, radius_scale=rs) if label == "culled" else {}
        for tau in bs.probe_taus(v, 40, seed=1):
            e, par, rows = bs.oracle_counts(nodes, boxes, tau, vp, **kw)
            assert bs.entries_formula(v, tau) == e and bs.parents_formula(v, tau) == par
            assert bs.rows_formula(v, tau) >= rows
            strict += bs.rows_formula(v, tau) > rows
            assert bs.Events(v, "rows").cost(bs.bits(tau)) == bs.rows_formula(v, tau)
    print("samples where rows(tau) exceeds the distinct rows:", strict)


def _check_descent(ev, tau_min, budget, c_inf):
    t_min = bs.bits(tau_min)
    if budget < c_inf:
        with pytest.raises(bs.Capacity) as e:
            bs.descent(ev, tau_min, budget)
        assert e.value.cost == c_inf
        return None
    t, c = bs.descent(ev, tau_min, budget)
    assert t >= t_min and c == ev.cost(t) and c <= budget                       # rule 1
    assert t == t_min or ev.cost(bs.prev(t)) > budget                           # rule 2
    if ev.cost(t_min) <= budget:                                                # rule 3
        assert t == t_min
    if ev.is_monotone(tau_min):                                                 # rule 5
        assert t == ev.smallest_fit(tau_min, budget)
    return t


@pytest.mark.parametrize("P", bc.CPU_LEAVES + ("multi",))
def test_descent_keeps_the_rules(P):
    nodes, boxes, bounds, _, _ = bc.multi_row() if P == "multi" else bc.built(P)
    N = len(nodes)
    ran = mono = 0
    for name in "ABC":
        cam, vp, planes, rs, views = _views(nodes, boxes, bounds, name)
        for label, v in views:
            for cost in ("entries", "rows"):
                ev = bs.Events(v, cost)
                c_inf = ev.cost(bs.INF_BITS)
                assert c_inf == int(v.kept[0]) * int(v.L[0] + v.M[0])           # the root's kept rows
                for px in bc.TAU_MINS_PX:
                    tau_min = bc.tau_min_of(cam, px)
                    mono += ev.is_monotone(tau_min)
                    for budget in bc.budgets(N, c_inf):
                        ran += _check_descent(ev, tau_min, budget, c_inf) is not None
                # (a builder or merger hierarchy: a node's merged rows stand for at least as many rows below it; the
                # hand-built one has a childless node with a merged row, whose count RISES when it turns fine)
                if cost == "entries" and label == "plain" and P != "multi":
                    assert ev.is_monotone(0.0)
    print(f"{P}: {ran} descents, {mono} monotone (cost, request) pairs")
    assert ran > 0


def test_descent_at_interior_keys_and_the_ends():
    """A budget of exactly cost(t) and cost(t) - 1 at interior keys; tau_min = +inf; a key of FLT_MAX (camera inside)."""
    nodes, boxes, bounds, _, _ = bc.built(129)
    cam, vp, planes, rs, views = _views(nodes, boxes, bounds, "B")
    for label, v in views:
        for cost in ("entries", "rows"):
            ev = bs.Events(v, cost)
            c_inf = ev.cost(bs.INF_BITS)
            keys = np.unique(ev.keys[ev.keys < bs.INF_BITS])
            for t in keys[[len(keys) // 4, len(keys) // 2, 3 * len(keys) // 4]]:
                for budget in (ev.cost(int(t)), ev.cost(int(t)) - 1):
                    if budget >= 0:
                        _check_descent(ev, 0.0, budget, c_inf)
            assert bs.descent(ev, np.inf, c_inf) == (bs.INF_BITS, c_inf)


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("c++filt")),
                    reason="needs hipcc (cross-compiles without a GPU) and c++filt")
def test_no_budget_kernel_uses_scratch_or_doubles():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    rows = kernel_resources.collect([os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc", "lod_budget.hip")])
    names = {r["kernel"] for r in rows}
    assert {"budget_size_kernel", "budget_parent_kernel", "budget_hist_kernel", "budget_pick_kernel",
            "budget_mark_kernel", "budget_scan_sums_kernel", "budget_emit_kernel"} <= names, names
    for r in rows:
        assert r["scratch"] == 0, (r["kernel"], r["scratch"])
        assert r["mix"]["valu_f64"] == 0, r["kernel"]
        assert r["waves_regs"] >= 8, (r["kernel"], r["vgpr"])


def test_cut_to_budget_refuses_bad_arguments_without_touching_the_gpu():
    nodes = torch.zeros(3, 7, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU tensor"):
        frustum.cut_to_budget(nodes, torch.zeros(3, 2, 4), None, 10, torch.zeros(3))
    assert {"tau", "cost", "n", "n_unculled", "weights", "kids"} <= set(frustum.BudgetCut.__dataclass_fields__)
    assert issubclass(frustum.BudgetCut, frustum.CutView)


def test_the_c_abi_refuses_bad_arguments_before_any_hip_call():
    """NULL pointers, N <= 0, budget < 0, a negative or NaN tau_min, an unknown cost and capacity < budget: refused on
    the host (this machine may have no GPU at all: the calls must not get as far as needing one)."""
    import ctypes as C
    from hgs import _lib
    lib = _lib.lib()
    assert lib.hgs_lod_cut_budget_tmp_bytes(1000) >= 3 * 4000 + 2048 * 4 + 48
    assert lib.hgs_lod_cut_budget_tmp_bytes(0) == lib.hgs_lod_cut_budget_tmp_bytes(1)
    buf = (C.c_int32 * 64)()
    a = C.cast(buf, C.c_void_p)
    vp = (C.c_float * 3)(0, 0, 0)
    pl = (C.c_float * 20)()
    n, na, tau, cst = C.c_int32(7), C.c_int32(7), C.c_float(7), C.c_int32(7)

    def call(nodes=a, boxes=a, bounds=None, N=4, tau_min=0.0, budget=4, mode=1, planes=None, out=a, cap=8, tmp=a,
             res=(n, na, tau, cst)):
        r = [C.byref(x) if x is not None else None for x in res]
        return lib.hgs_lod_cut_budget(nodes, boxes, bounds, N, tau_min, budget, mode, vp, planes, 1.0, out, out, out, out,
                                      out, cap, tmp, r[0], r[1], r[2], r[3], None, 0)

    for kw, word in ((dict(nodes=None), b"null"), (dict(boxes=None), b"null"), (dict(out=None), b"null"),
                     (dict(tmp=None), b"null"), (dict(res=(n, na, None, cst)), b"null"), (dict(N=0), b"N = 0"),
                     (dict(N=-3), b"N = -3"), (dict(budget=-1), b"budget = -1"), (dict(tau_min=-1.0), b"tau_min"),
                     (dict(tau_min=float("nan")), b"tau_min"), (dict(mode=2), b"cost_mode"),
                     (dict(budget=9, cap=8), b"budget of 9"), (dict(bounds=a), b"go together"),
                     (dict(planes=pl), b"go together")):
        assert call(**kw) == 1, kw
        assert word in lib.hgs_last_error(), (kw, lib.hgs_last_error())
