"""``slots="half"`` end to end (hgs/residency.py; csrc/residency.hip: resid_fetch_half_slots_kernel; csrc/preprocess.hip:
preprocess_fwd_lod_half_kernel) on the 2 000-leaf hierarchy of test_half_rows_gpu.py.

At an equal ROW budget a viewer with half slots is the ``rows="half"`` viewer with float slots: the slots hold the bits
the float slots hold widened, widening is exact and the interpolation stays in float32 -- every selection and every image
bit for bit, at 124 instead of 236 bytes a slot.  At an equal budget in MEGABYTES the half slots are 1.90 times as many,
and ``fit="budget"`` turns them into a finer cut: the granularities below were first computed without a GPU from
tests/budget_cut_spec.py (profiles/f16_half_slots.md holds the six pairs)."""
import pytest
import torch

import test_half_rows_gpu as hr
import test_residency_gpu as rg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["generous", "quarter", "frustum", "fit_budget"])
def test_half_slots_render_what_float_slots_render_at_equal_rows(gpu, mode):
    h, attrs, rounded = hr._scene()
    nodes, boxes = h.nodes.to(gpu), h.boxes.to(gpu)
    G = attrs["means3D"].shape[0]
    need = hr._largest_view_rows(gpu, rounded, nodes, boxes)
    budget = {"generous": G, "quarter": need // 4, "frustum": need, "fit_budget": need // 4}[mode]
    run = dict(use_frustum=mode == "frustum", fit="budget" if mode == "fit_budget" else "regulate")
    half = hr._make(attrs, gpu, "half", budget_rows=budget, slots="half")
    flt = hr._make(attrs, gpu, "half", budget_rows=budget)
    assert half.B == flt.B == min(budget, G) and (half.row_bytes, flt.row_bytes) == (124, 236)
    assert half.budget_bytes * 236 == flt.budget_bytes * 124
    assert half.host_row_bytes == flt.host_row_bytes == 128
    for k in ("shs", "opacities", "scales", "rotations"):
        assert getattr(half, k).dtype == torch.float16 and getattr(flt, k).dtype == torch.float32
        assert getattr(half, k).shape == getattr(flt, k).shape
    assert half.means3D.dtype == torch.float32
    # free slots are initialised as the float slots are: scale 1, rotation (1, 0, 0, 0)
    assert torch.equal(half.scales.float(), flt.scales) and torch.equal(half.rotations.float(), flt.rotations)
    a, b = hr._fly(half, gpu, nodes, boxes, **run), hr._fly(flt, gpu, nodes, boxes, **run)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["ints"] == y["ints"] and x["tau"] == y["tau"], (mode, k, x["ints"], y["ints"], x["tau"], y["tau"])
        for key in ("ri", "pi", "kids", "radii"):
            assert torch.equal(x[key], y[key]), (mode, k, key)
        assert torch.equal(x["w"].view(torch.int32), y["w"].view(torch.int32)), (mode, k)
        assert torch.equal(x["color"], y["color"]), (mode, k)
        assert float(x["color"].max()) > 0.0
    if mode in ("quarter", "fit_budget"):
        assert any(r["tau"] > tau for r, (_, tau) in zip(a, rg._views())), "the small budget did not coarsen any view"
    sh, sf = half.stats, flt.stats
    assert sh["rows_fetched"] == sf["rows_fetched"] > 0 and sh["evictions"] == sf["evictions"]
    assert sh["bytes_fetched"] == sf["bytes_fetched"] == 128 * sh["rows_fetched"]
    assert int((half.slot_of == -2).sum()) == 0
    # what the slots hold is what the float slots hold, narrowed back without loss
    torch.cuda.synchronize()
    ids = torch.nonzero(half.slot_of >= 0).reshape(-1)
    assert torch.equal(ids, torch.nonzero(flt.slot_of >= 0).reshape(-1)), "another set of rows is resident"
    sh_, sf_ = half.slot_of[ids].long(), flt.slot_of[ids].long()       # (which slot a row got follows the miss list's order)
    for k in ("shs", "opacities", "scales", "rotations"):
        assert torch.equal(getattr(half, k)[sh_].float(), getattr(flt, k)[sf_]), k
    assert torch.equal(half.means3D[sh_], flt.means3D[sf_])


def test_the_same_megabytes_buy_a_finer_cut(gpu):
    """``budget_mb`` chosen so that float slots get need // 4 rows: half slots get int(budget_mb * 1e6 // 124), and under
    fit="budget" every view is rendered at a granularity no coarser than with float slots -- finer for at least one."""
    h, attrs, rounded = hr._scene()
    nodes, boxes = h.nodes.to(gpu), h.boxes.to(gpu)
    need = hr._largest_view_rows(gpu, rounded, nodes, boxes)
    rows_float = need // 4
    budget_mb = (rows_float * 236 + 118) / 1e6                    # (mid-row: no rounding of the product decides the count)
    half = hr._make(attrs, gpu, "half", budget_mb=budget_mb, slots="half")
    flt = hr._make(attrs, gpu, "half", budget_mb=budget_mb)
    assert flt.B == rows_float and half.B == int(budget_mb * 1e6 // 124)
    assert 1.89 < half.B / flt.B < 1.92
    assert half.budget_bytes <= budget_mb * 1e6 and flt.budget_bytes <= budget_mb * 1e6
    a = hr._fly(half, gpu, nodes, boxes, fit="budget")
    b = hr._fly(flt, gpu, nodes, boxes, fit="budget")
    taus = [(x["tau"], y["tau"]) for x, y in zip(a, b)]
    print("tau rendered per view (half slots, float slots) at", budget_mb, "MB:", taus)
    for k, ((th, tf), (_, request)) in enumerate(zip(taus, rg._views())):
        assert request <= th <= tf, (k, th, tf)
        assert a[k]["ints"][3] <= half.B and b[k]["ints"][3] <= flt.B          # the cost each cut was counted at
        assert float(a[k]["color"].max()) > 0.0
    assert any(th < tf for th, tf in taus), taus
