"""``rows="half"`` end to end (hgs/residency.py, csrc/residency.hip: resid_fetch_half_kernel, resid_pack_kernel; DESIGN.md
section 7 f-14) on a hierarchy of 2 000 leaves from the project's builder.  The property: a hierarchy with half host
rows is, for the viewer, the hierarchy with float host rows built from ``round_rows_to_half`` of the same arrays -- every
selection and every image bit for bit, at half the bytes over PCIe.  How far that is from the UNROUNDED float render is
measured (a PSNR, printed), not asserted: profiles/f14_half_rows.md holds the figures."""
import functools
import math

import numpy as np
import pytest
import torch

import half_rows_cases as hc
import test_residency_gpu as rg
from hgs import hierarchy, residency, synth
from hgs.residency import BudgetedHierarchy

pytestmark = pytest.mark.gpu
W, H = rg.W, rg.H
KEYS = ("means3D", "shs", "opacities", "scales", "rotations")


@functools.lru_cache(maxsize=None)
def _scene():
    """(hierarchy, attributes as CPU tensors, the same rounded to half): computed once, never modified."""
    h = hierarchy.build_hierarchy(synth.make_scene(2_000, synth.make_camera(W, H), seed=8))
    attrs = dict(means3D=h.xyz, shs=h.shs, opacities=h.alpha.abs().reshape(-1, 1), scales=torch.exp(h.log_scales),
                 rotations=torch.nn.functional.normalize(h.rots))
    rounded = dict(zip(KEYS, residency.round_rows_to_half(*[attrs[k] for k in KEYS])))
    return h, attrs, rounded


def _make(attrs, gpu, rows, **kw):
    return BudgetedHierarchy(*[attrs[k] for k in KEYS], gpu, rows=rows, **kw)


def _planes(cam):
    from hgs.frustum import frustum_planes
    return frustum_planes(cam.world_view_transform, cam.tanfovx, cam.tanfovy, W, H)


def _fly(bh, gpu, nodes, boxes, use_frustum=False, fit="regulate"):
    """The six views of test_residency_gpu.py through select -> render -> prefetch of the next view: per view the
    Selection's integers and tau, the row ids its slot tensors name, weights and sibling counts, the image and radii."""
    views = rg._views()
    kws = [dict(fit=fit, **(dict(frustum=_planes(cam)) if use_frustum else {})) for cam, _ in views]
    vp = lambda cam: (cam.camera_center.to(gpu), cam.camera_center.cpu())
    out = []
    for k, (cam, tau) in enumerate(views):
        sel = bh.select(nodes, boxes, tau, *vp(cam), **kws[k])
        arrays = {key: getattr(bh, key) for key in KEYS}
        color, radii = rg._render(gpu, cam, arrays, sel.render_indices, sel.parent_indices, sel.weights, sel.kids)
        ids = bh.id_of_slot.long()
        rec = dict(ints=(sel.n, sel.misses, sel.attempts, sel.cost), tau=sel.tau, color=color.clone(), radii=radii.clone(),
                   ri=ids[sel.render_indices.long()].clone(), pi=ids[sel.parent_indices.long()].clone(),
                   w=sel.weights[:sel.n].clone(), kids=sel.kids[:sel.n].clone())
        if k + 1 < len(views):
            nxt_cam, nxt_tau = views[k + 1]
            bh.prefetch(nodes, boxes, nxt_tau, *vp(nxt_cam), **kws[k + 1])
        out.append(rec)
    torch.cuda.synchronize()
    return out


def _largest_view_rows(gpu, attrs, nodes, boxes):
    full = {k: v.to(gpu).contiguous() for k, v in attrs.items()}
    return max(rg._reference(gpu, cam, full, nodes, boxes, tau)[3] for cam, tau in rg._views())


@pytest.mark.parametrize("mode", ["generous", "quarter", "frustum", "fit_budget"])
def test_half_rows_render_what_float_rows_of_the_rounded_arrays_render(gpu, mode):
    h, attrs, rounded = _scene()
    nodes, boxes = h.nodes.to(gpu), h.boxes.to(gpu)
    G = attrs["means3D"].shape[0]
    need = _largest_view_rows(gpu, rounded, nodes, boxes)
    budget = {"generous": G, "quarter": need // 4, "frustum": need, "fit_budget": need // 4}[mode]
    run = dict(use_frustum=mode == "frustum", fit="budget" if mode == "fit_budget" else "regulate")
    half = _make(attrs, gpu, "half", budget_rows=budget)
    flt = _make(rounded, gpu, "float", budget_rows=budget)
    assert half.B == flt.B and half.row_bytes == flt.row_bytes == 4 * (3 * 16 + 11)      # a budget buys the same rows
    assert (half.host_row_bytes, flt.host_row_bytes) == (128, 256)
    assert half._rows.nbytes == G * 128 and flt._rows.nbytes == G * 256
    a, b = _fly(half, gpu, nodes, boxes, **run), _fly(flt, gpu, nodes, boxes, **run)
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
    assert sh["bytes_fetched"] == 128 * sh["rows_fetched"] and sf["bytes_fetched"] == 256 * sf["rows_fetched"]
    assert 2 * sh["bytes_fetched"] == sf["bytes_fetched"]
    assert int((half.slot_of == -2).sum()) == 0


@pytest.mark.parametrize("rows", ["float", "half"])
def test_from_device_arrays_writes_the_constructors_host_rows(gpu, rows):
    h, attrs, _ = _scene()
    cpu = _make(attrs, gpu, rows, budget_rows=100)
    dev = BudgetedHierarchy.from_device_arrays(*[attrs[k].to(gpu) for k in KEYS], rows=rows, budget_rows=100)
    assert dev._rows.shape == cpu._rows.shape and dev._rows.dtype == cpu._rows.dtype
    assert np.array_equal(dev._rows.view(np.uint8), cpu._rows.view(np.uint8))
    assert (dev.G, dev.M, dev.B, dev.host_row_bytes, dev.dev) == (cpu.G, cpu.M, cpu.B, cpu.host_row_bytes, cpu.dev)
    # and it serves a view: the same image as the constructor's hierarchy
    nodes, boxes = h.nodes.to(gpu), h.boxes.to(gpu)
    big_c = _make(attrs, gpu, rows, budget_rows=cpu.G)
    big_d = BudgetedHierarchy.from_device_arrays(*[attrs[k].to(gpu) for k in KEYS], rows=rows, budget_rows=cpu.G)
    x, y = _fly(big_d, gpu, nodes, boxes)[0], _fly(big_c, gpu, nodes, boxes)[0]
    assert x["ints"] == y["ints"] and torch.equal(x["color"], y["color"])
    with pytest.raises(ValueError, match="from_device_arrays"):
        _make({k: v.to(gpu) for k, v in attrs.items()}, gpu, rows, budget_rows=100)


def test_hier_file_written_in_half_to_half_rows(gpu, tmp_path):
    """write_hierarchy(half=True) -> from_hier_file(rows="half") renders what rows="float" renders from the rounded
    activations of the same file."""
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    h, _, _ = _scene()
    path = str(tmp_path / "scene_half.hier")
    write_hierarchy(path, h.xyz, h.shs, h.alpha, h.log_scales, h.rots, h.nodes, h.boxes, half=True)
    G = h.xyz.shape[0]
    bh, nodes, boxes = BudgetedHierarchy.from_hier_file(path, gpu, budget_rows=G, rows="half")
    assert bh.host_row_bytes == 128 and torch.equal(nodes.cpu(), h.nodes) and torch.equal(boxes.cpu(), h.boxes)
    xyz, shs, alpha, log_scales, rots, _, _ = load_hierarchy(path)
    loaded = dict(means3D=xyz, shs=shs, opacities=alpha.abs(), scales=torch.exp(log_scales),
                  rotations=torch.nn.functional.normalize(rots))
    flt = _make(dict(zip(KEYS, residency.round_rows_to_half(*[loaded[k] for k in KEYS]))), gpu, "float", budget_rows=G)
    x, y = _fly(bh, gpu, nodes, boxes)[0], _fly(flt, gpu, nodes, boxes)[0]
    assert x["ints"] == y["ints"] and x["tau"] == y["tau"]
    assert torch.equal(x["color"], y["color"]) and float(x["color"].max()) > 0.0


def test_half_rows_differ_from_unrounded_float_rows_and_by_how_much(gpu):
    """Condition: the half render is NOT the unrounded float render (the half path ran).  Measurement, printed and not
    asserted (no bar was fixed in advance; profiles/f14_half_rows.md): the PSNR between the two at every view."""
    h, attrs, _ = _scene()
    nodes, boxes = h.nodes.to(gpu), h.boxes.to(gpu)
    G = attrs["means3D"].shape[0]
    a = _fly(_make(attrs, gpu, "half", budget_rows=G), gpu, nodes, boxes)
    b = _fly(_make(attrs, gpu, "float", budget_rows=G), gpu, nodes, boxes)
    psnr = []
    for x, y in zip(a, b):
        assert x["ints"] == y["ints"]                                   # (the mean is not narrowed: the same cut)
        mse = float(((x["color"].double() - y["color"].double()) ** 2).mean())
        psnr.append(math.inf if mse == 0.0 else 10.0 * math.log10(1.0 / mse))
    print("PSNR of rows='half' against rows='float' (peak 1.0), 2 000 leaves, six views:", [round(p, 2) for p in psnr])
    assert any(not torch.equal(x["color"], y["color"]) for x, y in zip(a, b))


def test_a_partial_best_effort_pass_brings_in_the_lowest_missing_rows(gpu):
    """What a prefetch that cannot fit its whole miss list leaves resident must not depend on the order in which the mark
    pass queued the rows (the order of its atomics): otherwise two hierarchies fed the same views fetch and evict
    differently later, and ``bytes_fetched`` of a half and a float hierarchy are no longer comparable.  Ten slots, six
    taken by the frame; a best-effort pass for eight other rows, given in descending order, gets the four lowest."""
    G, M = 100, 2
    a = [torch.from_numpy(x) for x in hc.attribute_arrays(G, M, seed=2, with_cases=False)]
    for rows in ("half", "float"):
        bh = BudgetedHierarchy(*a, gpu, budget_rows=10, index_capacity=16, rows=rows)
        t = lambda ids: torch.tensor(ids, dtype=torch.int32, device=gpu)
        frame = t([50, 51, 52, 53, 54, 55])
        ro, po, m = bh.make_resident(frame, frame)
        assert m == 6 and bh.free_top == 4
        want = t([97, 90, 88, 71, 64, 33, 20, 9])
        ro, po, m = bh.make_resident(want, want, _new_frame=False, _best_effort=True)
        torch.cuda.synchronize()
        assert ro is None and m == 4 and bh.free_top == 0
        resident = torch.nonzero(bh.slot_of >= 0).reshape(-1).tolist()
        assert resident == [9, 20, 33, 50, 51, 52, 53, 54, 55, 64], resident
        assert int((bh.slot_of == -2).sum()) == 0 and bh.stats["bytes_fetched"] == 10 * bh.host_row_bytes
