"""Leaf removal on the device (csrc/hier_prune.hip through hgs.hierarchy.prune_hierarchy_gpu and the C ABI) against the
numpy spec hgs.hierarchy.prune_hierarchy: sizes on both sides of a wave, a workgroup and a scan chunk, six removal masks,
three SH widths, the three re-merge modes, each criterion alone and all together, guarded workspaces and outputs, a tail
behind N, unaligned bases, determinism, the refusals with untouched outputs, cuts and a render of the result, the command.
Records, boxes, maps, counts and every copied row are compared bit for bit; re-merged rows within the builder's bounds
(tests/test_hier_build_gpu.py): mean, SH and opacity within parity.assert_stats at 1e-5, covariance within 1e-5 Frobenius
per node, unit quaternions to 1e-6, ascending eigenvalues.  Covariances are compared, not frames."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import frustum_cases as fc
import parity as pa
import ws_guard as wg
from hgs import _lib, hierarchy, synth
from test_hier_prune_cpu import MASKS, SIZES, case, dirty_new, pruned, removal_mask
from test_hier_refit_cpu import nested_np
from test_hier_trim_cpu import ARRAYS, CAM, VIEWS, bits, check_layout, oracle_cut, scene2000
from test_hier_trim_gpu import AbiRun, _gpu_cuts, _render, _stream, to_dev

pytestmark = pytest.mark.gpu
ROWS = ARRAYS[:5]
COUNTS = ("removed_leaves", "dead", "dirty", "single_child")


def with_width(h, M):
    return h if M == 16 else hierarchy.Hierarchy(h.xyz, h.shs[:, :M].contiguous(), h.alpha, h.log_scales, h.rots, h.nodes, h.boxes)


def cov_rows(log_scales, rots):
    q = rots.double().numpy()
    R = hierarchy._rot_from_quat(q / np.linalg.norm(q, axis=1, keepdims=True))
    return (R * np.exp(2.0 * log_scales.double().numpy())[:, None, :]) @ R.transpose(0, 2, 1)


def assert_within_builders_bounds(name, got, want, sel):
    """Rows ``sel`` (bool [n]) of two host hierarchies: the builder's bounds."""
    if not bool(sel.any()):
        return
    s = torch.from_numpy(sel)
    stats = {k: pa.err_stats(getattr(got, k)[s], getattr(want, k)[s]) for k in ("xyz", "shs", "alpha")}
    print(name, {k: (v["maxrel"], v["l2"]) for k, v in stats.items()})
    pa.assert_stats(name, stats, rel_tol=1e-5)
    assert float((got.rots[s].double().norm(dim=1) - 1).abs().max()) <= 1e-6, name
    ls = got.log_scales[s]
    assert bool((ls[:, 0] <= ls[:, 1]).all()) and bool((ls[:, 1] <= ls[:, 2]).all()), name
    cg, cw = cov_rows(got.log_scales[s], got.rots[s]), cov_rows(want.log_scales[s], want.rots[s])
    rel = np.linalg.norm(cg - cw, axis=(1, 2)) / np.linalg.norm(cw, axis=(1, 2))
    print(name, "covariance", float(rel.max()))
    assert float(rel.max()) <= 1e-5, (name, float(rel.max()), int(rel.argmax()))


def assert_equals_spec(name, got_h, got_maps, want, recomputed):
    """got_h: a host Hierarchy; got_maps: (old_of_new, new_of_old) on the host; want: the spec's PruneResult;
    recomputed: bool [N'], the rows the mode computes again (all others are bit copies on both sides)."""
    wh = want.hierarchy
    for k in ARRAYS:
        a, b = getattr(got_h, k), getattr(wh, k)
        assert a.shape == b.shape and a.dtype == b.dtype, (name, k, a.shape, b.shape)
    assert torch.equal(got_h.nodes, wh.nodes) and torch.equal(bits(got_h.boxes), bits(wh.boxes)), name
    assert got_maps[0].dtype == torch.int32 and torch.equal(got_maps[0], want.old_of_new), name
    assert got_maps[1].dtype == torch.int32 and torch.equal(got_maps[1], want.new_of_old), name
    copied = torch.from_numpy(~recomputed)
    for k in ROWS:
        assert torch.equal(bits(getattr(got_h, k)[copied]), bits(getattr(wh, k)[copied])), (name, k)
    assert_within_builders_bounds(name, got_h, wh, recomputed)


def host(h):
    return hierarchy.Hierarchy(*(getattr(h, k).cpu() for k in ARRAYS))


def run_case(gpu, h, want, remerge="dirty", **criteria):
    got = hierarchy.prune_hierarchy_gpu(to_dev(h, gpu), remerge=remerge, **criteria)
    for k in COUNTS:
        assert getattr(got, k) == getattr(want, k), (k, getattr(got, k), getattr(want, k))
    d = dirty_new(h, want)
    inner = want.hierarchy.nodes[:, 6].numpy() > 0
    recomputed = {"dirty": d, "none": np.zeros_like(d), "all": inner}[remerge]
    assert_equals_spec(f"{remerge}", host(got.hierarchy), (got.old_of_new.cpu(), got.new_of_old.cpu()), want, recomputed)
    return got


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("P", SIZES + ("merged",))
def test_sizes_and_masks(gpu, P, kind):
    h, want = case(P), pruned(P, kind)
    mask = removal_mask(h, kind)
    if want is None:                                    # every leaf goes: refused, as by the spec
        with pytest.raises(hierarchy.HierarchyPruneError) as e:
            hierarchy.prune_hierarchy_gpu(to_dev(h, gpu), remove=mask)
        assert e.value.check == hierarchy.PRUNE_ROOT_DEAD and e.value.node == 0
        return
    got = run_case(gpu, h, want, remove=mask)
    check_layout(got.hierarchy.nodes.cpu().numpy())
    run_case(gpu, h, pruned(P, kind, "none"), "none", remove=torch.from_numpy(mask).to(gpu))     # all seven: bit for bit


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("M", (1, 4))
@pytest.mark.parametrize("P", (129, "merged"))
def test_sh_widths(gpu, P, M, kind):
    h = with_width(case(P), M)
    mask = removal_mask(h, kind)
    run_case(gpu, h, hierarchy.prune_hierarchy(h, remove=mask), remove=mask)


@functools.lru_cache(maxsize=None)
def two_scan_chunks():
    """1 050 000 leaves: 2 099 999 nodes = 8 204 workgroups, one more scan chunk than 8 192 -- built on the device."""
    return hierarchy.build_hierarchy_on_device(1_050_000, CAM, torch.device("cuda", torch.cuda.current_device()), seed=3)


def carried_weights(o):
    """float64 [N']: alpha s0 s1 s2 at the leaves of a host hierarchy, the clamped sum of the children's at the others."""
    nd = o.nodes.numpy()
    s = np.exp(o.log_scales.double().numpy())
    w = np.where(nd[:, 6] == 0, o.alpha.double().numpy().reshape(-1) * ((s[:, 0] * s[:, 1]) * s[:, 2]), 0.0)
    for d in range(int(nd[:, 0].max()) - 1, -1, -1):
        ids = np.nonzero((nd[:, 0] == d) & (nd[:, 6] > 0))[0]
        if ids.size == 0:
            continue
        total = np.zeros(ids.size)
        for j in range(int(nd[ids, 6].max())):
            has = nd[ids, 6] > j
            total = total + np.where(has, w[np.where(has, nd[ids, 5] + j, nd[ids, 5])], 0.0)
        w[ids] = np.maximum(total, 1e-30)
    return w


def test_the_second_scan_chunk(gpu):
    d = two_scan_chunks()
    N = d.num_nodes
    assert (N + 255) // 256 > 8192
    h = host(d)
    mask = removal_mask(h, "every_second_leaf")
    mask[N - 40000:] = 0                                 # ... and a long clean run at the end of the index range
    want = hierarchy.prune_hierarchy(h, remove=mask, remerge="none")
    got = hierarchy.prune_hierarchy_gpu(d, remove=mask, remerge="none")
    for k in COUNTS:
        assert getattr(got, k) == getattr(want, k), k
    for k in ARRAYS:
        assert torch.equal(bits(getattr(got.hierarchy, k).cpu()), bits(getattr(want.hierarchy, k))), k
    assert torch.equal(got.old_of_new.cpu(), want.old_of_new) and torch.equal(got.new_of_old.cpu(), want.new_of_old)
    # the re-merge at this size: determinism, and a sample of the dirty rows against the spec's rule on the device's rows
    a = hierarchy.prune_hierarchy_gpu(d, remove=mask)
    b = hierarchy.prune_hierarchy_gpu(d, remove=mask)
    for k in ARRAYS:
        assert torch.equal(bits(getattr(a.hierarchy, k)), bits(getattr(b.hierarchy, k))), k
    o = host(a.hierarchy)
    nd = o.nodes.numpy()
    ids = np.nonzero(dirty_new(h, want))[0][::997]
    kids = np.concatenate([np.arange(nd[i, 5], nd[i, 5] + nd[i, 6]) for i in ids])
    t = torch.from_numpy(kids)
    m = hierarchy.merge_rows(o.xyz[t].numpy(), o.shs[t].numpy(), o.alpha[t].numpy(), o.log_scales[t].numpy(), o.rots[t].numpy(),
                             nd[ids, 6], weights=carried_weights(o)[kids])
    f = lambda k, shape: torch.from_numpy(m[k].astype(np.float32)).reshape(shape)
    n = ids.size
    ref = hierarchy.Hierarchy(f("xyz", (n, 3)), f("shs", (n, 16, 3)), f("alpha", (n, 1)), f("log_scales", (n, 3)),
                              f("rots", (n, 4)), None, None)
    s = torch.from_numpy(ids)
    sub = hierarchy.Hierarchy(o.xyz[s], o.shs[s], o.alpha[s], o.log_scales[s], o.rots[s], None, None)
    assert_within_builders_bounds("second chunk", sub, ref, np.ones(n, dtype=bool))


@pytest.mark.parametrize("P", (262_145, 300_000))
def test_the_plan_walks_second_trip(gpu, P):
    """The plan kernel's grid is capped at 2048 workgroups of 256 threads: above 524 288 nodes a workgroup goes through
    its loop a second time, with its sums in registers and its depth bins in LDS from the first.  262 145 leaves are
    524 289 nodes (the second trip holds ONE node), 300 000 leaves are 599 999 nodes (many workgroups make the trip, the
    last of them partly filled).  Built on the device; one remove box over a corner of the scene, the re-merge of the
    dirty nodes.  The numpy spec at 599 999 nodes takes 0.4 s on the CPU host these tests were written on."""
    h = host(hierarchy.build_hierarchy_on_device(P, CAM, gpu, seed=3))
    N = h.num_nodes
    assert N == 2 * P - 1 and N > 2048 * 256
    x = h.xyz.numpy()[h.nodes.numpy()[:, 6] == 0]
    box = (tuple(float(v) for v in x.min(0)), tuple(float(v) for v in np.quantile(x, 0.4, axis=0)))
    want = hierarchy.prune_hierarchy(h, remove_boxes=[box], remerge="dirty")
    print(f"{P} leaves: removed {want.removed_leaves}, dead {want.dead}, dirty {want.dirty}, single {want.single_child}")
    assert 0 < want.removed_leaves < P // 4 and want.dirty > 0
    stats = {}
    got = run_case(gpu, h, want, remove_boxes=[box], stats=stats)
    assert stats["levels"] == int(h.nodes[:, 0].max()) + 1
    assert got.hierarchy.num_nodes == N - want.dead


def parents_of_leaves(nodes):
    nd = np.asarray(nodes)
    has_inner_child = np.zeros(nd.shape[0], dtype=bool)
    inner = np.nonzero(nd[:, 6] > 0)[0]
    has_inner_child[nd[inner[inner > 0], 1]] = True
    return (nd[:, 6] > 0) & ~has_inner_child


def test_remerge_all_with_nothing_removed(gpu):
    """Every interior row again from its children's float32 rows: the spec's rows within the builder's bounds, records,
    boxes and leaves the input's bits; the parents of leaves on their own (a leaf's alpha s0 s1 s2 is the weight the
    builder gave it), all interior rows in the test below."""
    h = case(2000)
    got = run_case(gpu, h, hierarchy.prune_hierarchy(h, remerge="all"), "all")
    o = host(got.hierarchy)
    assert (got.dead, got.dirty, got.removed_leaves) == (0, 0, 0)
    assert torch.equal(o.nodes, h.nodes) and torch.equal(bits(o.boxes), bits(h.boxes))
    leaf = h.nodes[:, 6].numpy() == 0
    for k in ROWS:
        assert torch.equal(bits(getattr(o, k)[torch.from_numpy(leaf)]), bits(getattr(h, k)[torch.from_numpy(leaf)])), k
    low = parents_of_leaves(h.nodes.numpy())
    assert int(low.sum()) > 900
    assert_within_builders_bounds("parents of leaves vs the input", o, h, low)


def test_remerge_all_with_nothing_removed_stays_within_the_builders_bounds_of_the_input(gpu):
    """On the built 2 000-leaf scene with nothing removed, EVERY interior row of remerge="all" lies within the builder's
    bounds of the input's row: a node's weight is the sum over its surviving leaves of alpha s0 s1 s2, which is the
    weight the builder carried, so the re-merge reproduces the builder up to the float32 rounding of the children's
    rows (on the spec: xyz 9.5e-8, shs 1.4e-7, alpha 1.5e-7 of the largest value, covariance 1.3e-6).  With a node's
    weight taken from its OWN merged row (alpha s0 s1 s2 of a merged Gaussian) this failed with xyz 0.52, shs 0.74,
    alpha 0.57: the two are different numbers above the parents of leaves."""
    h = case(2000)
    o = host(hierarchy.prune_hierarchy_gpu(to_dev(h, gpu), remerge="all").hierarchy)
    assert_within_builders_bounds("all vs the input", o, h, h.nodes[:, 6].numpy() > 0)


# ---- the criteria ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def criteria2000():
    """One remove box with about a tenth of the leaves, an opacity floor and a scale ceiling from the scene's quantiles;
    the shares are asserted on the spec's side."""
    h = case(2000)
    nd = h.nodes.numpy()
    leaf = nd[:, 6] == 0
    x, a, ls = h.xyz.numpy()[leaf], h.alpha.numpy().reshape(-1)[leaf], h.log_scales.numpy()[leaf]
    a_, b_ = 0.0, 0.5                              # the box between the axes' quantiles 0.5 -+ m, m bisected to a tenth
    for _ in range(20):
        m = 0.5 * (a_ + b_)
        lo, hi = np.quantile(x, 0.5 - m, axis=0), np.quantile(x, 0.5 + m, axis=0)
        share = float(((x >= lo.astype(np.float32)) & (x <= hi.astype(np.float32))).all(1).mean())
        a_, b_ = (m, b_) if share < 0.1 else (a_, m)
    A, S = float(np.quantile(a, 0.10)), float(np.exp(np.quantile(ls.max(1), 0.88)))
    crit = dict(box=dict(remove_boxes=[(lo, hi)]), opacity=dict(min_opacity=A), scale=dict(max_scale=S),
                keep=dict(keep_box=(np.quantile(x, 0.02, axis=0), np.quantile(x, 0.98, axis=0))),
                mask=dict(remove=(np.arange(nd.shape[0]) % 7 == 3).astype(np.uint8)))
    crit["all"] = {k: v for c in list(crit.values()) for k, v in c.items()}
    want = {name: hierarchy.prune_hierarchy(h, **kw) for name, kw in crit.items()}
    P = int(leaf.sum())
    assert 0.07 * P <= want["box"].removed_leaves <= 0.14 * P, want["box"].removed_leaves
    for name in ("opacity", "scale"):
        assert 0.05 * P <= want[name].removed_leaves <= 0.20 * P, (name, want[name].removed_leaves)
    return crit, want


@pytest.mark.parametrize("name", ("box", "opacity", "scale", "keep", "mask", "all"))
def test_each_criterion_and_all_combined(gpu, name):
    h = case(2000)
    crit, want = criteria2000()
    got = run_case(gpu, h, want[name], **crit[name])
    leaf = h.nodes[:, 6].numpy() == 0
    gone = lambda r: np.nonzero(leaf & (r.new_of_old.cpu().numpy() < 0))[0]
    assert np.array_equal(gone(got), gone(want[name])) and gone(got).size == want[name].removed_leaves > 0
    assert nested_np(got.hierarchy.nodes.cpu().numpy(), got.hierarchy.boxes.cpu().numpy())


def test_nan_rows_meet_the_criteria_as_in_the_spec(gpu):
    h = hierarchy.Hierarchy(*(getattr(case(257), k).clone() for k in ARRAYS))
    ids = np.nonzero(h.nodes[:, 6].numpy() == 0)[0]
    h.xyz[ids[3], 1], h.alpha[ids[5], 0], h.log_scales[ids[7], 0] = float("nan"), float("nan"), float("nan")
    h.log_scales[ids[7], 1:] = -9.0
    big = ((-1e9, -1e9, -1e9), (1e9, 1e9, 1e9))
    for kw, node in ((dict(remove_boxes=[big]), None), (dict(keep_box=big), ids[3]), (dict(min_opacity=0.0), ids[5]),
                     (dict(max_scale=1e9), ids[7])):
        if node is None:                     # everything but the NaN mean lies in the box: one leaf survives
            want = hierarchy.prune_hierarchy(h, remerge="none", **kw)
            assert want.hierarchy.nodes[:, 6].eq(0).sum() == 1
        else:
            want = hierarchy.prune_hierarchy(h, remerge="none", **kw)
            assert want.removed_leaves == 1 and int(want.new_of_old[node]) == -1
        got = hierarchy.prune_hierarchy_gpu(to_dev(h, gpu), remerge="none", **kw)
        assert torch.equal(got.new_of_old.cpu(), want.new_of_old) and torch.equal(got.hierarchy.nodes.cpu(), want.hierarchy.nodes)


# ---- the C ABI on guarded buffers ------------------------------------------------------------------------------------
def _args(**kw):
    a = _lib.HierPruneArgs()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


class PruneRun(AbiRun):
    """test_hier_trim_gpu.AbiRun's guarded layout for hgs_hier_prune_plan / _apply: tmp exactly tmp_bytes, the mask in a
    guarded allocation of its own."""

    def __init__(self, h, gpu, mask, **kw):
        super().__init__(h, gpu, **kw)
        self.tmp = wg.guarded(_lib.lib().hgs_hier_prune_tmp_bytes(self.N), gpu, 0x00, "tmp")
        self.mask = wg.guarded(self.N, gpu, 0xFF, "mask")
        self.mask.body[:self.N] = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(gpu)
        self.inputs["mask"] = self.mask

    def plan(self, args=None):
        rep = _lib.HierPruneReport()
        rc = _lib.lib().hgs_hier_prune_plan(C.byref(self.view(self.inputs, self.G, self.N)), C.byref(args or _args()),
                                            self.mask.addr, self.tmp.addr, C.byref(rep), _stream(), self.gpu.index or 0)
        return rc, rep

    def apply(self, out_N, out_G=None, remerge=1):
        o = self.outputs
        return _lib.lib().hgs_hier_prune_apply(C.byref(self.view(self.inputs, self.G, self.N)),
                                               C.byref(self.view(o, out_N if out_G is None else out_G, out_N, self.out_shift)),
                                               self.tmp.addr, remerge, o["old_of_new"].addr, o["new_of_old"].addr, _stream(),
                                               self.gpu.index or 0)


@pytest.mark.parametrize("fill", (0x00, 0xFF))
@pytest.mark.parametrize("P,M,kind", [(2, 16, "first_leaf"), (129, 16, "every_second_leaf"), (129, 4, "under_node_1"),
                                      (257, 16, "all_but_one_leaf"), (2000, 16, "every_second_leaf"), ("merged", 16, "last_leaf")])
def test_the_calls_stay_in_bounds(gpu, P, M, kind, fill):
    """Inputs with a 5-row tail of 0xFF bytes (never read, never changed); outputs and both maps with 2 guard rows of their
    own behind the N' rows and allocation guards behind those; tmp exactly tmp_bytes."""
    h = with_width(case(P), M)
    mask = removal_mask(h, kind)
    want = hierarchy.prune_hierarchy(h, remove=mask)
    run = PruneRun(h, gpu, mask, tail=5)
    rc, rep = run.plan()
    assert rc == 0 and list(rep.first_bad) == [-1] * 6, _lib.lib().hgs_last_error()
    assert (rep.kept, rep.removed_leaves, rep.dead, rep.dirty, rep.single_child, rep.root_dead) == \
        (want.hierarchy.num_nodes, want.removed_leaves, want.dead, want.dirty, want.single_child, 0)
    assert rep.children_sum == h.num_nodes - 1 and rep.levels == int(h.nodes[:, 0].max()) + 1
    kept = int(rep.kept)
    run.allocate(kept, fill, extra_rows=2)
    assert run.apply(kept, kept + 2) == 0, _lib.lib().hgs_last_error()
    run.guards()
    out_h, oon, noo = run.result(kept)
    assert_equals_spec("guarded", out_h, (oon, noo), want, dirty_new(h, want))
    for k in ARRAYS + ("old_of_new",):                      # the rows behind N' still hold the fill
        w = 1 if k == "old_of_new" else run.width[k]
        off = run.out_shift.get(k, 0)
        rest = run.outputs[k].body[off + kept * w * 4:].cpu()
        assert rest.numel() == 2 * w * 4 and bool((rest == fill).all()), k
    run.inputs_unchanged()


def test_bases_off_the_16_byte_grid(gpu):
    """xyz, alpha, log_scales, nodes (and shs: it then takes the 4-byte pieces) off the 16-byte grid are accepted and give
    the spec's result; rots or boxes off it are refused before any launch."""
    h = case(129)
    mask = removal_mask(h, "every_second_leaf")
    want = hierarchy.prune_hierarchy(h, remove=mask)
    for shift in (dict(xyz=4, alpha=4, log_scales=12), dict(xyz=8, shs=4, alpha=12, log_scales=4, nodes=4)):
        run = PruneRun(h, gpu, mask, tail=3, shift=shift)
        rc, rep = run.plan()
        assert rc == 0 and rep.kept == want.hierarchy.num_nodes
        run.allocate(int(rep.kept))
        assert run.apply(int(rep.kept)) == 0, _lib.lib().hgs_last_error()
        run.guards()
        out_h, oon, noo = run.result(int(rep.kept))
        assert_equals_spec("shifted", out_h, (oon, noo), want, dirty_new(h, want))
        run.inputs_unchanged()
    for k in ("rots", "boxes"):
        run = PruneRun(h, gpu, mask, shift={k: 4})
        assert run.plan()[0] == 1 and b"16-byte" in _lib.lib().hgs_last_error()
        run = PruneRun(h, gpu, mask, out_shift={k: 8})
        rc, rep = run.plan()
        assert rc == 0
        run.allocate(int(rep.kept))
        assert run.apply(int(rep.kept)) == 1 and b"16-byte" in _lib.lib().hgs_last_error()
        torch.cuda.synchronize()
        assert all(bool((g.body == 0xFF).all()) for g in run.outputs.values())


def test_two_runs_give_equal_bits_and_leave_the_input_alone(gpu):
    h = case(2000)
    crit, _ = criteria2000()
    d = to_dev(h, gpu)
    before = [getattr(d, k).clone() for k in ARRAYS]
    a = hierarchy.prune_hierarchy_gpu(d, **crit["all"])
    b = hierarchy.prune_hierarchy_gpu(d, **crit["all"])
    s1 = torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        c = hierarchy.prune_hierarchy_gpu(d, **crit["all"])
    torch.cuda.synchronize()
    for other in (b, c):
        for k in ARRAYS:
            assert torch.equal(bits(getattr(a.hierarchy, k)), bits(getattr(other.hierarchy, k))), k
        assert torch.equal(a.old_of_new, other.old_of_new) and torch.equal(a.new_of_old, other.new_of_old)
    for k, t in zip(ARRAYS, before):
        assert torch.equal(bits(getattr(d, k)), bits(t)), f"input {k} was modified"


def _corruptions():
    """(name, hierarchy, index into PRUNE_CHECKS or None for the children sum, node): the trimmer's three layout
    corruptions and the refit's layout, depth and two-claims ones.  (The trimmer's fourth, closure, lowers an extent: this
    rule does not read extents, so it is no corruption here -- test_an_extent_is_not_this_rules_business.)"""
    from test_hier_refit_cpu import corruptions as refit_corruptions
    from test_hier_trim_cpu import corruptions as trim_corruptions
    out = [("trim." + name, c, check, node) for name, c, _, check, node in trim_corruptions() if check < 3]
    out += [("refit." + name, c, check, node) for name, c, _, check, node in refit_corruptions() if check is None or check < 6]
    return out


CORRUPTIONS = 3 + 11


@pytest.mark.parametrize("i", range(CORRUPTIONS))
def test_rejections_on_the_device(gpu, i):
    cases = _corruptions()
    assert len(cases) == CORRUPTIONS
    name, c, check, node = cases[i]
    want = hierarchy.PRUNE_CHILDREN_SUM if check is None else hierarchy.PRUNE_CHECKS[check]
    with pytest.raises(hierarchy.HierarchyPruneError) as e:
        hierarchy.prune_hierarchy_gpu(to_dev(c, gpu), min_opacity=0.01)
    assert e.value.check == want and e.value.node == node, (name, e.value.check, e.value.node)
    # through the ABI: the report, the message, and no output written -- an apply behind the failed plan is refused
    run = PruneRun(c, gpu, np.zeros(c.num_nodes, dtype=np.uint8))
    run.allocate(c.num_nodes)
    rc, rep = run.plan()
    assert rc == 1, name
    if check is None:
        assert list(rep.first_bad) == [-1] * 6 and b"count_children sums to" in _lib.lib().hgs_last_error()
    else:
        assert rep.first_bad[check] == node and f"first offending node {node}".encode() in _lib.lib().hgs_last_error(), name
    assert run.apply(c.num_nodes) == 1 and b"no successful hgs_hier_prune_plan" in _lib.lib().hgs_last_error()
    run.guards()
    assert all(bool((g.body == 0xFF).all()) for g in run.outputs.values())
    run.inputs_unchanged()


def test_an_extent_is_not_this_rules_business(gpu):
    from test_hier_trim_cpu import corruptions as trim_corruptions
    name, c, _, check, _ = trim_corruptions()[0]
    assert name == "closure" and check == 3
    mask = removal_mask(c, "first_leaf")
    run_case(gpu, c, hierarchy.prune_hierarchy(c, remove=mask), remove=mask)


def test_a_dead_root_is_refused_and_nothing_is_written(gpu):
    h = case(257)
    mask = np.ones(h.num_nodes, dtype=np.uint8)
    run = PruneRun(h, gpu, mask)
    run.allocate(h.num_nodes)
    rc, rep = run.plan()
    assert rc == 1 and rep.root_dead == 1 and rep.kept == 0 and rep.removed_leaves == 257
    assert b"every leaf would be removed" in _lib.lib().hgs_last_error()
    assert run.apply(h.num_nodes) == 1 and b"no successful hgs_hier_prune_plan" in _lib.lib().hgs_last_error()
    run.guards()
    assert all(bool((g.body == 0xFF).all()) for g in run.outputs.values())
    run.inputs_unchanged()
    # a plan that succeeded before on the same tmp does not outlive the refusal; an output of another size is refused
    run = PruneRun(h, gpu, removal_mask(h, "first_leaf"))
    rc, rep = run.plan()
    assert rc == 0
    run.allocate(int(rep.kept) + 1)
    for n in (int(rep.kept) - 1, int(rep.kept) + 1):
        assert run.apply(n, int(rep.kept) + 1) == 1 and b"kept count" in _lib.lib().hgs_last_error()
    assert run.apply(int(rep.kept), int(rep.kept) + 1, remerge=5) == 1 and b"remerge" in _lib.lib().hgs_last_error()
    run.mask.body[:h.num_nodes] = 1
    assert run.plan()[0] == 1
    assert run.apply(int(rep.kept), int(rep.kept) + 1) == 1 and b"no successful hgs_hier_prune_plan" in _lib.lib().hgs_last_error()
    torch.cuda.synchronize()
    assert all(bool((g.body == 0xFF).all()) for g in run.outputs.values())


# ---- the result in use ---------------------------------------------------------------------------------------------------
def test_cuts_and_a_render_of_the_pruned_hierarchy(gpu):
    from gaussian_hierarchy._C import _boxes_nested
    h = case(2000)
    crit, want = criteria2000()
    got = hierarchy.prune_hierarchy_gpu(to_dev(h, gpu), **crit["box"])
    w = want["box"]
    g = got.hierarchy
    assert _boxes_nested(g.nodes, g.boxes)
    leaves = np.nonzero(w.hierarchy.nodes[:, 6].numpy() == 0)[0]
    dead = w.new_of_old.numpy() < 0
    cam = synth.make_camera(64, 48)
    for v in VIEWS[:2]:
        for px in (None, 3.0, 30.0):
            tau = 0.0 if px is None else fc.tau_of(CAM, px)
            cv, ex = _gpu_cuts(g, tau, v, gpu)
            ri, pi, ni, wt, kids = oracle_cut(w.hierarchy, tau, v)
            assert cv.n == len(ri) > 0
            for a, b in ((cv.render_indices, ri), (cv.parent_indices, pi), (cv.node_indices, ni), (cv.kids, kids)):
                assert np.array_equal(a.cpu().numpy(), np.asarray(b)), (v, px)
            assert np.array_equal(cv.weights.cpu().numpy().view(np.uint32), np.asarray(wt, dtype=np.float32).view(np.uint32))
            if px is None:
                assert np.array_equal(np.sort(cv.node_indices.cpu().numpy()), leaves)
            for idx in (cv.render_indices, cv.parent_indices, cv.node_indices):
                assert not dead[got.old_of_new.cpu().numpy()[idx.cpu().numpy()]].any()
    v = VIEWS[0]
    cv, _ = _gpu_cuts(g, fc.tau_of(cam, 3.0), v, gpu)
    color_g, radii_g = _render(gpu, cam, g, cv.render_indices, cv.parent_indices, cv.weights, cv.kids)
    color_w, radii_w = _render(gpu, cam, to_dev(w.hierarchy, gpu), cv.render_indices, cv.parent_indices, cv.weights, cv.kids)
    top = float(color_w.abs().max())
    err = float((color_g - color_w).abs().max())
    print("render: max", top, "difference", err)
    assert top > 0.05 and int((radii_w > 0).sum()) > 0
    assert err <= 1e-5 * top


# ---- the command -------------------------------------------------------------------------------------------------------
def test_command_round_trip(gpu, tmp_path, capsys):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from hgs import prune_hierarchy as cmd
    h = case(2000)
    crit, want = criteria2000()
    w = want["box"]
    lo, hi = crit["box"]["remove_boxes"][0]
    g = torch.Generator().manual_seed(4)
    tail = lambda t: torch.cat([t, torch.randn(5, *t.shape[1:], generator=g)])
    (tmp_path / "in").mkdir()
    src, dst = str(tmp_path / "in" / "in.hier"), str(tmp_path / "out" / "pruned.hier")
    write_hierarchy(src, tail(h.xyz), tail(h.shs), tail(h.alpha).abs(), tail(h.log_scales), tail(h.rots), h.nodes, h.boxes)
    anchors = np.arange(0, 3999, 37, dtype=np.int32)[::-1].copy()
    cmd.write_anchors(str(tmp_path / "in" / "anchors.bin"), anchors)
    (tmp_path / "in" / "exposure.json").write_text(json.dumps({"img_0": [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]}))
    box = ["--remove-box"] + [repr(float(np.float32(x))) for x in list(lo) + list(hi)]
    assert cmd.main([src, dst] + box) == 0
    out = capsys.readouterr().out
    kept_anchors, dropped = cmd.remap_anchors(anchors, w.new_of_old.numpy())
    assert dropped > 0
    assert f"N = 3999 -> {w.hierarchy.num_nodes} nodes: {w.removed_leaves} leaves removed, {w.dead} nodes dropped" in out
    assert f"{w.dirty} ancestors re-merged" in out and f"{w.single_child} nodes left with a single child" in out
    assert "5 rows behind" in out and f"anchors.bin remapped, {dropped} of {anchors.size} anchors dropped" in out
    assert "exposure.json copied" in out and " ms" in out and out.count("\n") == 1
    h0, got = hierarchy.Hierarchy(*load_hierarchy(src)), hierarchy.Hierarchy(*load_hierarchy(dst))
    n = w.hierarchy.num_nodes
    assert got.num_nodes == n and got.xyz.shape[0] == n + 5
    body = hierarchy.Hierarchy(*(getattr(got, k)[:n] for k in ROWS), got.nodes, got.boxes.reshape(n, 2, 4))
    assert_equals_spec("command", body, (w.old_of_new, w.new_of_old), w, dirty_new(h, w))
    for k in ROWS:
        assert torch.equal(bits(getattr(got, k)[n:]), bits(getattr(h0, k)[3999:])), f"tail of {k}"
    assert cmd.read_anchors(str(tmp_path / "out" / "anchors.bin")).tolist() == kept_anchors.tolist()
    raw = open(str(tmp_path / "out" / "anchors.bin"), "rb").read()
    assert int.from_bytes(raw[:4], "little") == kept_anchors.size == (len(raw) - 4) // 4
    assert (tmp_path / "out" / "exposure.json").read_text() == (tmp_path / "in" / "exposure.json").read_text()
    # --half: readable by the loader, the records and boxes the same; --align: no node beyond the aligner's 62.8 degrees
    half, aligned = str(tmp_path / "half" / "p.hier"), str(tmp_path / "aligned" / "p.hier")
    assert cmd.main([src, half, "--half"] + box) == 0
    hh = hierarchy.Hierarchy(*load_hierarchy(half))
    assert torch.equal(hh.nodes, got.nodes) and torch.equal(bits(hh.boxes), bits(got.boxes)) and hh.xyz.shape[0] == n + 5
    assert float((hh.shs[:n] - got.shs[:n]).abs().max()) <= 2e-3 * float(got.shs[:n].abs().max())
    assert cmd.main([src, aligned, "--align", "--remerge", "all"] + box) == 0
    assert "frames aligned" in capsys.readouterr().out
    ha = hierarchy.Hierarchy(*load_hierarchy(aligned))
    ha = hierarchy.Hierarchy(*(getattr(ha, k)[:n] for k in ROWS), ha.nodes, ha.boxes)
    assert torch.equal(ha.nodes, got.nodes)
    assert float((hierarchy.alignment_dots(ha) < hierarchy.ALIGN_BOUND).mean()) == 0.0
    # every leaf removed: named, nothing written, exit status 1
    never = str(tmp_path / "never" / "p.hier")
    assert cmd.main([src, never, "--min-opacity", "2"]) == 1
    err = capsys.readouterr().err
    assert "every leaf would be removed" in err and "nothing written" in err and not (tmp_path / "never" / "p.hier").exists()
