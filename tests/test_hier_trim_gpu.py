"""The HIP trimmer (hgs.hierarchy.trim_hierarchy_gpu, csrc/hier_trim.hip) against the numpy spec
hgs.hierarchy.trim_hierarchy: all seven output tensors, both maps, N' and the stub count bit for bit, at node counts on
both sides of a wave, a workgroup and a scan chunk, for every SH width; guarded buffers, tails, unaligned bases;
determinism; the four rejections through the C ABI; the contract end to end (GPU cuts and an in-op LOD render of the
trimmed hierarchy equal the original's after mapping); the command's round trip."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import parity as pa
import ws_guard as wg
from hgs import _lib, hierarchy, synth
from test_hier_trim_cpu import (ARRAYS, CAM, INF, ROI, VIEWS, bits, check_layout, corruptions, scene2000, stub_tau)

pytestmark = pytest.mark.gpu

LEAVES = (1, 2, 128, 129, 257, 2000)          # N = 2 P - 1 = 1, 3, 255, 257, 513, 3999
MODES = ("floor", "region", "floor_region", "budget", "identity", "root_only")
ROWS = ARRAYS[:5]
ALL_INSIDE = torch.tensor([[0.0, 0.0, 1.0, 1e30]] * 5)


@functools.lru_cache(maxsize=None)
def built(P, M=16):
    """(host hierarchy with M SH coefficients per row, the median extent of its nodes with children or 1.0)."""
    h = scene2000()[0] if P == 2000 else hierarchy.build_hierarchy(synth.make_scene_trained_like(P, CAM, seed=5))
    if M != 16:
        h = hierarchy.Hierarchy(h.xyz, h.shs[:, :M].contiguous(), h.alpha, h.log_scales, h.rots, h.nodes, h.boxes)
    inner = h.boxes[:, 0, 3].numpy()[h.nodes[:, 6].numpy() > 0]
    return h, (float(np.median(inner)) if inner.size else 1.0)


def to_dev(h, gpu):
    return hierarchy.Hierarchy(*(getattr(h, k).to(gpu).contiguous() for k in ARRAYS))


def mode_kwargs(mode, h, med):
    return {"floor": dict(min_extent=med), "region": dict(roi=ROI), "floor_region": dict(min_extent=med, roi=ROI),
            "budget": dict(max_nodes=max(1, h.num_nodes // 2)), "identity": {}, "root_only": dict(min_extent=INF)}[mode]


def assert_equals_spec(got, want):
    """got: a TrimResult of device tensors; want: the spec's."""
    assert got.hierarchy.num_nodes == want.hierarchy.num_nodes and got.stubs == want.stubs
    assert got.min_extent == want.min_extent
    for k in ARRAYS:
        a, b = getattr(got.hierarchy, k).cpu(), getattr(want.hierarchy, k)
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape)
        assert torch.equal(bits(a), bits(b)), k
    for k in ("old_of_new", "new_of_old", "stub_ids"):
        a, b = getattr(got, k).cpu(), getattr(want, k)
        assert a.dtype == torch.int32 and torch.equal(a, b), k


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", LEAVES)
def test_sizes_and_modes(gpu, P, mode):
    h, med = built(P)
    kw = mode_kwargs(mode, h, med)
    stats = {}
    got = hierarchy.trim_hierarchy_gpu(to_dev(h, gpu), stats=stats, **kw)
    want = hierarchy.trim_hierarchy(h, **kw)
    assert_equals_spec(got, want)
    assert stats["trim_ms"] > 0.0 and got.hierarchy.nodes.device == gpu
    if mode == "identity":
        assert got.hierarchy.num_nodes == h.num_nodes and got.stubs == 0
    if mode == "root_only":
        assert got.hierarchy.nodes.tolist() == [[0, -1, 0, 1, 0, 0, 0]]


@pytest.mark.parametrize("mode", ("floor", "region", "identity"))
@pytest.mark.parametrize("M", (1, 4, 9))
def test_sh_widths(gpu, M, mode):
    """12 M bytes per shs row: 12 and 108 take the 4-byte pieces, 48 (and 192 above) the 16-byte ones."""
    h, med = built(129, M)
    kw = mode_kwargs(mode, h, med)
    got = hierarchy.trim_hierarchy_gpu(to_dev(h, gpu), **kw)
    assert got.hierarchy.shs.shape[1:] == (M, 3)
    assert_equals_spec(got, hierarchy.trim_hierarchy(h, **kw))


def test_a_region_keeps_siblings_scattered_through_the_index_range(gpu):
    h, _ = built(2000)
    roi = ((1.0, -3.0, 8.0), (4.0, 0.0, 16.0))
    want = hierarchy.trim_hierarchy(h, roi=roi)
    old = want.old_of_new.numpy()
    runs = int((np.diff(old) != 1).sum()) + 1
    assert 100 < old.size < 3000 and runs > 50 and old[-1] > 3000, (old.size, runs, int(old[-1]))
    assert_equals_spec(hierarchy.trim_hierarchy_gpu(to_dev(h, gpu), roi=roi), want)


@functools.lru_cache(maxsize=None)
def two_scan_chunks():
    """N = 2 097 153 nodes at one SH coefficient: 8 193 workgroup sums, the smallest count with a second scan chunk."""
    dev = torch.device("cuda:0")
    h = hierarchy.build_hierarchy_on_device(1_048_577, CAM, dev, seed=2, sh_degree=0)
    h = hierarchy.Hierarchy(h.xyz, h.shs[:, :1].contiguous(), h.alpha, h.log_scales, h.rots, h.nodes, h.boxes)
    host = hierarchy.Hierarchy(*(getattr(h, k).cpu() for k in ARRAYS))
    inner = host.boxes[:, 0, 3].numpy()[host.nodes[:, 6].numpy() > 0]
    return h, host, float(np.median(inner))


@pytest.mark.parametrize("mode", ("floor", "region", "identity"))
def test_the_second_scan_chunk(gpu, mode):
    """The kept count is the second chunk's total behind the first chunk's published one; under identity the last node's
    new index is its workgroup's scanned sum, the one entry of the second chunk."""
    h, host, med = two_scan_chunks()
    assert h.num_nodes == 2_097_153 and (h.num_nodes + 255) // 256 == 8193
    kw = mode_kwargs(mode, host, med)
    got = hierarchy.trim_hierarchy_gpu(h, **kw)
    want = hierarchy.trim_hierarchy(host, **kw)
    if mode == "identity":
        assert int(want.new_of_old[-1]) == 2_097_152
    else:
        assert 1000 < want.hierarchy.num_nodes < h.num_nodes - 1000
    assert_equals_spec(got, want)


# ---- the C ABI on guarded buffers ------------------------------------------------------------------------------------
WIDTH = dict(xyz=3, alpha=1, log_scales=3, rots=4, nodes=7, boxes=8)


def _args(min_extent=0.0, roi=None):
    a = _lib.HierTrimArgs(float(min_extent), 0 if roi is None else 1)
    if roi is not None:
        a.roi_lo[:], a.roi_hi[:] = roi
    return a


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class AbiRun:
    """One hierarchy laid out in guarded allocations, one per array, for hgs_hier_trim_plan / _apply.
    tail: rows behind the N nodes (0xFF bytes); shift: name -> bytes the array's base is moved inside its allocation
    (out_shift: the same for the outputs, by default as the inputs)."""

    def __init__(self, h, gpu, tail=0, shift=None, out_shift=None):
        self.h, self.gpu, self.N, self.G = h, gpu, h.num_nodes, h.num_nodes + tail
        self.M = h.shs.shape[1]
        self.shift = shift or {}
        self.out_shift = self.shift if out_shift is None else out_shift
        self.width = dict(WIDTH, shs=3 * self.M)
        self.inputs = {}
        for k in ARRAYS:
            rows = self.N if k in ("nodes", "boxes") else self.G
            g = wg.guarded(rows * self.width[k] * 4 + self.shift.get(k, 0), gpu, 0xFF, "in." + k)
            src = getattr(h, k).contiguous().reshape(-1).view(torch.uint8).to(gpu)
            off = self.shift.get(k, 0)
            g.body[off:off + src.numel()] = src
            self.inputs[k] = g
        self.tmp = wg.guarded(_lib.lib().hgs_hier_trim_tmp_bytes(self.N), gpu, 0x00, "tmp")
        self.outputs = {}

    def view(self, gs, G, N, shift=None):
        shift = self.shift if shift is None else shift
        return _lib.HierView(G, N, self.M, 0, *(gs[k].addr + shift.get(k, 0) for k in ARRAYS))

    def plan(self, args):
        rep = _lib.HierTrimReport()
        rc = _lib.lib().hgs_hier_trim_plan(C.byref(self.view(self.inputs, self.G, self.N)), C.byref(args), self.tmp.addr,
                                           C.byref(rep), _stream(), self.gpu.index or 0)
        return rc, rep

    def allocate(self, kept, fill=0xFF, extra_rows=0):
        rows = kept + extra_rows
        self.outputs = {k: wg.guarded(rows * self.width[k] * 4 + self.out_shift.get(k, 0), self.gpu, fill, "out." + k)
                        for k in ARRAYS}
        self.outputs["old_of_new"] = wg.guarded(rows * 4, self.gpu, fill, "old_of_new")
        self.outputs["new_of_old"] = wg.guarded(self.N * 4, self.gpu, fill, "new_of_old")

    def apply(self, out_N, out_G=None):
        o = self.outputs
        return _lib.lib().hgs_hier_trim_apply(C.byref(self.view(self.inputs, self.G, self.N)),
                                              C.byref(self.view(o, out_N if out_G is None else out_G, out_N, self.out_shift)),
                                              self.tmp.addr, o["old_of_new"].addr, o["new_of_old"].addr, _stream(),
                                              self.gpu.index or 0)

    def guards(self):
        wg.check(self.tmp, *self.inputs.values(), *self.outputs.values())

    def result(self, kept):
        """The first `kept` output rows as a host Hierarchy, and the two maps."""
        torch.cuda.synchronize()
        t = {}
        for k in ARRAYS:
            off = self.out_shift.get(k, 0)
            raw = self.outputs[k].body[off:off + kept * self.width[k] * 4].cpu()
            t[k] = raw.view(torch.int32 if k == "nodes" else torch.float32).reshape(kept, *getattr(self.h, k).shape[1:])
        oon = self.outputs["old_of_new"].body[:kept * 4].cpu().view(torch.int32)
        noo = self.outputs["new_of_old"].view(torch.int32).cpu()
        return hierarchy.Hierarchy(*(t[k] for k in ARRAYS)), oon, noo

    def inputs_unchanged(self):
        for k in ARRAYS:
            off = self.shift.get(k, 0)
            body = self.inputs[k].body.cpu()
            src = getattr(self.h, k).contiguous().reshape(-1).view(torch.uint8)
            assert torch.equal(body[off:off + src.numel()], src), f"input {k} was modified"
            assert bool((body[off + src.numel():] == 0xFF).all()) and bool((body[:off] == 0xFF).all()), f"the tail of {k} was modified"


def _against_spec(run, want, out_h, oon, noo):
    for k in ARRAYS:
        assert torch.equal(bits(getattr(out_h, k)), bits(getattr(want.hierarchy, k))), k
    assert torch.equal(oon, want.old_of_new) and torch.equal(noo, want.new_of_old)


@pytest.mark.parametrize("fill", (0x00, 0xFF))
@pytest.mark.parametrize("P,M", [(1, 16), (2, 16), (129, 16), (129, 9), (257, 16), (2000, 16)])
def test_the_calls_stay_in_bounds(gpu, P, M, fill):
    """Inputs with a 5-row tail of 0xFF bytes (never read into the output, never changed); outputs and both maps with
    2 guard rows of their own behind the N' rows and allocation guards behind those; tmp exactly tmp_bytes."""
    h, med = built(P, M)
    want = hierarchy.trim_hierarchy(h, med, ROI if P == 2000 else None)
    run = AbiRun(h, gpu, tail=5)
    rc, rep = run.plan(_args(med, ROI if P == 2000 else None))
    assert rc == 0 and list(rep.first_bad) == [-1] * 4
    assert (rep.kept, rep.stubs) == (want.hierarchy.num_nodes, want.stubs)
    kept = int(rep.kept)
    run.allocate(kept, fill, extra_rows=2)
    assert run.apply(kept, kept + 2) == 0, _lib.lib().hgs_last_error()
    run.guards()
    _against_spec(run, want, *run.result(kept))
    for k in ARRAYS + ("old_of_new",):                      # the rows behind N' still hold the fill
        w = 1 if k == "old_of_new" else run.width[k]
        off = run.out_shift.get(k, 0)
        rest = run.outputs[k].body[off + kept * w * 4:].cpu()
        assert rest.numel() == 2 * w * 4 and bool((rest == fill).all()), k
    run.inputs_unchanged()


def test_bases_off_the_16_byte_grid(gpu):
    """xyz, alpha, log_scales (and shs: it then takes the 4-byte pieces) 4 bytes off are accepted and give the spec's
    result; rots or boxes off the 16-byte grid are refused before any launch."""
    h, med = built(129)
    want = hierarchy.trim_hierarchy(h, med)
    for shift in (dict(xyz=4, alpha=4, log_scales=12), dict(xyz=8, shs=4, alpha=12, log_scales=4, nodes=4)):
        run = AbiRun(h, gpu, tail=3, shift=shift)
        rc, rep = run.plan(_args(med))
        assert rc == 0 and rep.kept == want.hierarchy.num_nodes
        run.allocate(int(rep.kept))
        assert run.apply(int(rep.kept)) == 0, _lib.lib().hgs_last_error()
        run.guards()
        _against_spec(run, want, *run.result(int(rep.kept)))
        run.inputs_unchanged()
    for k in ("rots", "boxes"):
        run = AbiRun(h, gpu, shift={k: 4})
        rc, _ = run.plan(_args(med))
        assert rc == 1 and b"16-byte" in _lib.lib().hgs_last_error()
        # an aligned input with a misaligned output: refused by apply, the outputs keep their fill
        run = AbiRun(h, gpu, out_shift={k: 8})
        rc, rep = run.plan(_args(med))
        assert rc == 0
        run.allocate(int(rep.kept))
        assert run.apply(int(rep.kept)) == 1 and b"16-byte" in _lib.lib().hgs_last_error()
        torch.cuda.synchronize()
        assert all(bool((g.body == 0xFF).all()) for g in run.outputs.values())


def test_determinism_and_untouched_inputs(gpu):
    h, med = built(2000)
    d = to_dev(h, gpu)
    before = [getattr(d, k).clone() for k in ARRAYS]
    a = hierarchy.trim_hierarchy_gpu(d, med, ROI)
    b = hierarchy.trim_hierarchy_gpu(d, med, ROI)
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        c = hierarchy.trim_hierarchy_gpu(d, med, ROI)
    with torch.cuda.stream(s2):
        e = hierarchy.trim_hierarchy_gpu(d, med, ROI)
    torch.cuda.synchronize()
    for other in (b, c, e):
        for k in ARRAYS:
            assert torch.equal(bits(getattr(a.hierarchy, k)), bits(getattr(other.hierarchy, k))), k
        assert torch.equal(a.old_of_new, other.old_of_new) and torch.equal(a.new_of_old, other.new_of_old)
        assert a.stubs == other.stubs
    for k, t in zip(ARRAYS, before):
        assert torch.equal(bits(getattr(d, k)), bits(t)), f"input {k} was modified"


@pytest.mark.parametrize("case", range(4), ids=["closure", "start", "children", "parent"])
def test_rejections_on_the_device(gpu, case):
    name, c, floor, check, node = corruptions()[case]
    with pytest.raises(hierarchy.HierarchyTrimError) as e:
        hierarchy.trim_hierarchy_gpu(to_dev(c, gpu), floor)
    assert e.value.check == hierarchy.TRIM_CHECKS[check] and e.value.node == node, (name, e.value.check, e.value.node)
    assert f"node {node}" in str(e.value)
    # through the ABI: the report, the message, and no output written -- an apply behind the failed plan is refused
    run = AbiRun(c, gpu)
    run.allocate(c.num_nodes)
    rc, rep = run.plan(_args(floor))
    assert rc == 1 and rep.first_bad[check] == node and list(rep.first_bad).count(-1) == 3
    assert f"first offending node {node}".encode() in _lib.lib().hgs_last_error()
    assert run.apply(c.num_nodes) == 1 and b"no successful hgs_hier_trim_plan" in _lib.lib().hgs_last_error()
    run.guards()
    assert all(bool((g.body == 0xFF).all()) for g in run.outputs.values())
    run.inputs_unchanged()


def test_an_output_of_another_size_is_refused(gpu):
    h, med = built(257)
    run = AbiRun(h, gpu)
    rc, rep = run.plan(_args(med))
    assert rc == 0 and 1 < rep.kept < h.num_nodes
    kept = int(rep.kept)
    run.allocate(kept + 1)
    for n in (kept - 1, kept + 1):
        assert run.apply(n, kept + 1) == 1 and b"kept count" in _lib.lib().hgs_last_error()
    torch.cuda.synchronize()
    assert all(bool((g.body == 0xFF).all()) for g in run.outputs.values())
    assert run.apply(kept, kept + 1) == 0
    run.guards()
    _against_spec(run, hierarchy.trim_hierarchy(h, med), *run.result(kept))


# ---- the contract end to end -------------------------------------------------------------------------------------------
def _gpu_cuts(h, tau, v, gpu):
    """(cut_view with planes that contain everything, expand_to_size + get_interpolation_weights), both on the device."""
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    from hgs.frustum import cull_bounds, cut_view
    N = h.num_nodes
    bounds = cull_bounds(h.nodes, h.xyz.contiguous(), torch.exp(h.log_scales).contiguous())
    cv = cut_view(h.nodes, h.boxes, bounds, float(tau), torch.tensor(v), ALL_INSIDE, 1.0)
    ri = torch.zeros(N, dtype=torch.int32, device=gpu); pi = torch.zeros_like(ri); ni = torch.zeros_like(ri)
    w = torch.zeros(N, device=gpu); ns = torch.zeros(N, dtype=torch.int32, device=gpu)
    n = expand_to_size(h.nodes, h.boxes, float(tau), torch.tensor(v).to(gpu), torch.zeros(3), ri, pi, ni)
    get_interpolation_weights(ni[:n], float(tau), h.nodes, h.boxes, torch.tensor(v), torch.zeros(3), w, ns)
    assert cv.n == cv.n_unculled == n
    return cv, (ri[:n], pi[:n], ni[:n], w[:n], ns[:n])


def _render(gpu, cam, h, ri, pi, w, ns):
    """The in-op LOD path (the route of tests/test_frustum_gpu.py::_render) on a hierarchy's own rows."""
    import diff_gaussian_rasterization as dgr
    kw = pa.settings_kwargs(cam, torch.zeros(3), 3, do_depth=False, device=gpu, interpolation_weights=w, num_node_kids=ns)
    kw.update(render_indices=ri.contiguous(), parent_indices=pi.contiguous())
    G = h.xyz.shape[0]
    with torch.no_grad():
        color, radii, _ = dgr.GaussianRasterizer(dgr.GaussianRasterizationSettings(**kw))(
            means3D=h.xyz, means2D=torch.zeros(G, 3, device=gpu), shs=h.shs, opacities=h.alpha,
            scales=torch.exp(h.log_scales), rotations=torch.nn.functional.normalize(h.rots))
    return color, radii


@pytest.mark.parametrize("v", VIEWS)
def test_cuts_and_render_of_the_trimmed_hierarchy_are_the_originals(gpu, v):
    h, med = scene2000()
    d = to_dev(h, gpu)
    r = hierarchy.trim_hierarchy_gpu(d, med)
    assert (r.hierarchy.num_nodes, r.stubs) == (2001, 435)
    tau = stub_tau(r, v)
    assert r.exact_for(v, tau) and not r.exact_for(v, tau / np.float32(10))
    m = r.new_of_old.long()
    (cv_o, ex_o), (cv_t, ex_t) = _gpu_cuts(d, tau, v, gpu), _gpu_cuts(r.hierarchy, tau, v, gpu)
    assert cv_o.n == cv_t.n > 0 and bool(torch.isin(cv_t.node_indices, r.stub_ids).any())
    for o, t in (((cv_o.render_indices, cv_o.parent_indices, cv_o.node_indices, cv_o.weights, cv_o.kids),
                  (cv_t.render_indices, cv_t.parent_indices, cv_t.node_indices, cv_t.weights, cv_t.kids)), (ex_o, ex_t)):
        for k in range(3):
            assert torch.equal(m[o[k].long()].to(torch.int32), t[k]), k
        assert torch.equal(bits(o[3]), bits(t[3])) and torch.equal(o[4], t[4])
    cam = synth.make_camera(64, 48)
    color_o, radii_o = _render(gpu, cam, d, cv_o.render_indices, cv_o.parent_indices, cv_o.weights, cv_o.kids)
    color_t, radii_t = _render(gpu, cam, r.hierarchy, cv_t.render_indices, cv_t.parent_indices, cv_t.weights, cv_t.kids)
    assert float(color_o.max()) > 0.05 and int((radii_o > 0).sum()) > 0
    assert torch.equal(color_o, color_t) and torch.equal(radii_o, radii_t)


def test_the_budget_on_the_device_is_the_specs(gpu):
    h, _ = built(2000)
    d = to_dev(h, gpu)
    for K in (1, 3, 100, 1001, 3998, 3999, 10 ** 9):
        got = hierarchy.trim_hierarchy_gpu(d, max_nodes=K)
        assert_equals_spec(got, hierarchy.trim_hierarchy(h, max_nodes=K))
        assert got.hierarchy.num_nodes <= K
    got = hierarchy.trim_hierarchy_gpu(d, max_nodes=1001, roi=ROI)
    assert_equals_spec(got, hierarchy.trim_hierarchy(h, max_nodes=1001, roi=ROI))
    check_layout(got.hierarchy.nodes.cpu().numpy())


# ---- the command -------------------------------------------------------------------------------------------------------
def test_command_round_trip(gpu, tmp_path, capsys):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from hgs import trim_hierarchy as cmd
    h, _ = built(2000)
    g = torch.Generator().manual_seed(4)
    tail = lambda t: torch.cat([t, torch.randn(5, *t.shape[1:], generator=g)])
    src, dst, again = (str(tmp_path / n) for n in ("in.hier", "out/trimmed.hier", "again.hier"))
    write_hierarchy(src, tail(h.xyz), tail(h.shs), tail(h.alpha).abs(), tail(h.log_scales), tail(h.rots), h.nodes, h.boxes)
    (tmp_path / "anchors.bin").write_bytes(b"x")
    assert cmd.main([src, dst, "--max-nodes", "1001"]) == 0
    out = capsys.readouterr().out
    assert "N = 3999 -> 1001 nodes" in out and "stubs" in out and "5 rows behind" in out and " ms" in out
    assert "anchors.bin beside the input is not copied" in out and "exposure.json" not in out
    h0, got = hierarchy.Hierarchy(*load_hierarchy(src)), hierarchy.Hierarchy(*load_hierarchy(dst))
    assert got.num_nodes == 1001 and got.xyz.shape[0] == 1006
    want = hierarchy.trim_hierarchy(h, max_nodes=1001)
    for k in ROWS:
        assert torch.equal(bits(getattr(got, k)[:1001]), bits(getattr(want.hierarchy, k))), k
        assert torch.equal(bits(getattr(got, k)[1001:]), bits(getattr(h0, k)[3999:])), f"tail of {k}"
    assert torch.equal(got.nodes, want.hierarchy.nodes) and torch.equal(bits(got.boxes), bits(want.hierarchy.boxes))
    assert cmd.main([dst, again, "--min-extent", "0"]) == 0
    assert "N = 1001 -> 1001 nodes (0 stubs)" in capsys.readouterr().out
    assert open(again, "rb").read() == open(dst, "rb").read()
    # a hierarchy that fails a check: named, nothing written, exit status 1
    bad = hierarchy.Hierarchy(*(getattr(h0, k).clone() for k in ARRAYS))
    bad.nodes[1234, 2] += 1
    bad_path, never = str(tmp_path / "bad.hier"), str(tmp_path / "never.hier")
    write_hierarchy(bad_path, bad.xyz, bad.shs, bad.alpha, bad.log_scales, bad.rots, bad.nodes, bad.boxes)
    assert cmd.main([bad_path, never, "--min-extent", "1"]) == 1
    err = capsys.readouterr().err
    assert "node 1234" in err and "nothing written" in err and not (tmp_path / "never.hier").exists()
