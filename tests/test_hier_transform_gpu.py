"""The HIP similarity transform (hgs.hierarchy.transform_hierarchy_gpu, csrc/hier_transform.hip) against the numpy spec
hgs.hierarchy.transform_hierarchy: all seven tensors bit for bit, at node counts on both sides of a wave and a
workgroup, for five transforms, every SH width, tails behind the nodes, in place and out of place; guarded buffers and
unaligned bases through the C ABI; determinism; the rejections (HGS_ERR_INVALID, the output untouched); end to end on
the 2 000-leaf scene (the device cut of a half-turned hierarchy, the in-op LOD render of a generally moved one from
the moved camera); the command's round trip."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import parity as pa
import ws_guard as wg
from boundary_fixtures import lod_lerp
from hgs import _lib, hierarchy, synth
from oracle import raster_oracle as ro
from test_hier_transform_cpu import HALF_TURNS, bad_parameter_blocks, general
from test_hier_trim_cpu import ARRAYS, CAM, VIEWS, bits, scene2000
from test_hier_trim_gpu import _gpu_cuts, _render

pytestmark = pytest.mark.gpu

LEAVES = (1, 2, 128, 129, 257, 2000)          # N = 2 P - 1 = 1, 3, 255, 257, 513, 3999
ROWS = ARRAYS[:5]
WIDTH = dict(xyz=3, alpha=1, log_scales=3, rots=4, nodes=7, boxes=8)


@functools.lru_cache(maxsize=None)
def transforms():
    tiny = 1e-4
    return {"identity": hierarchy.similarity(),
            "half_turn_s2": hierarchy.similarity(R=HALF_TURNS[1], scale=2.0),
            "quarter_turn_t": hierarchy.similarity(R=np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), translate=(0.5, -4.0, 2.0)),
            "tiny_rotation": hierarchy.similarity(quat=(np.cos(tiny / 2), 0.0, np.sin(tiny / 2) * 0.6, np.sin(tiny / 2) * 0.8)),
            "general": general()}


@functools.lru_cache(maxsize=None)
def built(P, M=16, tail=0):
    """A host hierarchy of P leaves with M SH coefficients per row and ``tail`` rows behind the N node rows."""
    h = scene2000()[0] if P == 2000 else hierarchy.build_hierarchy(synth.make_scene_trained_like(P, CAM, seed=5))
    g = torch.Generator().manual_seed(P + tail)
    more = lambda t: torch.cat([t, torch.randn(tail, *t.shape[1:], generator=g)]) if tail else t
    return hierarchy.Hierarchy(more(h.xyz), more(h.shs[:, :M].contiguous()), more(h.alpha), more(h.log_scales), more(h.rots),
                               h.nodes, h.boxes)


@functools.lru_cache(maxsize=None)
def spec(P, M, tail, name):
    return hierarchy.transform_hierarchy(built(P, M, tail), transforms()[name])


def to_dev(h, gpu):
    return hierarchy.Hierarchy(*(getattr(h, k).to(gpu).clone().contiguous() for k in ARRAYS))


def assert_bits(got, want, what=""):
    for k in ARRAYS:
        a, b = getattr(got, k).cpu(), getattr(want, k)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape)
        assert torch.equal(bits(a), bits(b)), (what, k, int((bits(a) != bits(b)).sum()))


def both_ways(gpu, P, M, tail, name):
    """Out of place (the input unchanged), then in place: both equal the spec bit for bit."""
    h, sim, want = built(P, M, tail), transforms()[name], spec(P, M, tail, name)
    d = to_dev(h, gpu)
    stats = {}
    out = hierarchy.transform_hierarchy_gpu(d, sim, stats=stats)
    assert out is not d and stats["transform_ms"] > 0.0 and out.nodes.device == gpu
    assert all(getattr(out, k).data_ptr() != getattr(d, k).data_ptr() for k in ARRAYS)
    assert_bits(out, want, (P, M, tail, name, "out of place"))
    assert_bits(d, h, (P, M, tail, name, "the input"))
    assert hierarchy.transform_hierarchy_gpu(d, sim, inplace=True) is d
    assert_bits(d, want, (P, M, tail, name, "in place"))


@pytest.mark.parametrize("P", LEAVES)
def test_sizes_and_transforms(gpu, P):
    for name in transforms():
        both_ways(gpu, P, 16, 0, name)
    if P == 2000:       # the identity returns the input's bits
        assert_bits(spec(P, 16, 0, "identity"), built(P))


@pytest.mark.parametrize("M", (1, 4, 9, 16))
def test_sh_widths(gpu, M):
    """12 M bytes per shs row: 12 (band 0 alone: copied) and 108 move in 4-byte pieces, 48 and 192 in 16-byte ones."""
    for name in ("general", "quarter_turn_t", "identity"):
        both_ways(gpu, 129, M, 0, name)
    assert spec(129, M, 0, "general").shs.shape[1:] == (M, 3)


@pytest.mark.parametrize("tail", (0, 1, 100))
def test_rows_behind_the_nodes_are_transformed(gpu, tail):
    for P in (128, 129):
        both_ways(gpu, P, 16, tail, "general")
        want, h = spec(P, 16, tail, "general"), built(P, 16, tail)
        assert want.xyz.shape[0] == h.num_nodes + tail
        if tail:
            assert not torch.equal(want.shs[h.num_nodes:, 1:], h.shs[h.num_nodes:, 1:])


def test_rows_past_two_to_the_31_elements(gpu):
    """G = 2^31 / 48 + 1000 rows of 16 coefficients: the shs array has more than 2^31 floats (8.6 GB), so a 32-bit element
    index would wrap inside it.  One node, everything else a tail; in place; rows are independent, so the spec is
    evaluated on slices: the first rows, the rows around element 2^31, the last rows."""
    G = (1 << 31) // 48 + 1000
    g = torch.Generator(device=gpu).manual_seed(7)
    r = lambda *shape: torch.randn(*shape, generator=g, device=gpu)
    h0 = built(1)
    d = hierarchy.Hierarchy(r(G, 3), r(G, 16, 3), r(G, 1), r(G, 3), r(G, 4), h0.nodes.to(gpu).clone(), h0.boxes.to(gpu).clone())
    cut = (1 << 31) // 48
    slices = (slice(0, 300), slice(cut - 300, cut + 300), slice(G - 300, G))
    before = [tuple(getattr(d, k)[sl].cpu().numpy() for k in ("xyz", "shs", "log_scales", "rots", "alpha")) for sl in slices]
    sim = general()
    hierarchy.transform_hierarchy_gpu(d, sim, inplace=True)
    for sl, (x, c, ls, q, al) in zip(slices, before):
        want = hierarchy.transform_rows(sim, x, c, ls, q)
        for k, w in zip(("xyz", "shs", "log_scales", "rots"), want):
            got = getattr(d, k)[sl].cpu()
            assert torch.equal(bits(got), bits(torch.from_numpy(w))), (sl, k)
        assert torch.equal(bits(d.alpha[sl].cpu()), bits(torch.from_numpy(al))), sl
    assert torch.equal(bits(d.boxes.cpu()), bits(spec(1, 16, 0, "general").boxes))
    del d
    torch.cuda.empty_cache()


# ---- the C ABI on guarded buffers ------------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class AbiRun:
    """One hierarchy laid out in guarded allocations, one per array, for hgs_hier_transform.  shift: name -> bytes the
    array's base is moved inside its allocation (out_shift: the same for the outputs, by default as the inputs)."""

    def __init__(self, h, gpu, shift=None, out_shift=None, fill=0xFF):
        self.h, self.gpu, self.N, self.G, self.M = h, gpu, h.num_nodes, int(h.xyz.shape[0]), h.shs.shape[1]
        self.shift = shift or {}
        self.out_shift = self.shift if out_shift is None else out_shift
        self.width = dict(WIDTH, shs=3 * self.M)
        self.fill = fill
        self.inputs, self.outputs = {}, {}
        for k in ARRAYS:
            g = wg.guarded(self.nbytes(k) + self.shift.get(k, 0), gpu, 0xFF, "in." + k)
            src = getattr(h, k).contiguous().reshape(-1).view(torch.uint8).to(gpu)
            off = self.shift.get(k, 0)
            g.body[off:off + src.numel()] = src
            self.inputs[k] = g
            self.outputs[k] = wg.guarded(self.nbytes(k) + self.out_shift.get(k, 0), gpu, fill, "out." + k)

    def nbytes(self, k):
        return (self.N if k in ("nodes", "boxes") else self.G) * self.width[k] * 4

    def view(self, gs, shift):
        return _lib.HierView(self.G, self.N, self.M, 0, *(gs[k].addr + shift.get(k, 0) for k in ARRAYS))

    def call(self, sim, inplace=False, M=None):
        vi = self.view(self.inputs, self.shift)
        vo = vi if inplace else self.view(self.outputs, self.out_shift)
        if M is not None:
            vi.M = vo.M = M
        return _lib.lib().hgs_hier_transform(C.byref(vi), C.byref(vo), C.byref(hierarchy.transform_args(sim)), _stream(),
                                             self.gpu.index or 0)

    def guards(self):
        wg.check(*self.inputs.values(), *self.outputs.values())

    def result(self, gs, shift):
        torch.cuda.synchronize()
        t = {}
        for k in ARRAYS:
            off = shift.get(k, 0)
            raw = gs[k].body[off:off + self.nbytes(k)].cpu()
            t[k] = raw.view(torch.int32 if k == "nodes" else torch.float32).reshape(getattr(self.h, k).shape)
        return hierarchy.Hierarchy(*(t[k] for k in ARRAYS))

    def untouched(self, gs, shift, want_fill=None):
        """want_fill None: the arrays still hold the hierarchy; else: every byte still holds the fill."""
        torch.cuda.synchronize()
        for k in ARRAYS:
            body = gs[k].body.cpu()
            if want_fill is not None:
                assert bool((body == want_fill).all()), f"{k} was written"
                continue
            off = shift.get(k, 0)
            src = getattr(self.h, k).contiguous().reshape(-1).view(torch.uint8)
            assert torch.equal(body[off:off + src.numel()], src), f"input {k} was modified"
            assert bool((body[:off] == 0xFF).all()) and bool((body[off + src.numel():] == 0xFF).all()), k


@pytest.mark.parametrize("fill", (0x00, 0xFF))
@pytest.mark.parametrize("P,M,tail", [(1, 16, 0), (2, 16, 1), (129, 16, 100), (129, 9, 1), (129, 4, 0), (129, 1, 1), (257, 16, 0),
                                       (2000, 16, 0)])
def test_the_call_stays_in_bounds(gpu, P, M, tail, fill):
    """Every array in an allocation of exactly its size between guards: out of place into 0x00 / 0xFF-filled outputs
    (the input unchanged), then in place."""
    h, want = built(P, M, tail), spec(P, M, tail, "general")
    run = AbiRun(h, gpu, fill=fill)
    assert run.call(general()) == 0, _lib.lib().hgs_last_error()
    run.guards()
    assert_bits(run.result(run.outputs, run.out_shift), want)
    run.untouched(run.inputs, run.shift)
    assert run.call(general(), inplace=True) == 0, _lib.lib().hgs_last_error()
    run.guards()
    assert_bits(run.result(run.inputs, run.shift), want)


def test_bases_off_the_16_byte_grid(gpu):
    """xyz, alpha, log_scales, nodes (and shs: it then moves in 4-byte pieces) 4 bytes off are accepted, on either side
    alone too, and give the spec's result; rots or boxes off the 16-byte grid are refused before any launch."""
    h, want = built(129, 16, 1), spec(129, 16, 1, "general")
    off = dict(xyz=8, shs=4, alpha=12, log_scales=4, nodes=4)
    for shift, out_shift in ((dict(xyz=4, alpha=4, log_scales=12), None), (off, None), ({}, off), (off, {})):
        run = AbiRun(h, gpu, shift=shift, out_shift=out_shift)
        assert run.call(general()) == 0, _lib.lib().hgs_last_error()
        run.guards()
        assert_bits(run.result(run.outputs, run.out_shift), want)
        run.untouched(run.inputs, run.shift)
        assert run.call(general(), inplace=True) == 0
        run.guards()
        assert_bits(run.result(run.inputs, run.shift), want)
    for k in ("rots", "boxes"):
        for kw in (dict(shift={k: 4}, out_shift={}), dict(out_shift={k: 8})):
            run = AbiRun(h, gpu, **kw)
            assert run.call(general()) == 1 and b"16-byte" in _lib.lib().hgs_last_error()
            run.untouched(run.outputs, run.out_shift, want_fill=0xFF)


def test_determinism(gpu):
    h = built(2000)
    d = to_dev(h, gpu)
    a = hierarchy.transform_hierarchy_gpu(d, general())
    b = hierarchy.transform_hierarchy_gpu(d, general())
    s1 = torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        c = hierarchy.transform_hierarchy_gpu(d, general())
    torch.cuda.synchronize()
    for other in (b, c):
        for k in ARRAYS:
            assert torch.equal(bits(getattr(a, k)), bits(getattr(other, k))), k
    assert_bits(d, h, "the input")


def test_rejections_leave_the_output_untouched(gpu):
    h = built(129)
    run = AbiRun(h, gpu)
    for name, sim, word in bad_parameter_blocks():
        for inplace in (False, True):
            assert run.call(sim, inplace=inplace) == 1, name
            assert word in _lib.lib().hgs_last_error(), (name, _lib.lib().hgs_last_error())
    assert run.call(general(), M=2) == 1 and b"whole SH bands" in _lib.lib().hgs_last_error()
    run.guards()
    run.untouched(run.outputs, run.out_shift, want_fill=0xFF)
    run.untouched(run.inputs, run.shift)
    d = to_dev(h, gpu)
    for name, sim, _ in bad_parameter_blocks():
        with pytest.raises(ValueError):
            hierarchy.transform_hierarchy_gpu(d, sim, inplace=True)
    two = hierarchy.Hierarchy(d.xyz, d.shs[:, :2].contiguous(), d.alpha, d.log_scales, d.rots, d.nodes, d.boxes)
    with pytest.raises(ValueError, match="whole bands"):
        hierarchy.transform_hierarchy_gpu(two, general())
    assert_bits(d, h, "the input")


# ---- end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", VIEWS)
def test_the_device_cut_of_a_half_turned_hierarchy_is_the_originals(gpu, v):
    h, _ = scene2000()
    sim = hierarchy.similarity(R=HALF_TURNS[0], scale=2.0)
    d = to_dev(h, gpu)
    moved = hierarchy.transform_hierarchy_gpu(d, sim)
    v2 = tuple(float(x) for x in sim.apply(np.asarray(v)))
    tau = 0.02
    (cv_o, ex_o), (cv_t, ex_t) = _gpu_cuts(d, tau, v, gpu), _gpu_cuts(moved, tau, v2, gpu)
    assert cv_o.n == cv_t.n > 100
    for o, t in (((cv_o.render_indices, cv_o.parent_indices, cv_o.node_indices, cv_o.weights, cv_o.kids),
                  (cv_t.render_indices, cv_t.parent_indices, cv_t.node_indices, cv_t.weights, cv_t.kids)), (ex_o, ex_t)):
        for k in range(3):
            assert torch.equal(o[k], t[k]), k
        assert torch.equal(bits(o[3]), bits(t[3])) and torch.equal(o[4], t[4])
    assert bool(((cv_o.weights > 0) & (cv_o.weights < 1)).any())


def _oracle_lod_render(cam, h, ri, pi, w, kids):
    """The float64 oracle on the rows render_post's python glue would gather (boundary_fixtures.lod_lerp)."""
    full = dict(xyz=h.xyz, scaling=torch.exp(h.log_scales), rotation=torch.nn.functional.normalize(h.rots), opacity=h.alpha,
                features=h.shs)
    L = lod_lerp(full, ri.long(), pi.long(), w)
    n = ri.numel()
    return ro.rasterize(L["xyz"], torch.zeros(n, 3), L["features"], None, L["opacity"], L["scaling"], L["rotation"], None,
                        image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx,
                        tanfovy=cam.tanfovy, bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
                        projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center,
                        interpolation_weights=w, num_node_kids=kids, dtype=torch.float64).color.detach()


@pytest.mark.parametrize("weights", ("cut", "one"))
def test_the_render_of_a_moved_hierarchy_from_the_moved_camera_is_the_originals(gpu, weights):
    """One cut of the original (a general rotation grows the boxes: the cut at a given granularity is not invariant,
    the content rendered at a given cut is), rendered in-op from the original rows and camera and from the
    device-transformed rows and ``transform_camera``.  The bound is derived: the float64 oracle's own difference between
    the two renders plus, for each of the two HIP renders, the parity tolerance that holds it to its oracle (REL_TOL of
    the image's maximum).  Measured on one MI355X, image maximum 0.77: with the cut's weights the oracle's gap is
    2.3e-3 and the HIP difference equals it to three digits -- the renderer lerps a node's unit quaternion towards its
    parent's and builds the rotation from the shorter, unnormalised result, R(q) = (1 - |q|^2) I + |q|^2 R(q / |q|),
    which does not turn with the frame (f-13's alignment keeps |q| near 1) -- and at weight 1 (no lerp) the gap is the
    float32 rounding of the moved rows and matrices alone (see the printed figures)."""
    h, _ = scene2000()
    sim = general()
    d = to_dev(h, gpu)
    moved = hierarchy.transform_hierarchy_gpu(d, sim)
    cam = synth.make_camera(64, 48)
    cam_t = hierarchy.transform_camera(cam, sim)
    cv, _ = _gpu_cuts(d, 0.02, VIEWS[0], gpu)
    assert cv.n > 100 and bool(((cv.weights > 0) & (cv.weights < 1)).any())
    w = cv.weights if weights == "cut" else torch.ones_like(cv.weights)
    cut = (cv.render_indices, cv.parent_indices, w, cv.kids)
    color_o, radii_o = _render(gpu, cam, d, *cut)
    color_t, radii_t = _render(gpu, cam_t, moved, *cut)
    assert float(color_o.max()) > 0.05 and int((radii_o > 0).sum()) > 0
    host_cut = tuple(t.cpu() for t in cut)
    host = hierarchy.Hierarchy(*(getattr(moved, k).cpu() for k in ARRAYS))
    orc_o, orc_t = _oracle_lod_render(cam, h, *host_cut), _oracle_lod_render(cam_t, host, *host_cut)
    top = float(orc_o.abs().max())
    gap = float((orc_o - orc_t).abs().max())
    diff = float((color_o.cpu().double() - color_t.cpu().double()).abs().max())
    print(f"render of the moved hierarchy, weights = {weights}: HIP |d| = {diff:.3g}, oracle gap {gap:.3g}, image maximum "
          f"{top:.3g}, HIP vs its oracle {float((color_o.cpu().double() - orc_o).abs().max()):.3g} / "
          f"{float((color_t.cpu().double() - orc_t).abs().max()):.3g}")
    assert diff <= gap + 2 * pa.REL_TOL * top
    if weights == "one":
        assert gap <= 2e-5          # the bound of the oracle render test in tests/test_hier_transform_cpu.py
    # the old camera on the moved rows is another image: the check can fail
    other, _ = _render(gpu, cam, moved, *cut)
    assert float((other - color_o).abs().max()) > 10 * (gap + 2 * pa.REL_TOL * top)


# ---- the command -------------------------------------------------------------------------------------------------------
def test_command_round_trip(gpu, tmp_path, capsys):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from hgs import transform_hierarchy as cmd
    h = built(2000, 16, 5)
    src, dst, back = (str(tmp_path / n) for n in ("in.hier", "out/moved.hier", "out/back.hier"))
    write_hierarchy(src, h.xyz, h.shs, h.alpha.abs(), h.log_scales, h.rots, h.nodes, h.boxes)
    (tmp_path / "anchors.bin").write_bytes(b"anchors")
    h0 = hierarchy.Hierarchy(*load_hierarchy(src))
    argv = ["--scale", "1.7", "--axis-angle", "1", "2", "-0.5", "37", "--translate", "3", "-2", "9"]
    assert cmd.main([src, dst] + argv) == 0
    out = capsys.readouterr().out
    assert "N = 3999 nodes" in out and "5 rows behind the nodes transformed" in out and " ms on the device" in out
    assert "anchors.bin" in out and "copied beside the output" in out and "exposure.json" not in out
    assert (tmp_path / "out" / "anchors.bin").read_bytes() == b"anchors"
    sim = cmd.build_similarity(cmd.parse_args([src, dst] + argv))
    want = hierarchy.transform_hierarchy(h0, sim)
    got = hierarchy.Hierarchy(*load_hierarchy(dst))
    assert got.xyz.shape[0] == 4004 and got.num_nodes == 3999
    assert_bits(got, want, "the command")
    assert not torch.equal(got.shs[3999:, 1:], h0.shs[3999:, 1:])               # the tail rows moved too
    assert cmd.main([dst, back, "--invert"] + argv) == 0
    assert "stays valid beside the output" in capsys.readouterr().out
    again = hierarchy.Hierarchy(*load_hierarchy(back))
    assert_bits(again, hierarchy.transform_hierarchy(want, sim.inverse()), "the command, inverted")
    assert float((again.xyz - h0.xyz).abs().max()) <= 1e-4 and torch.equal(again.nodes, h0.nodes)
