"""The raw-parameter path (``GaussianRasterizer.forward_raw``: split SH storage, activations fused into K1 and K8a) at its
edges, against the float64 oracle behind ``ro.activate_raw`` (tests/raw_cases.py holds the cases, tests/test_raw_edges_cpu.py
checks them with no GPU).  Indices bit-exact, pixels and gradients within ``parity.REL_TOL``:

  A  split rows off the 256-row workgroup grid: the 16-byte body / scalar tail of coop_load_seg / coop_store_seg;
  B  an empty ``features_rest``, and an active degree below the stored one;
  C  a workgroup with under half of its rows in view (K1 then reads the split rows per lane: load_sh_split);
  D  accumulation into caller buffers (RasterContext.grad_buffers, key shs_rest included): coop_store_seg<true> and the
     per-lane accumulating store; a buffer off its 16-byte boundary is refused;
  E  sh_bwd_kernel<JAC = false> on split storage, through the C ABI with prepare_backward = 0;
  F  every activation where its derivative is special."""
import pytest
import torch

import parity as pa
import raw_cases as rc

pytestmark = pytest.mark.gpu

BUFFER_OF = dict(xyz="means3D", f_dc="shs", f_rest="shs_rest", opacity="opacities", scaling="scales", rotation="rotations",
                 means2D="means2D")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(name, gpu, **kw):
    """The named case through the kernels and the oracle: (case, kernel run, ``parity.verify`` result)."""
    case = rc.build(name)
    raw, cam, bg, gc, gd, stored, active, act = case
    hip = rc._run_hip_raw(raw, cam, bg, gc, gd, stored, act, gpu, active_degree=active, **kw)
    res = pa.verify(hip, rc._oracle_raw(raw, cam, bg, active, act), gc, gd, do_depth=kw.get("do_depth", True))
    for k, v in res["stats"].items():
        if isinstance(v, dict):
            print(f"{name}: {k} maxrel {v['maxrel']:.2e} l2 {v['l2']:.2e}")
    rc._compare(hip, res)
    for k, g in hip["grads"].items():
        assert bool(torch.isfinite(g).all()), (name, k)
    return case, hip, res


# ---- A: split rows off the grid --------------------------------------------------------------------------------------
@pytest.mark.parametrize("stored,P", [(3, P) for P in rc.SPLIT_P3] + [(s, P) for s in (1, 2) for P in rc.SPLIT_P12])
def test_split_rows_off_the_workgroup_grid(gpu, stored, P):
    _, hip, _ = _check(f"split_s{stored}_P{P}", gpu)
    assert hip["grads"]["f_rest"].shape == (P, (stored + 1) ** 2 - 1, 3)
    if P > 1:        # an all-zero output cannot pass on a dark scene
        assert bool(hip["grads"]["f_rest"].any()) and bool(hip["grads"]["f_dc"].any())


# ---- B: degree 0 and a lowered active degree -------------------------------------------------------------------------
def test_empty_features_rest(gpu):
    (raw, *_), hip, res = _check("degree0", gpu)
    assert raw["f_rest"].shape == (65, 0, 3)
    assert "f_rest" in hip["no_grad"] or hip["grads"]["f_rest"].numel() == 0
    assert bool(hip["grads"]["f_dc"].any()) and "d_f_dc" in res["stats"]


@pytest.mark.parametrize("stored,active", rc.DEGREE_PAIRS)
def test_active_degree_below_stored_degree(gpu, stored, active):
    _, hip, _ = _check(f"degree_s{stored}_a{active}", gpu)
    g, nb = hip["grads"]["f_rest"], (active + 1) ** 2
    assert g.shape[1] == (stored + 1) ** 2 - 1
    assert not bool(_bits(g[:, nb - 1:]).any()), "a coefficient beyond the active degree took a gradient (or a -0.0)"
    assert active == 0 or bool(g[:, :nb - 1].any())


# ---- C: mostly-culled workgroups --------------------------------------------------------------------------------------
@pytest.mark.parametrize("do_depth", [True, False])
@pytest.mark.parametrize("stored", [3, 2])
def test_mostly_culled_workgroup_and_clamped_colours(gpu, stored, do_depth):
    _, hip, _ = _check(f"culled_s{stored}", gpu, do_depth=do_depth)
    tt = hip["views"]["tiles_touched"]
    vis = tt > 0
    assert 0 < int(vis[:256].sum()) < 128, "workgroup 0 must take the per-lane loads"
    assert int(vis[256:512].sum()) >= 128, "workgroup 1 must take the cooperative loads"
    assert 0 < int(vis[512:].sum()) < 88
    g = hip["grads"]
    for k in rc.RAW_KEYS + ("means2D",):                            # a culled row: zeros everywhere
        assert not bool(g[k][~vis].any()), k
    # a clamped channel takes no SH gradient, its neighbour does
    rows = torch.arange(600)
    red_only = vis & (rows % 5 == 2)
    assert int(red_only.sum()) >= 30
    for k in ("f_dc", "f_rest"):
        assert not bool(g[k][red_only][:, :, 0].any()) and bool(g[k][red_only][:, :, 1].any()), k
    all_three = vis & (rows % 5 == 1)
    assert int(all_three.sum()) >= 30 and not bool(g["f_dc"][all_three].any()) and not bool(g["f_rest"][all_three].any())


# ---- D: accumulation into caller buffers ------------------------------------------------------------------------------
GUARD, STALE, FENCE = 64, 123.0, -7.5          # floats of guard around every buffer (256 bytes: slices stay 16-byte aligned)


def _guarded_buffers(shapes, dev, shift=None):
    """Every buffer a slice of ONE flat tensor, a guard of FENCE on both sides, the buffers pre-filled with STALE.
    ``shift``: {name: floats} by which a buffer is moved into the guard in front of it (off its 16-byte boundary)."""
    offs, total = {}, GUARD
    for k, s in shapes.items():
        n = int(torch.Size(s).numel())
        offs[k] = (total - (shift or {}).get(k, 0), n)
        total += (n + 3) // 4 * 4 + GUARD
    flat = torch.full((total,), FENCE, device=dev)
    assert flat.data_ptr() % 16 == 0
    is_guard = torch.ones(total, dtype=torch.bool, device=dev)
    bufs = {}
    for k, (o, n) in offs.items():
        flat[o:o + n] = STALE
        is_guard[o:o + n] = False
        bufs[k] = flat[o:o + n].view(*shapes[k])
        assert bufs[k].data_ptr() % 16 == (-4 * (shift or {}).get(k, 0)) % 16
    return flat, is_guard, bufs


def _guards_intact(flat, is_guard):
    torch.cuda.synchronize()
    return bool((_bits(flat[is_guard]) == _bits(torch.tensor([FENCE]))[0].item()).all())


def _buffer_shapes(raw):
    P = raw["xyz"].shape[0]
    return dict(means3D=(P, 3), shs=(P, 1, 3), shs_rest=tuple(raw["f_rest"].shape), opacities=(P, 1), scales=(P, 3),
                rotations=(P, 4), means2D=(P, 3))


@pytest.mark.parametrize("stored", [3, 2])
def test_accumulation_into_caller_buffers(gpu, stored):
    """Stored degree 3: 48-float rows, coop_store_seg<ACC>; stored degree 2: 27-float rows, the per-lane store.  View 0
    overwrites stale buffers, view 1 adds to them.  sh_bwd_kernel adds the stored value ONCE to the finished row (both
    stores: ``row + old``), so the shs / shs_rest buffers hold the float32 sum of the two single-view gradients to the
    bit; dL/dmeans3D is added to twice (K8a: ``d_mean + old``, K8b: ``+= view-direction term``), so that buffer and the
    other per-row ones are held to the oracle's sum only.  means2D is a per-view quantity and never accumulated."""
    import diff_gaussian_rasterization as dgr
    cases = [rc.build(f"accum_s{stored}_v{v}") for v in (0, 1)]
    sep, ref = [], []
    for v in (0, 1):
        _, hip, res = _check(f"accum_s{stored}_v{v}", gpu)
        sep.append(hip["grads"])
        ref.append(res["grads"])
    raw = cases[0][0]
    flat, is_guard, bufs = _guarded_buffers(_buffer_shapes(raw), gpu)
    ctx = dgr.RasterContext(grad_buffers=bufs)
    for v, (raw_v, cam, bg, gc, gd, _, active, act) in enumerate(cases):
        ctx.grad_accumulate = v > 0
        hip = rc._run_hip_raw(raw_v, cam, bg, gc, gd, stored, act, gpu, context=ctx, active_degree=active)
        assert sorted(hip["no_grad"]) == sorted(BUFFER_OF) and not hip["grads"], "a buffered gradient reached .grad"
        assert _guards_intact(flat, is_guard), f"view {v} wrote outside a gradient buffer"
        if v == 0:               # the stale contents are gone: the buffers hold the unbuffered gradients of view 0
            for k, b in BUFFER_OF.items():
                assert torch.equal(_bits(bufs[b].cpu().reshape(sep[0][k].shape)), _bits(sep[0][k])), (k, "view 0")
    got = {k: bufs[b].cpu().reshape(sep[0][k].shape) for k, b in BUFFER_OF.items()}
    for k in ("f_dc", "f_rest"):
        assert torch.equal(_bits(got[k]), _bits(sep[0][k] + sep[1][k])), (k, "not the float32 sum of the two views")
    assert torch.equal(_bits(got["means2D"]), _bits(sep[1]["means2D"])), "means2D must hold the second view alone"
    for k in rc.RAW_KEYS:
        st = pa.err_stats(got[k], ref[0][k] + ref[1][k])
        print(f"accumulated d_{k}: maxrel {st['maxrel']:.2e} l2 {st['l2']:.2e}")
        assert st["maxrel"] <= pa.REL_TOL and st["l2"] <= pa.REL_TOL, (k, st)


@pytest.mark.parametrize("name", ["shs", "shs_rest", "rotations"])
def test_gradient_buffer_off_its_16_byte_boundary_is_refused(gpu, name):
    """coop_store_seg / coop_store_sh / k8_store_row write these three as float4: a buffer 4 bytes off the boundary is
    refused like such an input, before the backward launches anything (every buffer keeps its stale contents)."""
    import diff_gaussian_rasterization as dgr
    raw, cam, bg, gc, gd, stored, active, act = rc.build("accum_s3_v0")
    flat, is_guard, bufs = _guarded_buffers(_buffer_shapes(raw), gpu, shift={name: 1})
    before = flat.clone()
    with pytest.raises(RuntimeError, match="16-byte"):
        rc._run_hip_raw(raw, cam, bg, gc, gd, stored, act, gpu, context=dgr.RasterContext(grad_buffers=bufs))
    torch.cuda.synchronize()
    assert torch.equal(_bits(flat), _bits(before))


# ---- E: the SH backward that reads the coefficients (JAC = false) on split storage ------------------------------------
@pytest.mark.parametrize("P", [65, 257])
@pytest.mark.parametrize("deg", [1, 2, 3])
def test_split_storage_without_a_prepared_backward(gpu, deg, P):
    """hgs_raster_fwd / hgs_raster_bwd with prepare_backward = 0 and shs_rest, M = 4 / 9 / 16: K1 stores no d(rgb)/d(dir),
    sh_bwd_kernel<JAC = false> stages the split rows through coop_load_seg (M = 4, 16) or reads them per lane (M = 9).
    Every buffer guarded, 0x00- and 0xFF-filled.  Compared with the oracle only: the comments of csrc/preprocess.hip
    promise equal bits between the fused and the two-kernel backward, not between the prepared (gr . J) and the
    unprepared (sum over the basis gradients) form of the view-direction term."""
    import test_workspace_bounds_gpu as wb
    from hgs import synth
    cam = synth.make_camera(wb.W, wb.H, 60.0)
    scene = synth.make_scene(P, cam, seed=P % 89 + deg, sh_degree=deg)
    gc, gd = synth.upstream_grads(wb.H, wb.W, seed=2)
    inp = wb._inputs("shs_rest", scene, gpu)
    assert inp["sh_rest"].shape == (P, (deg + 1) ** 2 - 1, 3)
    hip = wb._both_fills(lambda fill: wb.raster_chain(cam, inp, deg, gc, gd, gpu, fill, prepare_backward=0)[0])
    assert bool(hip["grads"]["shs_rest"].any())
    hip["grads"]["shs"] = torch.cat([hip["grads"]["shs"], hip["grads"].pop("shs_rest")], 1)
    wb._check_against_reference(f"shs_rest JAC=false M={(deg + 1) ** 2} P={P}", hip, pa.oracle_run(scene, cam, wb.BG), gc, gd)


# ---- F: activation edges ---------------------------------------------------------------------------------------------
def _rows(values, rows, *idx):
    return torch.cat([rows[i::len(values)] for i in idx])


def test_sigmoid_saturated_both_ways(gpu):
    """Besides the usual comparison: dL/d(raw opacity) divided by the exact d sigmoid -- that is dL/d(opacity), of one
    magnitude over all rows, so a saturated row's gradient (1e-8 .. 1e-13 of the others') is compared at all.  The
    kernel forms 1 - o in float64; rounding o to 2^-53 leaves 1 - o a relative error of 2^-53 / (1 - o) (1e-3 at raw
    30), which the bound of a row admits on top of REL_TOL.  Raw +-90: the derivative is below float32's normal range."""
    (raw, *_), hip, res = _check("act_sigmoid", gpu)
    sp = rc._special_rows(rc.P_ACT)
    g, ref = hip["grads"]["opacity"].double().reshape(-1), res["grads"]["opacity"].reshape(-1)
    never = _rows(rc.SIGMOID_RAW, sp, 0, 1, 2, 3)                   # below 1/255: never blended
    assert not bool(_bits(hip["grads"]["opacity"][never]).any())
    x = raw["opacity"].double().reshape(-1)
    e = torch.exp(-x.abs())
    dact, one_minus_o = e / (1 + e) ** 2, torch.where(x > 0, e, torch.ones_like(e)) / (1 + e)
    sel = x.abs() <= 30
    a, b = (g / dact)[sel], (ref / dact)[sel]
    bound = pa.REL_TOL * b.abs().max() + 2.0 ** -52 / one_minus_o[sel] * b.abs()
    worst = ((a - b).abs() / bound).max().item()
    print(f"act_sigmoid: dL/do through the exact derivative, worst |d| / bound {worst:.3f}")
    assert worst <= 1.0
    sat = _rows(rc.SIGMOID_RAW, sp, 6, 7)                           # raw 17 and 30 do blend: a tiny gradient, not none
    assert int((g[sat] != 0).sum()) >= 15


def test_abs_at_zeros_and_denormals(gpu):
    _, hip, res = _check("act_abs", gpu)
    sp = rc._special_rows(rc.P_ACT)
    never = _rows(rc.ABS_RAW, sp, 0, 1, 2, 3)                       # +0, -0, +-1e-40: never blended
    assert not bool(_bits(hip["grads"]["opacity"][never]).any())
    g, ref = hip["grads"]["opacity"].reshape(-1), res["grads"]["opacity"].reshape(-1)
    neg = _rows(rc.ABS_RAW, sp, 5, 7)                               # d|x|/dx = -1 there
    assert int((ref[neg] != 0).sum()) >= 15 and bool((torch.sign(g[neg].double()) == torch.sign(ref[neg])).all())


def test_opacity_passed_as_it_is(gpu):
    _, hip, _ = _check("act_none", gpu)
    never = rc._special_rows(rc.P_ACT)[::2]                         # rows <= 0
    for k in ("opacity", "xyz", "f_dc", "f_rest", "scaling", "rotation"):
        assert not bool(hip["grads"][k][never].any()), k
    assert not bool(_bits(hip["grads"]["opacity"][never]).any())


def test_exp_of_extreme_scales(gpu):
    _, hip, _ = _check("act_scaling", gpu)
    tiny = _rows(rc.SCALING_RAW, rc._special_rows(rc.P_ACT)[::2], 0)
    assert bool((hip["radii"][tiny] == 3).all()) and bool(hip["grads"]["scaling"][tiny].any())


def _assert_rows_scaled(name, hip_g, ref_g, scale):
    """``grad * scale`` row-wise, then the usual norm-wise comparison."""
    st = pa.err_stats(hip_g.double() * scale[:, None], ref_g * scale[:, None])
    print(f"{name}: maxrel {st['maxrel']:.2e} l2 {st['l2']:.2e}")
    assert st["maxrel"] <= pa.REL_TOL and st["l2"] <= pa.REL_TOL, (name, st)


def test_quaternion_norms_over_ten_decades(gpu):
    """dL/d(raw rotation) = (I - q q^T) dL/dq / |raw| scales with 1 / |raw|: compared as it is, the rows of norm 1e-6
    drown the others.  ``grad * |raw|`` is free of the norm, and every row counts."""
    (raw, *_), hip, res = _check("act_rotation", gpu)
    n = raw["rotation"].double().norm(dim=1)
    _assert_rows_scaled("act_rotation: d_rotation |raw|", hip["grads"]["rotation"], res["grads"]["rotation"], n)


def test_zero_quaternion(gpu):
    (raw, *_), hip, res = _check("act_zero_quat", gpu)
    z = rc.ZERO_QUAT_ROW
    g, ref = hip["grads"]["rotation"], res["grads"]["rotation"]
    st = pa.err_stats(g[z], ref[z])                                 # that row against the oracle's, to its own scale
    assert st["maxrel"] <= pa.REL_TOL and st["l2"] <= pa.REL_TOL, st
    keep = torch.ones(rc.P_ZERO_QUAT, dtype=torch.bool)
    keep[z] = False
    st = pa.err_stats(g[keep], ref[keep])
    assert st["maxrel"] <= pa.REL_TOL and st["l2"] <= pa.REL_TOL, st
    assert bool(hip["grads"]["scaling"][z].any()) and hip["radii"][z] > 0          # the row is drawn: R = identity
