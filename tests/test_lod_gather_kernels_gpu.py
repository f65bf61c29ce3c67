"""The LOD gather / scatter device code on hand-built cuts (tests/lod_gather_spec.py), at every SH width.

Part 1: the C entry points hgs_lod_gather / hgs_lod_gather_bwd, called directly with guarded buffers -- the float SH
kernels (M = 1, 9: 3 and 27 floats per row) next to the float4 ones (M = 4, 16), run leaders with and without atomics,
runs that end on, start on and straddle a 256-row workgroup boundary, a 600-sibling run, one-row cuts, a self-parent
row, weights of exactly 0 and 1, dot products of exactly 0 and -0.0, and every attribute group alone.  The gather is held
to the bits of the float32 model, the scatter to the derived bound of the float64 adjoint.

Part 2: the same cuts through GaussianRasterizer with non-empty render / parent indices (the LOD instantiations of the
per-Gaussian kernels; the in-kernel scatter at cpr = 3 and 12, the through-memory glue branch at M = 1, 9) against the
rows route: the reference glue's torch lerp feeds the op with empty indices, the lerped rows are leaves, and their
gradients go through the float64 adjoint.  Culled rows inside runs, and the weight-1 rule: a parent that has no weight
in any row may hold NaN."""
import numpy as np
import pytest
import torch

import boundary_fixtures as bf
import lod_gather_spec as ls
import parity as pa
from hgs import _lib, synth
from test_workspace_bounds_gpu import Bufs, _both_fills, _ok, _stream

pytestmark = pytest.mark.gpu

GROUPS = ls.GROUPS
W, H = 64, 48


def _inner(M):
    return dict(means3D=(3,), scales=(3,), rotations=(4,), shs=(M, 3), opacities=(1,))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ================================================================================================================
# 1. the C entry points, direct
# ================================================================================================================
def _direct(gpu, cut, M, groups):
    lib = _lib.lib()
    n, G, dev = cut.n, cut.G, gpu.index or 0
    inner = _inner(M)
    attrs, grads = ls.make_attrs(cut, M), ls.make_row_grads(cut, M)
    emitted = cut.order == "emitted"
    scattered = []                                     # (atomic sums of three or more partial sums have no fixed bits)

    def run(fill):
        bufs = Bufs(gpu, fill)
        ri = bufs.copy_of("render_indices", torch.from_numpy(cut.ri))
        pi = bufs.copy_of("parent_indices", torch.from_numpy(cut.pi))
        w = bufs.copy_of("weights", torch.from_numpy(cut.w))
        src = {k: bufs.copy_of(k, torch.from_numpy(attrs[k])) for k in groups}
        o = {k: bufs.filled("o_" + k, torch.float32, (n,) + inner[k]) for k in groups}
        ptr = lambda d, k: d[k].data_ptr() if k in d else None
        _ok(lib.hgs_lod_gather(ri.data_ptr(), pi.data_ptr(), w.data_ptr(), n, M, *(ptr(src, k) for k in GROUPS),
                               *(ptr(o, k) for k in GROUPS), _stream(), dev), "hgs_lod_gather")
        gi = {k: bufs.copy_of("g_" + k, torch.from_numpy(grads[k])) for k in groups}
        res = {"o": {k: v.cpu().clone() for k, v in o.items()}, "flag": [], "d": []}
        for rep in range(2):                           # (a second call: same bits when no atomics are involved)
            d = {k: bufs.filled(f"d{rep}_{k}", torch.float32, (G,) + inner[k], fill=0x00) for k in groups}   # zeroed: caller
            flag = bufs.filled(f"flag{rep}", torch.int32, (1,))
            _ok(lib.hgs_lod_gather_bwd(ri.data_ptr(), pi.data_ptr(), w.data_ptr(), n, M, ptr(src, "rotations"),
                                       *(ptr(gi, k) for k in GROUPS), *(ptr(d, k) for k in GROUPS), flag.data_ptr(),
                                       _stream(), dev), "hgs_lod_gather_bwd")
            res["flag"].append(int(flag.cpu()[0]))
            dd = {k: v.cpu().clone() for k, v in d.items()}
            scattered.append(dd)
            if emitted:
                res["d"].append(dd)
        bufs.check()
        return res

    r = _both_fills(run)
    want = ls.gather_f32({k: attrs[k] for k in groups}, cut.ri, cut.pi, cut.w)
    for k in groups:
        got = r["o"][k].numpy()
        same = _bits(got) == _bits(want[k])
        assert same.all(), ("gather", k, int((~same).sum()), np.argwhere(~same)[:4].tolist())
    model = ls.scatter_f64({k: grads[k] for k in groups}, cut.ri, cut.pi, cut.w, G, rotations=attrs["rotations"])
    assert len(scattered) == 4
    for dd in scattered:
        ls.check_scatter({k: v.numpy() for k, v in dd.items()}, model)
    if emitted:
        assert r["flag"] == [0, 0], r["flag"]
        for k in groups:
            assert torch.equal(r["d"][0][k].view(torch.int32), r["d"][1][k].view(torch.int32)), ("second call", k)
    else:
        assert all(f != 0 for f in r["flag"]), r["flag"]


@pytest.mark.parametrize("M", [1, 4, 9, 16])
@pytest.mark.parametrize("name", ls.CUT_NAMES)
def test_entry_points_on_hand_built_cuts(gpu, name, M):
    _direct(gpu, ls.named_cut(name), M, GROUPS)


SUBSETS = [(("shs",), M) for M in (1, 4, 9, 16)] + [((k,), 9) for k in GROUPS if k != "shs"] + \
          [(tuple(k for k in GROUPS if k != "shs"), 9)]


@pytest.mark.parametrize("groups,M", SUBSETS, ids=["+".join(g) + f"-M{M}" for g, M in SUBSETS])
def test_entry_points_with_absent_groups(gpu, groups, M):
    """NULL for the groups that are not given: each group alone, and everything except the SH rows."""
    _direct(gpu, ls.named_cut("wave"), M, groups)


# ================================================================================================================
# 2. the in-op route through GaussianRasterizer
# ================================================================================================================
KEY = dict(means3D="xyz", scales="scaling", rotations="rotation", shs="features", opacities="opacity")
# (active degree, stored M, lod_scatter_in_kernel): M = 1, 9 can only take the through-memory glue branch
CONFIGS = [(0, 1, True), (1, 4, True), (1, 4, False), (2, 9, True), (3, 16, True), (3, 16, False), (1, 16, True),
           (1, 16, False)]
CONFIG_IDS = [f"deg{d}-M{M}-{'kernel' if k else 'memory'}" if (M * 3) % 4 == 0 else f"deg{d}-M{M}" for d, M, k in CONFIGS]
SKY = 10


def _cull_plan(cut, variant):
    """Rows of "seams" to put behind the camera.  Both variants: a run of three or more loses its leader, another run is
    culled whole.  "cull255": also rows 255 and 511, the last rows of their workgroups; "cull256": rows 256 and 512, the
    first rows of theirs (512 leads the second half of the run 510..513 there)."""
    runs = cut.runs()
    far = [(a, b) for a, b in runs if b <= 200]
    lead = next(a for a, b in far if b - a >= 3 and cut.w[a] > 0)
    whole = next((a, b) for a, b in far if b - a >= 2 and a != lead)
    single = {lead} | ({255, 511} if variant == "cull255" else {256, 512})
    assert all(cut.w[i] > 0 for i in single)
    return sorted(single), whole


def _case(name, M_store, cull=None):
    """Cut, camera and the full attribute arrays (CPU tensors; SKY more rows at the tail for the skybox cut)."""
    cut = ls.named_cut(name)
    sky = SKY if name == "skybox" else 0
    cam = synth.make_camera(W, H)
    deg_store = int(round(M_store ** 0.5)) - 1
    sc = synth.make_scene(cut.G + sky, cam, seed=31, sh_degree=deg_store, s_px=(1.0, 4.0))
    rot = sc.rotations.numpy().copy()
    rot[:cut.G] = ls.make_rotations(cut, **ls.forced_dots(cut))
    means = sc.means3D.numpy().copy()                  # the camera sits at the origin and looks down +z
    culled = np.zeros(cut.n + sky, dtype=bool)
    if cull is not None:
        single, (a, b) = _cull_plan(cut, cull)
        for i in single:
            w, zp = float(cut.w[i]), float(means[cut.pi[i], 2])
            means[cut.ri[i], 2] = (-2.0 - (1.0 - w) * zp) / w
            culled[i] = True
        means[cut.pi[a], 2] = -5.0
        means[cut.ri[a:b], 2] = -5.0
        culled[a:b] = True
    A = dict(means3D=torch.from_numpy(means), scales=sc.scales, rotations=torch.from_numpy(rot), shs=sc.shs,
             opacities=sc.opacities)
    counts = np.bincount(cut.pi, minlength=cut.G)
    kids = torch.from_numpy(counts[cut.pi].astype(np.int32))
    return cut, cam, A, kids, sky, culled


def _settings(cam, deg, gpu, ri, pi, w, kids):
    import diff_gaussian_rasterization as dgr
    kw = pa.settings_kwargs(cam, torch.zeros(3), deg, do_depth=False, device=gpu, interpolation_weights=w, num_node_kids=kids)
    kw["render_indices"], kw["parent_indices"] = ri, pi
    return dgr.GaussianRasterizationSettings(**kw)


def _upstream(gpu):
    return synth.upstream_grads(H, W)[0].to(gpu)


@pytest.fixture(scope="module")
def rows_cache():
    """The rows-route references of this module, computed once per (cut, degree, M, cull variant), freed at its end."""
    cache = {}
    yield cache
    cache.clear()


def _rows_route(gpu, cache, name, deg, M_store, cull=None):
    """The reference: the torch lerp of the reference glue feeds the op with empty indices, the lerped rows (and the
    skybox tail) are leaves.  Returns the image, the radii and the float64 model of the full-array gradients (shared
    through ``cache``, the rows_cache fixture)."""
    key = (name, deg, M_store, cull)
    if key in cache:
        return cache[key]
    import diff_gaussian_rasterization as dgr
    cut, cam, A, kids, sky, culled = _case(name, M_store, cull)
    G, n = cut.G, cut.n
    r, p = torch.from_numpy(cut.ri.astype(np.int64)).to(gpu), torch.from_numpy(cut.pi.astype(np.int64)).to(gpu)
    w = torch.from_numpy(cut.w).to(gpu)
    full = {KEY[k]: v.to(gpu) for k, v in A.items()}
    with torch.no_grad():
        L = bf.lod_lerp(full, r, p, w)
    leaves = {k: torch.cat((L[KEY[k]], full[KEY[k]][G:G + sky])).contiguous().requires_grad_(True) for k in GROUPS}
    w_ext = torch.cat((w, torch.ones(sky, device=gpu)))
    k_ext = torch.cat((kids.to(gpu), torch.ones(sky, dtype=torch.int32, device=gpu)))
    m2 = torch.zeros(n + sky, 3, device=gpu, requires_grad=True)
    e = torch.empty(0, dtype=torch.int32, device=gpu)
    color, radii, _ = dgr.GaussianRasterizer(_settings(cam, deg, gpu, e, e, w_ext, k_ext))(
        means3D=leaves["means3D"], means2D=m2, shs=leaves["shs"], opacities=leaves["opacities"],
        scales=leaves["scales"], rotations=leaves["rotations"])
    (color * _upstream(gpu)).sum().backward()
    radii_np = radii.cpu().numpy()
    # a condition on the inputs: exactly the chosen rows are off screen
    assert np.array_equal(radii_np == 0, culled), (np.flatnonzero(radii_np == 0).tolist(), np.flatnonzero(culled).tolist())
    g = {k: leaves[k].grad.cpu().numpy() for k in GROUPS}
    tail = np.arange(G, G + sky, dtype=np.int32)
    ri_x, pi_x = np.concatenate((cut.ri, tail)), np.concatenate((cut.pi, tail))       # skybox rows: their own parents,
    w_x = np.concatenate((cut.w, np.ones(sky, dtype=np.float32)))                     # weight 1
    model = ls.scatter_f64(g, ri_x, pi_x, w_x, G + sky, rotations=A["rotations"].numpy())
    out = dict(color=color.detach().cpu(), radii=radii.cpu(), m2=m2.grad.cpu(), model=model, row_grads=g)
    cache[key] = out
    return out


def _in_op(gpu, name, deg, M_store, in_kernel, cull=None, poison=None):
    """Full arrays + index tensors (+ the skybox count on the context).  ``poison``: rows whose every attribute is NaN."""
    import diff_gaussian_rasterization as dgr
    cut, cam, A, kids, sky, _ = _case(name, M_store, cull)
    B = {}
    for k, v in A.items():
        t = v.clone()
        if poison is not None and len(poison):
            t[torch.from_numpy(poison)] = float("nan")
        B[k] = t.to(gpu).requires_grad_(True)
    m2 = torch.zeros(cut.G + sky, 3, device=gpu, requires_grad=True)
    ctx = dgr.RasterContext(skybox_points=sky) if sky else None
    rs = _settings(cam, deg, gpu, torch.from_numpy(cut.ri).to(gpu), torch.from_numpy(cut.pi).to(gpu),
                   torch.from_numpy(cut.w).to(gpu), kids.to(gpu))
    dgr._C.lod_scatter_in_kernel = in_kernel
    try:
        color, radii, _ = dgr.GaussianRasterizer(rs, context=ctx)(
            means3D=B["means3D"], means2D=m2, shs=B["shs"], opacities=B["opacities"], scales=B["scales"],
            rotations=B["rotations"])
        call = color.grad_fn.call
        (color * _upstream(gpu)).sum().backward()
    finally:
        dgr._C.lod_scatter_in_kernel = True
    expect = int(in_kernel and (M_store * 3) % 4 == 0)
    assert call.args.lod_scatter == expect, (call.args.lod_scatter, expect)
    return dict(color=color.detach().cpu(), radii=radii.cpu(), m2=m2.grad[:cut.n + sky].cpu(),
                grads={k: B[k].grad.cpu() for k in GROUPS})


def _check_values(grads, model):
    got = {k: grads[k].numpy() for k in GROUPS}
    for k in GROUPS:                                   # the suite's rule for this comparison (tests/test_lod_gpu.py)
        ref = model[k].ref
        scale = float(np.abs(ref).max())
        err = float(np.abs(got[k].reshape(ref.shape).astype(np.float64) - ref).max())
        assert scale > 0 and err <= 2e-5 * scale, (k, err, scale)
    ls.check_rows(got, model, rel=2e-5)                # and per row; rows outside the cut exactly +0.0


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _fixed_rows(cut, total):
    """bool [total]: the rows whose gradient bits do not depend on the order of atomic adds, or None when no row's do
    (a shuffled cut).  On the emitted order a run cut by ONE workgroup boundary is two partial sums added to zero -- the
    same bits in either order; only the parent row of a run that lies in three or more workgroups is left out."""
    if cut.order != "emitted":
        return None
    fixed = np.ones(total, dtype=bool)
    for a, b in cut.runs():
        if (b - 1) // ls.BLOCK - a // ls.BLOCK >= 2:
            fixed[cut.pi[a]] = False
    return torch.from_numpy(fixed)


def _in_op_case(gpu, cache, name, deg, M_store, in_kernel, cull=None):
    cut = ls.named_cut(name)
    ref = _rows_route(gpu, cache, name, deg, M_store, cull)
    got = _in_op(gpu, name, deg, M_store, in_kernel, cull)
    assert torch.equal(ref["radii"], got["radii"])
    assert _same_bits(ref["color"], got["color"])
    _check_values(got["grads"], ref["model"])
    fixed = _fixed_rows(cut, got["grads"]["means3D"].shape[0])
    if fixed is not None:                              # (the 600-sibling run's parent row: the value rules only)
        again = _in_op(gpu, name, deg, M_store, in_kernel, cull)
        for k in GROUPS:
            assert _same_bits(got["grads"][k][fixed], again["grads"][k][fixed]), ("second run", k)
    return ref, got


@pytest.mark.parametrize("deg,M_store,in_kernel", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("name", ["wave", "seams", "long", "seams_shuf", "skybox"])
def test_in_op_route_matches_the_rows_route(gpu, rows_cache, name, deg, M_store, in_kernel):
    ref, got = _in_op_case(gpu, rows_cache, name, deg, M_store, in_kernel)
    if name == "skybox":                               # the tail starts mid-workgroup and crosses row 256
        n = ls.named_cut(name).n
        assert n < ls.BLOCK < n + SKY and int((got["radii"][n:] > 0).sum()) == SKY
        assert float(got["grads"]["shs"][-SKY:].abs().sum()) > 0


@pytest.mark.parametrize("deg,M_store,in_kernel", [(1, 4, True), (3, 16, True), (2, 9, True)],
                         ids=["deg1-M4-kernel", "deg3-M16-kernel", "deg2-M9"])
@pytest.mark.parametrize("cull", ["cull255", "cull256"])
def test_culled_rows_inside_runs(gpu, rows_cache, cull, deg, M_store, in_kernel):
    """Off-screen rows inside runs of "seams": a culled leader with a visible follower, a wholly culled run (its parent
    and its node rows get nothing), and a culled row on either side of the workgroup boundaries."""
    cut = ls.named_cut("seams")
    single, (a, b) = _cull_plan(cut, cull)
    runs = cut.runs()
    assert any(s == ra and rb - ra >= 2 for s in single for ra, rb in runs), "a culled leader with a visible follower"
    ref, got = _in_op_case(gpu, rows_cache, "seams", deg, M_store, in_kernel, cull)
    par = int(cut.pi[a])
    for k in GROUPS:
        assert not got["grads"][k][par].any() and not got["grads"][k][torch.from_numpy(cut.ri[a:b].astype(np.int64))].any()
    assert int((ref["radii"] == 0).sum()) == len(single) + (b - a)


@pytest.mark.parametrize("deg,M_store,in_kernel", [(1, 4, True), (3, 16, True), (2, 9, True)],
                         ids=["deg1-M4-kernel", "deg3-M16-kernel", "deg2-M9"])
@pytest.mark.parametrize("name", ["wave", "seams", "long", "seams_shuf"])
def test_weight_one_rule_parents_without_weight_may_hold_nan(gpu, rows_cache, name, deg, M_store, in_kernel):
    """gaussian_math.h: a non-finite parent attribute does not reach rows in which it has no weight (hgs.residency
    leaves such parents unfetched).  NaN in every attribute of each parent row that only weight-1 entries name: same
    image, finite gradients, exactly zero on the poisoned rows, the others as without the poison.  (Not a property of
    hgs_lod_gather: the stand-alone gather follows the torch expression, where 0 * NaN is NaN.)"""
    cut = ls.named_cut(name)
    has_weight = np.zeros(cut.G, dtype=bool)
    has_weight[cut.pi[cut.w != 1.0]] = True
    poison = np.setdiff1d(np.unique(cut.pi), np.flatnonzero(has_weight)).astype(np.int64)
    assert len(poison) >= 1 and not np.isin(poison, cut.ri).any()
    ref = _rows_route(gpu, rows_cache, name, deg, M_store)
    fixed = _fixed_rows(cut, cut.G)
    clean = _in_op(gpu, name, deg, M_store, in_kernel)
    got = _in_op(gpu, name, deg, M_store, in_kernel, poison=poison)
    assert _same_bits(clean["color"], got["color"]) and torch.equal(clean["radii"], got["radii"])
    assert _same_bits(clean["m2"], got["m2"])
    for k in GROUPS:
        g = got["grads"][k]
        assert bool(torch.isfinite(g).all()), k
        assert not g[torch.from_numpy(poison)].any(), k
        if fixed is not None:                          # every row but the parent of a run in three workgroups
            assert _same_bits(g[fixed], clean["grads"][k][fixed]), k
    _check_values(got["grads"], ref["model"])
