"""tests/lod_gather_spec.py without a GPU: the float64 adjoint against torch autograd of the shared lerp, the float32
gather bit for bit against the rows the reference's render_post recorded in the boundary goldens, the builder's cuts,
and four wrong scatters that the two acceptance rules must reject."""
import os

import numpy as np
import pytest
import torch

import boundary_fixtures as bf
import lod_gather_spec as ls

ALL_CUTS = ls.CUT_NAMES + ("long_shuf", "skybox")
KEY = dict(means3D="xyz", scales="scaling", rotations="rotation", shs="features", opacities="opacity")


def _case(name, M=4):
    cut = ls.named_cut(name)
    return cut, ls.make_attrs(cut, M), ls.make_row_grads(cut, M)


@pytest.mark.parametrize("name", ALL_CUTS)
def test_built_cuts_are_valid(name):
    cut = ls.named_cut(name)
    ls.check_cut(cut)
    if cut.n >= 4:
        for v in ls.SPECIAL_WEIGHTS:
            assert (cut.w == np.float32(v)).any(), v
    ordinary = cut.w[~np.isin(cut.w, np.array(ls.SPECIAL_WEIGHTS, dtype=np.float32))]
    assert ((ordinary >= 0.05) & (ordinary <= 0.95)).all()
    if name.endswith("_shuf"):
        owners = [int(cut.pi[a]) for a, _ in cut.runs()]
        assert len(owners) > len(set(owners)) and bool((np.diff(cut.pi) < 0).any())
    if name == "root":
        assert cut.n == 1 and cut.ri[0] == cut.pi[0]
    if name in ("wave", "seams", "long", "skybox"):       # a parent that has no weight in any row (the weight-1 rule)
        u = 1.0 - cut.w.astype(np.float64)
        mass = np.zeros(cut.G)
        np.add.at(mass, cut.pi, u)
        assert ((mass == 0) & np.isin(np.arange(cut.G), cut.pi)).any()


@pytest.mark.parametrize("name", ALL_CUTS)
def test_forced_dot_products(name):
    cut = ls.named_cut(name)
    f = ls.forced_dots(cut)
    q = ls.make_rotations(cut, **f)                       # (asserts every pair's float64 dot product itself)
    assert np.allclose(np.linalg.norm(q.astype(np.float64), axis=1), 1.0, atol=1e-6)
    s = ls.flip_signs(q, cut.ri, cut.pi)
    assert set(np.flatnonzero(s < 0).tolist()) == set(f["negative"])
    if name in ("wave", "seams", "long"):
        assert f["zero"] and f["neg_zero"] and f["negative"]
    if name == "seams":                                   # negative pairs on both sides of both workgroup boundaries
        assert {255, 256, 511, 512} <= set(f["negative"])


@pytest.mark.parametrize("name", ALL_CUTS)
def test_scatter_f64_is_the_autograd_of_the_shared_lerp(name):
    cut, attrs, grads = _case(name)
    leaves = {KEY[k]: torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for k, v in attrs.items()}
    rows = bf.lod_lerp(leaves, torch.from_numpy(cut.ri.astype(np.int64)), torch.from_numpy(cut.pi.astype(np.int64)),
                       torch.from_numpy(cut.w.astype(np.float64)))
    loss = sum((rows[KEY[k]] * torch.from_numpy(g.astype(np.float64))).sum() for k, g in grads.items())
    loss.backward()
    model = ls.scatter_f64(grads, cut.ri, cut.pi, cut.w, cut.G, rotations=attrs["rotations"])
    for k, m in model.items():
        got = leaves[KEY[k]].grad.numpy().reshape(m.ref.shape)
        assert (np.abs(got - m.ref) <= 1e-13 * m.mass + 1e-300).all(), k
        assert not got[~m.touched].any()
        # terms and mass: counted independently, entry by entry
        terms = np.zeros(cut.G, dtype=np.int64)
        for r, p in zip(cut.ri, cut.pi):
            terms[r] += 1
            if p != r:
                terms[p] += 1
        assert np.array_equal(m.terms, np.broadcast_to(terms[:, None], m.terms.shape))
        assert (m.mass >= np.abs(m.ref) * (1 - 1e-12)).all()


LOD_GOLDENS = bf.cases("lod")


@pytest.mark.parametrize("fname,lod", LOD_GOLDENS, ids=[f"{f[:-4]}-{p}" for f, p in LOD_GOLDENS])
def test_gather_f32_reproduces_the_recorded_rows_bit_for_bit(fname, lod):
    z = bf.load(os.path.join(bf.GOLDEN, fname))
    op = f"op{int(z[f'{lod}__op'])}"
    full = {k: z[f"{lod}__full__{k}"] for k in bf.FULL}
    ri = z[f"{lod}__render_indices"]
    n = ri.size
    pi, w = z[f"{lod}__parent_indices"][:n], z[f"{lod}__weights"][:n]
    rows = ls.gather_f32(full, ri, pi, w, rot_key="rotation")
    for k in bf.FULL:
        want = z[f"{op}__arg__{bf.ROW_ARG[k]}"][:n]
        assert np.array_equal(rows[k].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), k


def test_at_least_one_golden_holds_a_lod_lerp():
    assert len(LOD_GOLDENS) >= 1


# ---- mutation checks ---------------------------------------------------------------------------------------------------
def _ordinary(w):
    return 0.05 <= float(w) <= 0.95


def _scatter_f32(cut, grads, rotations, mutation=None):
    """A plain float32 scatter in row order (u = f32(1) - w, rounded products, rounded running sums) -- with one of the
    named defects when ``mutation`` is given.  Returns None when the defect cannot occur on this cut."""
    f = np.float32
    n = cut.n
    sign = ls.flip_signs(rotations, cut.ri, cut.pi)
    self_par = cut.ri == cut.pi
    skip_parent, twice = set(), set()
    if mutation == "drop_last_sibling":
        pick = [b - 1 for a, b in cut.runs() if b - a >= 2 and not self_par[a] and _ordinary(cut.w[b - 1])]
        if not pick:
            return None
        skip_parent.add(pick[0])
    elif mutation == "ignore_sign":
        if not any(sign[i] < 0 and not self_par[i] and cut.w[i] <= 0.95 for i in range(n)):
            return None
        sign = np.ones(n, dtype=f)
    elif mutation == "swap_weights":
        if not any(not self_par[i] and cut.w[i] != 0.5 for i in range(n)):
            return None
    elif mutation == "second_half_twice":
        for a, b in cut.runs():
            seam = (a // ls.BLOCK + 1) * ls.BLOCK
            if seam < b and not self_par[a] and any(_ordinary(cut.w[j]) for j in range(seam, b)):
                twice = set(range(seam, b))
                break
        else:
            return None
    else:
        assert mutation is None
    out = {}
    for k, g in grads.items():
        g2 = g.reshape(n, -1)
        d = np.zeros((cut.G, g2.shape[1]), dtype=f)
        for i in range(n):
            r, p = int(cut.ri[i]), int(cut.pi[i])
            w = f(cut.w[i])
            u = f(f(1.0) - w)
            if mutation == "swap_weights" and r != p:
                w, u = u, w
            if r == p:
                d[r] += g2[i]
                continue
            d[r] += w * g2[i]
            if i in skip_parent:
                continue
            s = sign[i] if k == "rotations" else f(1.0)
            for _ in range(2 if i in twice else 1):
                d[p] += (u * s) * g2[i]
        out[k] = d.reshape((cut.G,) + g.shape[1:])
    return out


MUTATIONS = ("drop_last_sibling", "ignore_sign", "swap_weights", "second_half_twice")
_CASES = {name: _case(name) for name in ALL_CUTS}
POSSIBLE = [(name, m) for name in ALL_CUTS for m in MUTATIONS
            if _scatter_f32(_CASES[name][0], {"opacities": _CASES[name][2]["opacities"]}, _CASES[name][1]["rotations"], m)
            is not None]


def test_every_mutation_is_possible_where_the_geometry_allows_it():
    got = set(POSSIBLE)
    for name in ("wave", "seams", "long", "wave_shuf", "seams_shuf", "skybox"):
        assert {(name, m) for m in MUTATIONS[:3]} <= got, name
    assert ("pair", "drop_last_sibling") in got or ("pair", "swap_weights") in got
    assert {("seams", "second_half_twice"), ("long", "second_half_twice")} <= got
    assert not any(name == "root" for name, _ in got)         # a self-parent row is the identity: nothing to get wrong


@pytest.mark.parametrize("name", ALL_CUTS)
def test_a_plain_float32_scatter_passes_both_rules(name):
    cut, attrs, grads = _CASES[name]
    model = ls.scatter_f64(grads, cut.ri, cut.pi, cut.w, cut.G, rotations=attrs["rotations"])
    got = _scatter_f32(cut, grads, attrs["rotations"])
    ls.check_scatter(got, model)
    ls.check_rows(got, model)


@pytest.mark.parametrize("name,mutation", POSSIBLE)
def test_wrong_scatters_are_rejected(name, mutation):
    cut, attrs, grads = _CASES[name]
    model = ls.scatter_f64(grads, cut.ri, cut.pi, cut.w, cut.G, rotations=attrs["rotations"])
    got = _scatter_f32(cut, grads, attrs["rotations"], mutation)
    with pytest.raises(AssertionError):
        ls.check_scatter(got, model)
    with pytest.raises(AssertionError):
        ls.check_rows(got, model)
    if mutation != "ignore_sign":          # (the sign is the quaternions' alone) every other defect shows in every group
        for k in got:
            with pytest.raises(AssertionError):
                ls.check_scatter({k: got[k]}, {k: model[k]})


def test_a_value_outside_the_cut_is_rejected_even_when_it_is_minus_zero():
    cut, attrs, grads = _CASES["wave"]
    model = ls.scatter_f64(grads, cut.ri, cut.pi, cut.w, cut.G, rotations=attrs["rotations"])
    got = _scatter_f32(cut, grads, attrs["rotations"])
    row = int(np.flatnonzero(~model["means3D"].touched)[0])
    got["means3D"][row, 1] = -0.0
    with pytest.raises(AssertionError):
        ls.check_scatter(got, model)
    with pytest.raises(AssertionError):
        ls.check_rows(got, model)
