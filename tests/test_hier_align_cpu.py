"""The rotation-alignment rule (hgs.hierarchy.align_hierarchy, the float64 numpy spec) on numpy-built hierarchies, and the
host side of the device call (no GPU): what the rule must leave alone, what it must achieve, that it is idempotent, that
the unaligned input really is far from aligned, the size and pointer checks of the C ABI, and the ``--align`` flag of the
creator and merger commands."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from hgs import _lib, create_hierarchy, hierarchy, merge_hierarchies, synth
from hgs import align_hierarchy as align_cmd

CAM = synth.make_camera(640, 360)
KINDS = {"uniform": synth.make_scene, "trained_like": synth.make_scene_trained_like}
SIZES = [1, 2, 3, 257, 2000]
CASES = [(k, P) for k in KINDS for P in SIZES]
BOUND = (2.0 + np.sqrt(2.0)) / 4.0


@functools.lru_cache(maxsize=None)
def case(kind, P):
    """-> (the numpy-built hierarchy, its alignment, the chosen group element per node); computed once, never modified."""
    h = hierarchy.build_hierarchy(KINDS[kind](P, CAM, seed=3))
    choice = np.zeros(h.num_nodes, dtype=np.int64)
    return h, hierarchy.align_hierarchy(h, choice), choice


def bits(t):
    return t.contiguous().view(torch.int32)


def cov(log_scales, rots):
    """[n,3,3] float64 covariance R(q / |q|) diag(exp(2 log_scales)) R^T."""
    q = np.asarray(rots, dtype=np.float64)
    R = hierarchy._rot_from_quat(q / np.linalg.norm(q, axis=1, keepdims=True))
    L = R * np.exp(np.asarray(log_scales, dtype=np.float64))[:, None, :]
    return L @ L.transpose(0, 2, 1)


def signed_dots(h):
    """<q_i, q_parent> of the normalised quaternions at every node of depth > 0 (float64), and those nodes."""
    nodes = h.nodes.numpy()
    N = nodes.shape[0]
    q = h.rots[:N].double().numpy()
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    ids = np.nonzero(nodes[:, 0] > 0)[0]
    return (q[ids] * q[nodes[ids, 1]]).sum(1), ids


def best_alternative(h):
    """The largest |<q_i (x) g_j, q_parent>| over the 24 group elements, recomputed from ``h`` itself (normalised)."""
    nodes = h.nodes.numpy()
    N = nodes.shape[0]
    q = h.rots[:N].double().numpy()
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    ids = np.nonzero(nodes[:, 0] > 0)[0]
    g, _ = hierarchy.align_group()
    c = hierarchy._quat_mul(q[ids][:, None, :], g[None])
    return np.abs((c * q[nodes[ids, 1]][:, None, :]).sum(2)).max(1)


def detour(h):
    """Mean over the non-root nodes of || C(lerp at t = 0.5) - (C_i + C_p) / 2 ||_F / || (C_i + C_p) / 2 ||_F, the lerp
    being the renderer's: activated scales component by component, normalised quaternions after a sign flip."""
    nodes = h.nodes.numpy()
    N = nodes.shape[0]
    ids = np.nonzero(nodes[:, 0] > 0)[0]
    par = nodes[ids, 1]
    ls, q = h.log_scales[:N].double().numpy(), h.rots[:N].double().numpy()
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    qi, qp = q[ids], q[par]
    qp = np.where((qi * qp).sum(1, keepdims=True) < 0, -qp, qp)
    s = 0.5 * np.exp(ls[ids]) + 0.5 * np.exp(ls[par])
    mid = cov(np.log(s), 0.5 * qi + 0.5 * qp)
    mean = 0.5 * (cov(ls[ids], qi) + cov(ls[par], q[par]))
    return float((np.linalg.norm(mid - mean, axis=(1, 2)) / np.linalg.norm(mean, axis=(1, 2))).mean())


def check_properties(h, a):
    """Properties 1-5 of an alignment ``a`` of ``h`` (host hierarchies); the device tests reuse this."""
    N = h.num_nodes
    # 1. what the rule does not touch
    for k in ("nodes", "boxes", "xyz", "shs", "alpha"):
        assert torch.equal(bits(getattr(a, k)), bits(getattr(h, k))), k
    root = int(np.nonzero(h.nodes.numpy()[:, 0] == 0)[0][0])
    for k in ("log_scales", "rots"):
        assert torch.equal(bits(getattr(a, k)[root]), bits(getattr(h, k)[root])), f"root {k}"
        assert torch.equal(bits(getattr(a, k)[N:]), bits(getattr(h, k)[N:])), f"{k} behind the node rows"
    # 2. scales: a bitwise permutation per row
    assert torch.equal(bits(a.log_scales[:N]).sort(1).values, bits(h.log_scales[:N]).sort(1).values)
    # 3. the Gaussian and the quaternion norm
    c0, c1 = cov(h.log_scales[:N], h.rots[:N]), cov(a.log_scales[:N], a.rots[:N])
    rel = np.linalg.norm(c1 - c0, axis=(1, 2)) / np.linalg.norm(c0, axis=(1, 2))
    assert float(rel.max()) <= 1e-6, (float(rel.max()), int(rel.argmax()))
    n0, n1 = h.rots[:N].double().norm(dim=1), a.rots[:N].double().norm(dim=1)
    assert float(((n1 - n0).abs() / n0).max()) <= 1e-6
    if N == 1:
        return
    # 4. close to the parent, the sign folded in
    d, _ = signed_dots(a)
    assert float(d.min()) >= 0.0 and float(d.min()) >= BOUND - 1e-6, float(d.min())
    # 5. none of the 24 alternatives is better
    assert float((best_alternative(a) - d).max()) <= 1e-6


@pytest.mark.parametrize("kind,P", CASES)
def test_alignment_properties(kind, P):
    h, a, _ = case(kind, P)
    check_properties(h, a)
    assert a.rots.dtype == torch.float32 and a.log_scales.dtype == torch.float32 and not a.rots.is_cuda


@pytest.mark.parametrize("kind,P", CASES)
def test_a_second_alignment_changes_no_bit(kind, P):
    _, a, _ = case(kind, P)
    choice = np.full(a.num_nodes, -1, dtype=np.int64)
    b = hierarchy.align_hierarchy(a, choice)
    assert torch.equal(bits(b.rots), bits(a.rots)) and torch.equal(bits(b.log_scales), bits(a.log_scales))
    assert int(np.abs(choice).max()) == 0            # the identity everywhere: the bits are the input's own


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("P", [257, 2000])
def test_the_unaligned_input_is_far_from_aligned(kind, P):
    """Negative control for properties 4 and 8: the builder's canonical frames and the leaves' trained frames violate
    the bound at most nodes, and the renderer's half-way lerp detours further through them."""
    h, a, choice = case(kind, P)
    d = hierarchy.alignment_dots(h)
    assert float((d < BOUND).mean()) > 0.5, float((d < BOUND).mean())
    assert float((hierarchy.alignment_dots(a) < BOUND).mean()) == 0.0
    assert int((choice != 0).sum()) > P // 2
    before, after = detour(h), detour(a)
    assert after < before, (before, after)


@pytest.mark.parametrize("kind,P", [("uniform", 3), ("trained_like", 257), ("uniform", 2000)])
def test_the_torch_statement_of_the_rule_agrees(kind, P):
    """tests/align_spec.py (what scripts/bench_align.py times beside the HIP call) against the numpy spec, bit for bit."""
    import align_spec
    h, a, _ = case(kind, P)
    t = align_spec.align_torch(hierarchy.Hierarchy(h.xyz, h.shs, h.alpha, h.log_scales.clone(), h.rots.clone(), h.nodes,
                                                   h.boxes))
    assert torch.equal(bits(t.rots), bits(a.rots)) and torch.equal(bits(t.log_scales), bits(a.log_scales))


def test_the_group():
    g, perms = hierarchy.align_group()
    assert g.shape == (24, 4) and perms.shape == (24, 3)
    assert np.array_equal(g[0], [1.0, 0.0, 0.0, 0.0]) and list(perms[0]) == [0, 1, 2]
    R = hierarchy._rot_from_quat(g)
    assert np.allclose(np.abs(R).sum(1), 1.0, atol=1e-15) and np.allclose(np.linalg.det(R), 1.0)
    for j in range(24):                              # column k of M is +- e_perm[k]
        assert [int(np.abs(R[j][:, k]).argmax()) for k in range(3)] == list(perms[j])
    assert len({tuple(np.round(r.reshape(-1)).astype(int)) for r in R}) == 24


def test_rows_behind_the_nodes_and_unnormalised_quaternions_are_kept():
    """A skybox tail (rows at index >= N) is not touched; a quaternion that is not normalised keeps its norm; a dot of
    exactly zero takes the + sign; the identity element hands the input's bits through or negates them exactly."""
    h, _, _ = case("uniform", 257)
    g = torch.Generator().manual_seed(5)
    scale = 0.25 + 3.0 * torch.rand(h.num_nodes, 1, generator=g)
    tail = lambda t, *s: torch.cat([t, torch.randn(7, *s, generator=g)])
    ht = hierarchy.Hierarchy(tail(h.xyz, 3), tail(h.shs, 16, 3), tail(h.alpha, 1).abs(), tail(h.log_scales, 3),
                             tail(h.rots * scale, 4), h.nodes, h.boxes)
    check_properties(ht, hierarchy.align_hierarchy(ht))
    q = np.array([[0.3, -0.2, 0.9, 0.1], [0.0, 1.0, 0.0, 0.0]], dtype=np.float32)
    j, neg, best = hierarchy.align_choice(q, np.array([[-0.3, 0.2, -0.9, -0.1], [1.0, 0.0, 0.0, 0.0]], dtype=np.float32))
    assert list(j) == [0, 1] and list(neg) == [True, True]        # i (x) i = -1: the half turn about x, negated
    assert np.array_equal(best[0].view(np.uint32), (-q[0]).view(np.uint32))
    assert np.array_equal(best[1], np.array([1.0, 0.0, 0.0, 0.0], dtype=np.float32))
    j, neg, _ = hierarchy.align_choice(np.zeros((1, 4), np.float32), q[:1])
    assert list(j) == [0] and list(neg) == [False]


def test_tmp_bytes_needs_no_gpu():
    lib = _lib.lib()
    for N in (0, -1, 1 << 31, 1 << 40, -(1 << 40)):
        assert lib.hgs_hier_align_tmp_bytes(N) == 0, N
    prev = 0
    for N in (1, 3, 513, 3999, 50_000_000, (1 << 31) - 1):
        b = lib.hgs_hier_align_tmp_bytes(N)
        assert b >= 12 * N + 1024 + 32 and b % 256 == 0 and b >= prev, (N, b)
        prev = b


def test_bad_arguments_fail_before_any_hip_call():
    """(No GPU here: a call that got as far as HIP would return HGS_ERR_HIP, not HGS_ERR_INVALID.)"""
    lib = _lib.lib()
    rep = _lib.HierAlignReport()
    a = 4096                                   # any non-null, aligned address: it is never dereferenced
    cases = [((a, 0, a, a, a, C.byref(rep)), b"bad sizes"), ((a, -5, a, a, a, C.byref(rep)), b"bad sizes"),
             ((a, 1 << 31, a, a, a, C.byref(rep)), b"bad sizes"), ((None, 5, a, a, a, C.byref(rep)), b"null"),
             ((a, 5, None, a, a, C.byref(rep)), b"null"), ((a, 5, a, None, a, C.byref(rep)), b"null"),
             ((a, 5, a, a, None, C.byref(rep)), b"null"), ((a, 5, a, a, a, None), b"null"),
             ((a, 5, a, a + 8, a, C.byref(rep)), b"16-byte"), ((a, 5, a, a, a + 64, C.byref(rep)), b"256-byte")]
    for args, word in cases:
        assert lib.hgs_hier_align(*args, None, 0) == 1, args
        assert word in lib.hgs_last_error(), (args, lib.hgs_last_error())


def test_the_align_flag_leaves_the_positional_arguments_alone():
    pos = ["pc.ply", "chunk", "out", "scaffold"]
    assert create_hierarchy.split_flags(pos) == (pos, set())
    assert create_hierarchy.split_flags(pos[:3]) == (pos[:3], set())
    for at in range(5):
        argv = pos[:at] + ["--align"] + pos[at:]
        assert create_hierarchy.split_flags(argv) == (pos, {"--align"})
    merge = ["trained", "0", "chunks", "out.hier", "a", "b"]
    assert create_hierarchy.split_flags(merge) == (merge, set())
    assert create_hierarchy.split_flags(merge + ["--align"]) == (merge, {"--align"})
    # the usage errors are those of the flagless forms
    assert create_hierarchy.main(["--align", "only", "two"]) == 2
    assert merge_hierarchies.main(["--align", "trained", "0", "chunks", "out.hier"]) == 2
    assert merge_hierarchies.main(["trained", "1", "--align", "chunks", "out.hier", "a"]) == 2
    assert align_cmd.main([]) == 2 and align_cmd.main(["a.hier"]) == 2 and align_cmd.main(["a", "b", "c"]) == 2
    assert align_cmd.main(["/nonexistent/in.hier", "out.hier"]) == 2


def test_the_flags_default_to_off():
    import inspect
    for fn in (hierarchy.build_hierarchy_gpu, hierarchy.merge_hierarchies_gpu, create_hierarchy.run,
               merge_hierarchies.run):
        assert inspect.signature(fn).parameters["align"].default is False, fn
