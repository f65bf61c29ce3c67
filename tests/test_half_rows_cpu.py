"""Half-precision hierarchy rows without a GPU: the 128-byte host row layout of include/hgs.h
in numpy (hgs.residency.pack_rows_half, the layout's specification), the narrowing rule by hand-written examples, the
compressed .hier writer (hgs_hier_write with HGS_HIER_UPSTREAM_HALF, write_hierarchy(half=True),
python -m hgs.compress_hierarchy), the refusals of the two new C calls that return before any HIP call, and what the
compiler reports for the two new kernels."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import half_rows_cases as hc
from hgs import _lib, residency

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hierarchical-3d-gaussians_amd")
ERR_INVALID = 1


def _last_error():
    msg = _lib.lib().hgs_last_error()
    return msg.decode() if msg else ""


# ---- the narrowing rule ---------------------------------------------------------------------------------------------
def test_narrowing_rule_by_hand_written_examples():
    got = residency.narrow_to_half(hc.NARROW_VALUES)
    for (v, want), g in zip(hc.NARROW_CASES, got):
        assert int(g) == want, f"{v!r}: 0x{int(g):04x}, expected 0x{want:04x}"
    finite = np.isfinite(hc.NARROW_VALUES)
    assert np.isfinite(hc.widen(got[finite])).all(), "a finite value became an infinity or a NaN"


def test_widening_is_exact_for_every_half():
    bits = np.arange(1 << 16, dtype=np.uint16)
    got, want = residency.widen_half(bits), hc.WIDEN_TABLE
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    # and narrowing a widened half gives the half back (NaNs: the quiet NaN 0x7e00 under their sign)
    back = residency.narrow_to_half(got)
    assert np.array_equal(back[~nan], bits[~nan])
    assert np.array_equal(back[nan], (bits[nan] & 0x8000) | 0x7E00)


# ---- the host row ---------------------------------------------------------------------------------------------------
def test_pack_rows_half_known_answers():
    """One row of M = 2 whose halves are chosen bit patterns (each exactly representable, so the expected bytes are the
    patterns themselves) between two other rows: every field at its documented byte offset, the mean's bytes the
    float32's, the padding zero."""
    M = 2
    sh_bits = np.array([0x3C00, 0xBC00, 0x0001, 0x83FF, 0x7BFF, 0x4248], np.uint16)
    rot_bits = np.array([0x3800, 0xB800, 0x0400, 0x8000], np.uint16)
    scale_bits = np.array([0x2E66, 0x0200, 0x5640], np.uint16)
    opac_bits = np.array([0x3B00], np.uint16)
    mean = np.array([[123456.789, -0.001953125, 3.0e-20]], np.float32)
    between = lambda mid: np.concatenate([np.ones_like(mid), mid, np.ones_like(mid)])       # rows of 1.0 on either side
    rows = residency.pack_rows_half(between(mean), between(hc.widen(sh_bits).reshape(1, M, 3)),
                                    between(hc.widen(opac_bits).reshape(1, 1)), between(hc.widen(scale_bits).reshape(1, 3)),
                                    between(hc.widen(rot_bits).reshape(1, 4)))
    assert rows.shape == (3, 128) and rows.dtype == np.uint8
    row = rows[1]
    u16 = lambda lo, hi: row[lo:hi].view(np.uint16)
    assert np.array_equal(u16(0, 12), sh_bits)
    assert not row[12:96].any(), "SH padding"
    assert np.array_equal(u16(96, 104), rot_bits)
    assert np.array_equal(u16(104, 110), scale_bits)
    assert np.array_equal(u16(110, 112), opac_bits)
    assert row[112:124].tobytes() == mean.tobytes()
    assert not row[124:128].any(), "tail padding"
    # the neighbours: 1.0 = 0x3c00 in every half, the mean 1.0f
    for other in (rows[0], rows[2]):
        assert (other[:12].view(np.uint16) == 0x3C00).all() and (other[96:112].view(np.uint16) == 0x3C00).all()
        assert other[112:124].tobytes() == np.ones(3, np.float32).tobytes() and not other[12:96].any()


@pytest.mark.parametrize("M", [1, 5, 16])
def test_pack_rows_half_narrows_every_field_and_round_rows_widens_it_again(M):
    G = 37
    arrays = hc.attribute_arrays(G, M, seed=M)
    rows = residency.pack_rows_half(*arrays)
    means3D, shs, opac, scales, rots = arrays
    halves = rows[:, :112].view(np.uint16)
    assert np.array_equal(halves[:, :3 * M], residency.narrow_to_half(shs.reshape(G, -1)))
    assert (halves[:, 3 * M:48] == 0).all() and not rows[:, 124:].any()
    assert np.array_equal(halves[:, 48:52], residency.narrow_to_half(rots))
    assert np.array_equal(halves[:, 52:55], residency.narrow_to_half(scales))
    assert np.array_equal(halves[:, 55], residency.narrow_to_half(opac[:, 0]))
    assert rows[:, 112:124].tobytes() == means3D.tobytes()
    rounded = residency.round_rows_to_half(*arrays)
    assert rounded[0].tobytes() == means3D.tobytes()
    for got, src in zip(rounded[1:], arrays[1:]):
        assert got.shape == src.shape and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), hc.widen(residency.narrow_to_half(src)).view(np.uint32))
    # tensors in, tensors out; rounding is idempotent, and the rounded arrays pack to the same rows
    as_t = residency.round_rows_to_half(*[torch.from_numpy(a) for a in arrays])
    assert all(torch.is_tensor(t) and t.numpy().tobytes() == r.tobytes() for t, r in zip(as_t, rounded))
    assert np.array_equal(residency.pack_rows_half(*rounded), rows)


def test_python_errors_come_before_any_device_call():
    """Unknown ``rows``, tensors in the wrong constructor, wrong dtypes and shapes: ValueError, on a machine without a GPU
    as well (nothing was allocated or launched)."""
    from hgs.residency import BudgetedHierarchy
    G, M = 5, 2
    ok = [torch.zeros(G, 3), torch.zeros(G, M, 3), torch.zeros(G, 1), torch.ones(G, 3), torch.ones(G, 4)]
    with pytest.raises(ValueError, match="rows must be 'float' or 'half'"):
        BudgetedHierarchy(*ok, "cuda:0", budget_rows=2, rows="bfloat16")
    with pytest.raises(ValueError, match="rows must be 'float' or 'half'"):
        BudgetedHierarchy.from_device_arrays(*ok, rows="fp8", budget_rows=2)
    with pytest.raises(ValueError, match="rows must be 'float' or 'half'"):
        BudgetedHierarchy.from_hier_file("/nonexistent.hier", "cuda:0", budget_rows=2, rows="HALF")
    with pytest.raises(ValueError, match="takes GPU tensors"):
        BudgetedHierarchy.from_device_arrays(*ok, rows="half", budget_rows=2)
    for i, bad in ((1, torch.zeros(G, M, 3, dtype=torch.float64)), (0, torch.zeros(G, 4)), (1, torch.zeros(G, 17, 3)),
                   (1, torch.zeros(G, M * 3)), (2, torch.zeros(G + 1)), (3, torch.ones(G, 4)), (4, torch.ones(G, 3)),
                   (4, torch.ones(G, 4, dtype=torch.float16))):
        a = list(ok)
        a[i] = bad
        for rows in ("float", "half"):
            with pytest.raises(ValueError):
                BudgetedHierarchy(*a, "cuda:0", budget_rows=2, rows=rows)
        with pytest.raises(ValueError):
            residency.pack_rows_half(*a)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="from_device_arrays"):
            BudgetedHierarchy(*[t.cuda() for t in ok], "cuda:0", budget_rows=2, rows="half")


# ---- the compressed .hier file ------------------------------------------------------------------------------------------
def _hier_arrays(P, N, M=16, seed=0):
    a = hc.attribute_arrays(P, M, seed)
    rng = np.random.default_rng(seed + 1)
    nodes = rng.integers(-5, 1 << 30, (N, 7)).astype(np.int32)
    boxes = rng.standard_normal((N, 2, 4)).astype(np.float32)
    t = torch.from_numpy
    # (xyz, shs, alpha, log_scales, rots, nodes, boxes), each field holding the tie and saturation cases
    return t(a[0]), t(a[1]), t(a[2]), t(a[3]), t(a[4]), t(nodes), t(boxes)


def test_write_hierarchy_half_round_trip(tmp_path):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    P, N = 5000, 4993                                   # (more than one 4096-value block of every array; a 7-row tail)
    src = _hier_arrays(P, N)
    path, again = str(tmp_path / "half.hier"), str(tmp_path / "again.hier")
    write_hierarchy(path, *src, half=True)
    assert os.path.getsize(path) == 4 + 124 * P + 4 + 60 * N
    assert np.fromfile(path, np.int32, 1)[0] == -P
    got = load_hierarchy(path)
    for k in (0, 5, 6):                                 # xyz, nodes, boxes: bit for bit
        assert got[k].shape == src[k].shape and got[k].numpy().tobytes() == src[k].numpy().tobytes(), k
    for k in (1, 2, 3, 4):
        want = hc.widen(residency.narrow_to_half(src[k].numpy()))
        assert got[k].shape == src[k].shape
        assert np.array_equal(got[k].numpy().view(np.uint32), want.view(np.uint32)), k
        assert np.isfinite(got[k].numpy()[np.isfinite(src[k].numpy())]).all(), "a finite value became an infinity"
    write_hierarchy(again, *got, half=True)             # compressing what was loaded changes nothing
    assert open(again, "rb").read() == open(path, "rb").read()


def test_write_hierarchy_half_refuses_other_sh_counts_and_float_output_is_unchanged(tmp_path):
    from gaussian_hierarchy._C import write_hierarchy
    small = _hier_arrays(40, 33, M=4)
    with pytest.raises(_lib.HgsError, match="exactly 16 SH coefficients"):
        write_hierarchy(str(tmp_path / "m4.hier"), *small, half=True)
    with pytest.raises(TypeError):                      # keyword only: the positional signature is the reference's
        write_hierarchy(str(tmp_path / "pos.hier"), *small, True)
    src = _hier_arrays(300, 293)
    a, b = str(tmp_path / "a.hier"), str(tmp_path / "b.hier")
    write_hierarchy(a, *src)
    write_hierarchy(b, *src, half=False)
    xyz, shs, alpha, log_scales, rots, nodes, boxes = [t.numpy() for t in src]
    today = b"".join([np.int32(300).tobytes(), xyz.tobytes(), rots.tobytes(), log_scales.tobytes(), alpha.tobytes(),
                      shs.tobytes(), np.int32(293).tobytes(), nodes.tobytes(), boxes.tobytes()])
    assert open(a, "rb").read() == today and open(b, "rb").read() == today


def test_compress_hierarchy_command_keeps_a_skybox_tail(tmp_path):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    P, N = 207, 200                                     # seven rows behind the node rows
    src = _hier_arrays(P, N, seed=3)
    inp, out = str(tmp_path / "in.hier"), str(tmp_path / "sub" / "out.hier")
    write_hierarchy(inp, *src)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-m", "hgs.compress_hierarchy", inp, out], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    size_in, size_out = 4 + 236 * P + 4 + 60 * N, 4 + 124 * P + 4 + 60 * N
    assert os.path.getsize(inp) == size_in and os.path.getsize(out) == size_out
    assert f"{size_in} bytes" in r.stdout and f"{size_out} bytes" in r.stdout and "207 rows (7 behind" in r.stdout
    got = load_hierarchy(out)
    assert got[0].shape[0] == P and got[5].shape[0] == N
    assert got[0].numpy().tobytes() == src[0].numpy().tobytes()
    assert np.array_equal(got[1].numpy()[N:].view(np.uint32),
                          hc.widen(residency.narrow_to_half(src[1].numpy()[N:])).view(np.uint32))
    # in process: the refusals
    from hgs import compress_hierarchy
    before = open(inp, "rb").read()
    assert compress_hierarchy.main([inp, inp]) == 2
    assert compress_hierarchy.main([inp, str(tmp_path / "." / "in.hier")]) == 2         # the same file by another name
    assert open(inp, "rb").read() == before
    assert compress_hierarchy.main([inp]) == 2
    assert compress_hierarchy.main([str(tmp_path / "missing.hier"), out]) == 2
    m4 = str(tmp_path / "m4.hier")
    write_hierarchy(m4, *_hier_arrays(20, 20, M=4))
    assert compress_hierarchy.main([m4, str(tmp_path / "m4_half.hier")]) == 1
    assert not os.path.exists(str(tmp_path / "m4_half.hier"))


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared():
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "hgs.h")).read()
    for name in ("hgs_resid_fetch_half", "hgs_resid_pack_rows"):
        assert f" T {name}\n" in nm, name
        assert name in _lib.SIGNATURES and name + "(" in header
    assert "#define HGS_RESID_HOST_ROW_BYTES_HALF 128" in header and _lib.RESID_HOST_ROW_BYTES_HALF == 128
    assert "#define HGS_ABI_VERSION 14" in header and _lib.ABI_VERSION == 14 and _lib.lib().hgs_abi_version() == 14


def test_fetch_half_refusals_before_any_hip_call():
    """Addresses that are never dereferenced: every refusal below returns before the device is touched (without a GPU a
    later check would fail with the HIP status instead)."""
    lib = _lib.lib()
    x = C.c_void_p(0x1000)
    rows = _lib.ResidRows(*[C.c_void_p(0x1000)] * 5)
    args = [x, 2, x, 5, x, x, x, 7, x, C.byref(rows), 16, None, 0]
    for i in (0, 2, 4, 5, 6, 8, 9):
        a = list(args)
        a[i] = None
        assert lib.hgs_resid_fetch_half(*a) == ERR_INVALID and "null" in _last_error(), i
    for M in (0, 17, -1):
        a = list(args)
        a[10] = M
        assert lib.hgs_resid_fetch_half(*a) == ERR_INVALID and "SH coefficients per channel: 1..16" in _last_error()
    a = list(args)
    a[3] = 1
    assert lib.hgs_resid_fetch_half(*a) == _lib.ERR_CAPACITY and "1 free slots for 2 missing rows" in _last_error()
    a = [None, 0, None, 0, None, None, None, 0, None, None, 0, None, 0]
    assert lib.hgs_resid_fetch_half(*a) == 0                        # m = 0 returns before any check


def test_pack_rows_refusals_before_any_hip_call():
    lib = _lib.lib()
    x = C.c_void_p(0x1000)
    rows = _lib.ResidRows(*[C.c_void_p(0x1000)] * 5)
    ok = [C.byref(rows), 10, 16, 1, x, None, 0]
    for i in (0, 4):
        a = list(ok)
        a[i] = None
        assert lib.hgs_resid_pack_rows(*a) == ERR_INVALID and "null" in _last_error(), i
    for k in range(5):
        ptrs = [C.c_void_p(0x1000)] * 5
        ptrs[k] = None
        a = list(ok)
        a[0] = C.byref(_lib.ResidRows(*ptrs))
        assert lib.hgs_resid_pack_rows(*a) == ERR_INVALID and "null" in _last_error(), k
    for i, v, what in ((1, -1, "rows"), (1, 1 << 31, "rows"), (2, 0, "SH coefficients"), (2, 17, "SH coefficients"),
                       (3, 2, "half ="), (3, -1, "half =")):
        a = list(ok)
        a[i] = v
        assert lib.hgs_resid_pack_rows(*a) == ERR_INVALID and what in _last_error(), (i, v, _last_error())
    for half in (0, 1):
        a = list(ok)
        a[1], a[3] = 0, half
        assert lib.hgs_resid_pack_rows(*a) == 0                     # G = 0: nothing to do, no HIP call


# ---- what the compiler reports ------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("c++filt")),
                    reason="needs hipcc (cross-compiles without a GPU) and c++filt")
def test_new_kernels_use_no_scratch_and_no_lds():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    rows = kernel_resources.collect([os.path.join(PKG, "csrc", "residency.hip")])
    by = {}
    for r in rows:
        by.setdefault(r["kernel"].split("<")[0], []).append(r)
    assert len(by.get("resid_fetch_half_kernel", [])) == 2 and len(by.get("resid_pack_kernel", [])) == 2, sorted(by)
    for name in ("resid_fetch_half_kernel", "resid_pack_kernel"):
        for r in by[name]:
            assert r["scratch"] == 0 and r["spills"] == 0 and r["lds"] == 0, (r["kernel"], r["scratch"], r["spills"], r["lds"])
