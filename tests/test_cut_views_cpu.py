"""The cut for several views without a GPU (csrc/lod_views.hip, hgs.frustum.cut_views): the workspace query, what the
C ABI refuses before it touches a device, the constant the ctypes layer repeats, and the new kernels' static
resources."""
import ctypes as C
import os
import re
import shutil
import sys

import pytest
import torch

from hgs import _lib, frustum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_call_exists_and_its_constant_matches_the_header():
    assert callable(getattr(frustum, "cut_views", None))
    assert hasattr(_lib.lib(), "hgs_lod_cut_views")
    src = open(os.path.join(ROOT, "include", "hgs.h")).read()
    assert int(re.search(r"#define\s+HGS_CUT_MAX_VIEWS\s+(\d+)", src).group(1)) == _lib.CUT_MAX_VIEWS == 16
    assert int(re.search(r"#define\s+HGS_ABI_VERSION\s+(\d+)", src).group(1)) == 14      # additive: the number stays


def test_workspace_query():
    q = _lib.lib().hgs_lod_cut_views_tmp_bytes
    for V in (1, 3, 16):
        assert q(0, V) == q(1, V)
    sizes = (0, 1, 255, 256, 257, 1000, 65536, 65537, 10_000_000)
    for V in range(1, 17):
        vals = [q(N, V) for N in sizes]
        assert vals == sorted(vals), (V, vals)                     # non-decreasing in N
    for N in sizes:
        vals = [q(N, V) for V in range(1, 17)]
        assert vals == sorted(vals), (N, vals)                     # ... and in V
    # V emission counts per node, and per view the kept sums (+ 2 totals), the unculled sums and one scan chunk's word
    N, V, nblk = 1000, 3, 4
    assert q(N, V) >= V * 4 * N + V * (4 * (nblk + 2) + 4 * nblk + 8)
    assert q(2 ** 31 - 1, 16) >= 16 * 4 * (2 ** 31 - 1)             # computed in 64 bits


def test_the_c_abi_refuses_bad_arguments_before_any_hip_call():
    """Null pointers, V outside 1..16, a negative capacity, bounds without planes and the reverse: refused on the host
    (this machine may have no GPU at all), each with a message; N <= 0 is an empty answer; the next query works."""
    lib = _lib.lib()
    buf = (C.c_int32 * 64)()
    a = C.cast(buf, C.c_void_p)
    fl = lambda n: (C.c_float * n)()
    counts, unc, offs, need = (C.c_int32 * 16)(), (C.c_int32 * 16)(), (C.c_int32 * 16)(), C.c_int64(7)

    def call(nodes=a, boxes=a, bounds=None, N=4, V=2, sizes=fl(16), vps=fl(48), planes=None, rs=fl(16), out=a, cap=8,
             tmp=a, res=(counts, unc, offs, C.byref(need))):
        return lib.hgs_lod_cut_views(nodes, boxes, bounds, N, V, sizes, vps, planes, rs, out, out, out, out, out, cap,
                                     tmp, res[0], res[1], res[2], res[3], None, 0)

    for kw, word in ((dict(nodes=None), b"null"), (dict(boxes=None), b"null"), (dict(sizes=None), b"null"),
                     (dict(vps=None), b"null"), (dict(rs=None), b"null"), (dict(out=None), b"null"),
                     (dict(tmp=None), b"null"), (dict(res=(None, unc, offs, C.byref(need))), b"null"),
                     (dict(res=(counts, None, offs, C.byref(need))), b"null"),
                     (dict(res=(counts, unc, None, C.byref(need))), b"null"),
                     (dict(res=(counts, unc, offs, None)), b"null"), (dict(V=0), b"V = 0"), (dict(V=-1), b"V = -1"),
                     (dict(V=17), b"V = 17"), (dict(cap=-1), b"capacity = -1"), (dict(bounds=a), b"go together"),
                     (dict(planes=fl(320)), b"go together")):
        assert call(**kw) == 1, kw
        assert word in lib.hgs_last_error(), (kw, lib.hgs_last_error())
    for i in range(16):
        counts[i] = unc[i] = offs[i] = 7
    for N in (0, -3):
        assert call(N=N, V=16) == 0
        assert list(counts) == [0] * 16 and list(unc) == [0] * 16 and list(offs) == [0] * 16 and need.value == 0
    assert lib.hgs_lod_cut_views_tmp_bytes(1000, 3) > 0


def test_cut_views_refuses_bad_arguments_without_touching_the_gpu():
    nodes = torch.zeros(3, 7, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU tensor"):
        frustum.cut_views(nodes, torch.zeros(3, 2, 4), None, [0.1], torch.zeros(1, 3))
    with pytest.raises(ValueError, match="go together"):
        frustum.cut_views(nodes, torch.zeros(3, 2, 4), None, [0.1], torch.zeros(1, 3), planes=torch.zeros(1, 5, 4))
    with pytest.raises(ValueError, match="go together"):
        frustum.cut_views(nodes, torch.zeros(3, 2, 4), torch.zeros(3, 4), [0.1], torch.zeros(1, 3))


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("c++filt")),
                    reason="needs hipcc (cross-compiles without a GPU) and c++filt")
def test_no_views_kernel_uses_scratch_or_doubles():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    rows = kernel_resources.collect([os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc", "lod_views.hip")])
    names = {r["kernel"] for r in rows}
    assert {"views_mark_kernel", "views_scan_cull_kernel", "views_scan_kernel", "views_emit_kernel"} <= \
        {n.split("<")[0] for n in names}, names
    for r in rows:
        assert r["scratch"] == 0, (r["kernel"], r["scratch"])
        assert r["mix"]["valu_f64"] == 0, r["kernel"]
        assert r["waves_regs"] >= 8, (r["kernel"], r["vgpr"])
