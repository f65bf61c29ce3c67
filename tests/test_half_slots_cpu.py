"""Half-precision residency SLOTS without a GPU (hgs/residency.py ``slots="half"``, include/hgs.h: lod_half_rows,
hgs_resid_fetch_half_slots): the argument checks that come before any device use, the ABI word
the switch lives in, and the row-byte arithmetic a budget is counted in."""
import ctypes as C
import os
import re

import pytest
import torch

import half_rows_cases as hc
from hgs import _lib, residency
from hgs.residency import BudgetedHierarchy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "hgs.h")).read()


def _arrays(G=10, M=2):
    return [torch.from_numpy(a) for a in hc.attribute_arrays(G, M, seed=1, with_cases=False)]


def _no_device(monkeypatch):
    """Any touch of the device (pinned memory, a slot array) fails the test instead of being skipped."""
    def boom(*a, **k):
        raise AssertionError("the device was touched before the argument check")
    monkeypatch.setattr(residency, "_host_array", boom)
    monkeypatch.setattr(BudgetedHierarchy, "_setup", boom)


def test_half_slots_need_half_rows_and_say_why(monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="narrowing float host rows on fetch is not part"):
        BudgetedHierarchy(*_arrays(), "cuda:0", budget_rows=4, rows="float", slots="half")
    with pytest.raises(ValueError, match="rows='half'"):
        BudgetedHierarchy(*_arrays(), "cuda:0", budget_rows=4, slots="half")            # (rows defaults to float)
    with pytest.raises(ValueError, match="narrowing"):
        BudgetedHierarchy.from_hier_file("/nonexistent/scene.hier", "cuda:0", budget_rows=4, slots="half")


@pytest.mark.parametrize("rows", ["float", "half"])
def test_unknown_slots_value_is_refused_before_any_device_use(monkeypatch, rows):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="slots must be 'float' or 'half', not 'bfloat'"):
        BudgetedHierarchy(*_arrays(), "cuda:0", budget_rows=4, rows=rows, slots="bfloat")
    with pytest.raises(ValueError, match="slots must be"):
        BudgetedHierarchy.from_hier_file("/nonexistent/scene.hier", "cuda:0", budget_rows=4, rows=rows, slots="f16")


def test_the_switch_is_the_word_that_was_reserved1():
    """Same offset and size as the spare word behind lod_per_pixel; sizeof and the ABI number are unchanged."""
    f = _lib.RasterArgs.lod_half_rows
    assert f.size == 4 and f.offset == _lib.RasterArgs.lod_per_pixel.offset + 4 == 172
    assert _lib.RasterArgs.prepare_backward.offset == f.offset + 4
    assert not hasattr(_lib.RasterArgs, "reserved1")
    assert C.sizeof(_lib.RasterArgs) == 11 * 4 + 4 + 14 * 8 + 2 * 4 + 8 + 2 * 4 + 2 * 8 + 2 * 4 == 208
    assert _lib.RasterArgs.lod_render_indices.offset == 184
    assert _lib.ABI_VERSION == 14 and int(re.search(r"#define\s+HGS_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 14
    assert _lib.RasterArgs().lod_half_rows == 0                                         # (0 is today's behaviour)
    assert C.sizeof(_lib.ResidRowsHalf) == 5 * 8
    assert [n for n, _ in _lib.ResidRowsHalf._fields_] == [n for n, _ in _lib.ResidRows._fields_]


def test_header_declares_the_call_and_documents_the_flag():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bint32_t\s+lod_half_rows\s*;", code) and "reserved1" not in code
    assert re.search(r"\bint\s+hgs_resid_fetch_half_slots\s*\(", code)
    assert re.search(r"typedef\s+struct\s+hgs_resid_rows_half\s*\{(\s*void\s*\*\s*\w+\s*;){5}\s*\}", code)
    order = re.findall(r"void\s*\*\s*(\w+)\s*;", code[code.index("hgs_resid_rows_half"):])[:5]
    assert order == ["means3D", "shs", "opacities", "scales", "rotations"]
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int32_t\s+lod_half_rows", HEADER, flags=re.S).group(1)
    for word in ("lod_render_indices", "IEEE half", "means3D", "prepare_backward", "hgs_raster_bwd", "HGS_ERR_INVALID"):
        assert word in comment, word
    assert "hgs_resid_fetch_half_slots" in _lib.SIGNATURES
    assert _lib.SIGNATURES["hgs_resid_fetch_half_slots"][1][:9] == _lib.SIGNATURES["hgs_resid_fetch_half"][1][:9]


@pytest.mark.parametrize("M", [1, 4, 9, 16])
def test_row_byte_arithmetic(monkeypatch, M):
    """A half slot is 3 M + 8 halves and a float32 mean: 6 M + 28 bytes against 4 (3 M + 11); ``budget_rows`` from
    ``budget_mb`` is counted in it.  ``_setup`` runs up to its first device use."""
    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop

    monkeypatch.setattr(residency, "_host_array", stop)
    monkeypatch.setattr(_lib, "lib", lambda: None)
    seen = {}
    for slots, rows in (("half", "half"), ("float", "half"), ("float", "float")):
        bh = BudgetedHierarchy.__new__(BudgetedHierarchy)
        with pytest.raises(Stop):
            bh._setup(100_000, M, "cpu", 1.0, None, None, rows, slots)
        seen[slots, rows] = (bh.row_bytes, bh.B)
        assert bh.slots_format == slots and bh.rows_format == rows
    half_bytes, float_bytes = 2 * (3 * M + 4 + 3 + 1) + 4 * 3, 4 * (3 * M + 4 + 3 + 1 + 3)
    assert (half_bytes, float_bytes) == (6 * M + 28, 4 * (3 * M + 11))
    assert seen["half", "half"] == (half_bytes, int(1.0 * 1e6 // half_bytes))
    assert seen["float", "half"] == seen["float", "float"] == (float_bytes, int(1.0 * 1e6 // float_bytes))
    if M == 16:
        assert (half_bytes, float_bytes) == (124, 236)
        assert abs(seen["half", "half"][1] / seen["float", "half"][1] - 1.90) < 0.01


def test_half_tensor_uses_other_than_the_one_supported_raise_without_a_gpu():
    """The dtype rules of the rasterizer glue are decided before any tensor is touched: CPU tensors suffice."""
    from diff_gaussian_rasterization import _C as dc
    G, M = 6, 4
    f = dict(means3D=torch.zeros(G, 3), sh=torch.zeros(G, M, 3), opacity=torch.zeros(G, 1), scales=torch.ones(G, 3),
             rotations=torch.zeros(G, 4))
    h = {k: (v if k == "means3D" else v.half()) for k, v in f.items()}
    lod = (torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 0)
    call = lambda t, lod, **kw: dc._half_rows(t["means3D"], t["sh"], kw.get("colors"), t["opacity"], t["scales"],
                                              t["rotations"], kw.get("cov"), kw.get("sh_rest"), kw.get("act", 0), lod)
    assert call(f, lod) is False and call(f, None) is False
    assert call(h, lod) is True
    bad = [(h, None, {}),                                                               # half without render_indices
           (dict(h, sh=f["sh"]), lod, {}), (dict(h, opacity=f["opacity"]), lod, {}),     # a mix of dtypes
           (dict(h, means3D=f["means3D"].half()), lod, {}), (dict(f, scales=h["scales"]), lod, {}),
           (h, lod, dict(sh_rest=torch.zeros(G, 3, 3))), (h, lod, dict(act=3)),           # the raw-parameter path
           (h, lod, dict(colors=torch.zeros(G, 3))), (h, lod, dict(cov=torch.zeros(G, 6)))]
    for t, l, kw in bad:
        with pytest.raises(RuntimeError, match="ONE use: the in-op LOD interpolation"):
            call(t, l, **kw)
