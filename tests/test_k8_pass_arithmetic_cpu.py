"""The pass arithmetic of K8's record staging (k8_sum_runs<true>, csrc/preprocess.hip), no GPU.

A wave brings its contiguous range of 40-byte instance records into its 10 240-byte stage by LDS DMA in 16-byte pieces.
A pass starts at a record, so 8-byte aligned: the DMA starts at the 16-byte boundary at or below it and the sums read
the stage ``shift`` bytes further in.  The rules below restate k8_pass_shift / k8_pass_pieces and the pass loop; the
constants are read from the source, and the extent a caller grants comes from hgs_raster_ws_sizes (the scratch is the
first array of the backward workspace, csrc/abi.cpp BwdWs::layout).  Checked: every pass fits the stage, every record
is read from the bytes it was copied to, and no byte outside [0, size query) is addressed -- for every
``offsets mod 4`` and for ranges that end 0 to 3 records before the end of the scratch."""
import ctypes as C
import os
import re

import pytest

from hgs import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc", "preprocess.hip")).read()
REC = 40                                   # bytes per record (HGS_INST_GRAD_STRIDE floats)
ALIGN = 256
up = lambda x: (x + ALIGN - 1) // ALIGN * ALIGN


def _const(name):
    m = re.search(r"constexpr uint32_t %s = (\d+);" % name, SRC)
    assert m, name
    return int(m.group(1))


STAGE_REC, DMA_REC = _const("kK8StageRec"), _const("kK8DmaRec")
STAGE_BYTES = STAGE_REC * REC


def shift_of(first):                       # k8_pass_shift
    return (first * REC) & 15


def pieces_of(first, cnt):                 # k8_pass_pieces
    return (shift_of(first) + cnt * REC + 15) >> 4


def passes(base, total):
    """(first record, count, DMA source byte, shift, pieces) of every pass over records [base, base + total)."""
    for c0 in range(0, total, DMA_REC):
        cnt = min(DMA_REC, total - c0)
        first = base + c0
        yield first, cnt, first * REC - shift_of(first), shift_of(first), pieces_of(first, cnt)


def _bwd_bytes(L, P=300):
    g, b, i, w = (C.c_size_t() for _ in range(4))
    assert _lib.lib().hgs_raster_ws_sizes(P, 67, 45, L, C.byref(g), C.byref(b), C.byref(i), C.byref(w)) == 0
    return w.value


def test_constants_as_the_source_states_them():
    assert "k8_pass_shift(size_t first) { return (uint32_t)((first * (kInstStride * 4)) & 15u); }" in SRC
    assert "return (k8_pass_shift(first) + cnt * (kInstStride * 4) + 15u) >> 4;" in SRC
    assert STAGE_BYTES == 10240 and DMA_REC % 2 == 0          # an even pass: every pass of a range has the range's shift
    assert pieces_of(1, DMA_REC) <= STAGE_BYTES // 16 < pieces_of(1, DMA_REC + 2)      # the largest even pass that fits


TOTALS = (1, 2, 3, 170, DMA_REC - 1, DMA_REC, DMA_REC + 1, STAGE_REC, 2 * DMA_REC, 2 * DMA_REC + 1, 769)


@pytest.mark.parametrize("base", [0, 1, 2, 3, 4, 5, 6, 7, 1021, 1022, 1023, 1024, 107_374_181, 107_374_182])
def test_every_pass_fits_the_stage_and_reads_its_own_records(base):
    assert {b % 4 for b in (0, 1, 2, 3, 1021, 1022, 1023, 1024)} == {0, 1, 2, 3}
    for total in TOTALS:
        covered = 0
        for first, cnt, src, shift, pieces in passes(base, total):
            assert shift == (8 if first % 2 else 0) and src % 16 == 0 and 0 <= src <= first * REC
            assert 1 <= cnt <= DMA_REC and pieces * 16 <= STAGE_BYTES, (base, total, first, pieces)
            assert shift % 8 == 0                                     # the sums read float2: 8-byte aligned in the stage
            for k in (0, cnt // 2, cnt - 1):                          # record k of the pass: stage bytes -> scratch bytes
                lo = shift + k * REC
                assert lo + REC <= pieces * 16
                assert src + lo == (first + k) * REC
            assert pieces * 16 - (shift + cnt * REC) in (0, 8)        # at most 8 bytes behind the pass's last record
            covered += cnt
        assert covered == total


@pytest.mark.parametrize("short", [0, 1, 2, 3])
@pytest.mark.parametrize("L", [1, 2, 3, 4, 31, 32, 33, 255, 256, 257, 4097, 65_536, 1_000_003])
def test_no_byte_outside_the_size_query(L, short):
    """The wave's range ends ``short`` records before the end of the scratch; its start takes every residue mod 4."""
    granted = _bwd_bytes(L)
    assert granted >= up(L * REC)
    end = L - short
    for total in TOTALS + (end,):
        for back in range(4):
            base = end - total - back
            if base < 0 or total < 1:
                continue
            for first, cnt, src, shift, pieces in passes(base, total + back):
                assert 0 <= src and src + pieces * 16 <= up(L * REC) <= granted, (L, short, base, first, cnt)
