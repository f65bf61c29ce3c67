"""The host-checkable arithmetic of K6's 4x4 cells (csrc/render.hip, render_fwd_quad_kernel), restated on the CPU: the
cell masks of the staging lanes, the lane <-> pixel map and the bounds of the sixteen lists in LDS."""
import numpy as np

K6_BATCH = 64
CELLS = 16


def _popcount(m):
    return bin(m).count("1")


def test_cell_mask_of_box_bands_and_quadrants():
    """cell_hit: columns x rows of the box as one multiply (four column bits replicated to bits 4 cy), AND the cells of
    the quadrants the exact test keeps.  Against the cell-by-cell definition for every band / quadrant pattern."""
    quad_cells = [0x0033, 0x00CC, 0x3300, 0xCC00]
    for xb in range(16):
        for yb in range(16):
            spread = (yb & 1) | ((yb & 2) << 3) | ((yb & 4) << 6) | ((yb & 8) << 9)
            box = xb * spread
            for q in range(16):
                qm = 0
                for i in range(4):
                    if (q >> i) & 1:
                        qm |= quad_cells[i]
                want = 0
                for c in range(CELLS):
                    cx, cy = c & 3, c >> 2
                    quadrant = (cx >> 1) | ((cy >> 1) << 1)
                    if (xb >> cx) & 1 and (yb >> cy) & 1 and (q >> quadrant) & 1:
                        want |= 1 << c
                assert box & qm == want, (xb, yb, q)


def test_lane_pixel_map_covers_the_tile_once():
    """lane l: cell c = l >> 2, column 4 (c & 3) + (l & 3), rows 4 (c >> 2) + 0..3; every pixel of the 16x16 tile once,
    the four lanes of a quad (one DPP quad) inside one cell, the sixteen lanes of a DPP row in one row of cells."""
    seen = np.zeros((16, 16), int)
    for lane in range(64):
        c = lane >> 2
        x = 4 * (c & 3) + (lane & 3)
        y0 = 4 * (c >> 2)
        assert (lane >> 4) == (c >> 2)
        for s in range(4):
            seen[y0 + s, x] += 1
            assert (x // 4, (y0 + s) // 4) == (c & 3, c >> 2)
    assert (seen == 1).all()


def test_list_entries_and_indices_stay_inside_lds():
    """16-bit entries (record byte offsets up to the dummy instance's, 48- or 64-byte records), 67 rows of 16: the
    front-to-back positions (rank inside the cell's mask) and the look-ahead's reads (three rows past the longest list)
    stay inside the array."""
    for rec_bytes in (48, 64):
        assert K6_BATCH * rec_bytes < 1 << 16
    rows = K6_BATCH + 3
    for cn in range(1, K6_BATCH + 1):
        for rank in range(cn):
            assert 0 <= rank * CELLS + CELLS - 1 < rows * CELLS
        assert (cn - 1 + 3) * CELLS + CELLS - 1 < rows * CELLS
