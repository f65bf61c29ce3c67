"""The geometry workspace that hgs_raster_ws_sizes asks for covers everything the per-Gaussian kernel (K1) can store.

K1 works in 64-row waves.  On its cooperative H48 route (M = 16 plain SH, prepare_backward = 1) a wave with any visible
row stores the 36-byte Jacobian rows of all 64 of its Gaussians -- in the last wave also the rows from P up to
ceil64(P).  The layout below restates GeomWs::carve_from (csrc/abi.cpp) and is itself checked against the addresses
hgs_raster_views_get reports; no GPU is needed for either."""
import ctypes as C

from hgs import _lib

ALIGN, REC_BYTES, JAC_BYTES, PRE_BLOCK, BANDS, SCAN_CHUNK = 256, 64, 36, 256, 8, 8 * 1024

up = lambda x: (x + ALIGN - 1) // ALIGN * ALIGN
ceil64 = lambda n: (n + 63) // 64 * 64


def _front(P):
    """Byte offsets of the GeomWs arrays in front of the Jacobians, and the Jacobians' offset."""
    p = max(P, 1)
    nblk = (p + PRE_BLOCK - 1) // PRE_BLOCK
    off, o = {}, 0
    for name, n in (("records", p * REC_BYTES), ("depths", p * 4), ("rects", p * 8), ("tiles_touched", p * 4),
                    ("offsets", p * 4), ("flags", p * 4), ("block_sums", (nblk + 1) * 4),
                    ("block_band", (nblk + 1) * BANDS * 4)):
        off[name] = o
        o += up(n)
    chunks = (nblk + SCAN_CHUNK - 1) // SCAN_CHUNK
    return off, o, (1 + BANDS) * chunks * 8


def _sizes(lib, P, W=67, H=45):
    g, b, i, w = (C.c_size_t() for _ in range(4))
    assert lib.hgs_raster_ws_sizes(P, W, H, 0, C.byref(g), C.byref(b), C.byref(i), C.byref(w)) == 0
    return g.value


PS = list(range(1, 1025)) + [10_440, 16_769, 65_535, 65_537, 300_000, 1_000_003]


def test_every_residue_mod_256_is_covered():
    assert {P % 256 for P in PS} == set(range(256))


def test_layout_restatement_matches_the_library():
    lib = _lib.lib()
    base = 1 << 40                     # never dereferenced: views_get only carves addresses
    for P in (1, 63, 64, 65, 200, 257, 10_440, 16_769, 300_000):
        v = _lib.RasterViews()
        assert lib.hgs_raster_views_get(P, 67, 45, 1, C.c_void_p(base), C.c_void_p(base), C.c_void_p(base),
                                        C.byref(v)) == 0
        off, _, _ = _front(P)
        for name in ("records", "depths", "rects", "tiles_touched", "offsets"):
            assert getattr(v, name) - base == off[name], (P, name)


def test_geom_bytes_cover_whole_wave_stores():
    lib = _lib.lib()
    for P in PS:
        geom = _sizes(lib, P)
        off, jac, chain = _front(P)
        assert off["records"] + ceil64(P) * REC_BYTES <= geom, P
        # the Jacobians of whole waves, then the scan chain K1 clears and the scans publish into: nothing of either may
        # fall outside the workspace, nor may the Jacobian stores reach the chain
        need = jac + up(ceil64(P) * JAC_BYTES) + up(chain)
        assert geom >= need, f"P={P}: geom_bytes {geom} < {need} (whole-wave Jacobian rows + scan chain)"


def test_cut_workspace_sizes_keep_their_closed_forms():
    """hgs_expand_tmp_bytes, hgs_lod_cut_view_tmp_bytes and hgs_lod_cut_budget_tmp_bytes are answered by the code that
    carves the workspaces (csrc/lod_cut.h): no byte formula beside the layout can drift from it.  The closed forms
    below restate the three layouts; the sizes straddle the last partial workgroup of 256 nodes and the first second
    chunk of the scan (8192 workgroup sums)."""
    lib = _lib.lib()
    LEVELS, BINS, STATE = 64 + 2, 2048, 12
    for N in (0, 1, 255, 256, 257, 256 * SCAN_CHUNK - 1, 256 * SCAN_CHUNK, 256 * SCAN_CHUNK + 1, 50_000_000):
        n = max(N, 1)
        nblk = (n + 255) // 256
        chain = up(((nblk + SCAN_CHUNK - 1) // SCAN_CHUNK) * 8)
        expand = 3 * up(n * 4) + up(LEVELS * 4) + up((nblk + 1) * 4) + chain + ALIGN
        view = 3 * up(n * 4) + up(LEVELS * 4) + up((nblk + 2) * 4) + up(nblk * 4) + chain + ALIGN
        budget = 3 * up(n * 4) + up((nblk + 2) * 4) + up(nblk * 4) + chain + up(BINS * 4) + up(STATE * 4) + ALIGN
        assert lib.hgs_expand_tmp_bytes(N) == expand, N
        assert lib.hgs_lod_cut_view_tmp_bytes(N) == view, N
        assert lib.hgs_lod_cut_budget_tmp_bytes(N) == budget, N
