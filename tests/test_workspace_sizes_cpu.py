"""The geometry workspace that hgs_raster_ws_sizes asks for covers everything the per-Gaussian kernel (K1) can store.

K1 works in 64-row waves.  On its cooperative H48 route (M = 16 plain SH, prepare_backward = 1) a wave with any visible
row stores the 36-byte Jacobian rows of all 64 of its Gaussians -- in the last wave also the rows from P up to
ceil64(P).  The layout below restates GeomWs::layout (csrc/abi.cpp) and is itself checked against the addresses
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
    # the other five fields: the sorted lists and the tile ranges of BinWs (behind four [L] arrays), the two image planes
    for W, H in ((67, 45), (2064, 1536)):
        for L in (1, 4097):
            v = _lib.RasterViews()
            assert lib.hgs_raster_views_get(200, W, H, L, C.c_void_p(base), C.c_void_p(base), C.c_void_p(base),
                                            C.byref(v)) == 0
            want = {"tile_ids_sorted": 2 * up(L * 4), "point_list": 3 * up(L * 4), "ranges": 4 * up(L * 4),
                    "final_T": 0, "n_contrib": up(W * H * 4)}
            want.update({k: o for k, o in _front(200)[0].items() if k in ("records", "depths", "rects", "tiles_touched",
                                                                         "offsets")})
            assert len(want) == len(v._fields_) == 10
            for name, o in want.items():
                assert getattr(v, name) - base == o, (W, H, L, name)


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


def test_cut_views_workspace_size_keeps_its_closed_form():
    """hgs_lod_cut_views_tmp_bytes: V blocks of emission counts, V times the culled sums of one view, the result words."""
    lib = _lib.lib()
    MAX_VIEWS = 16
    for N in (0, 1, 255, 256, 257, 256 * SCAN_CHUNK - 1, 256 * SCAN_CHUNK, 256 * SCAN_CHUNK + 1, 50_000_000):
        n = max(N, 1)
        nblk = (n + 255) // 256
        sums = up((nblk + 2) * 4) + up(nblk * 4) + up(((nblk + SCAN_CHUNK - 1) // SCAN_CHUNK) * 8)
        for V in (1, 2, MAX_VIEWS):
            assert lib.hgs_lod_cut_views_tmp_bytes(N, V) == up(V * n * 4) + V * sums + up(2 * MAX_VIEWS * 4) + ALIGN, (N, V)


# ---- the raster workspaces and the other scratch sizes: closed forms restated from the layouts in csrc/ -----------------
TILE, GROUPS, MAX_BIN_TILES, INST_BYTES, LONG_RUN = 16, 8, 32768, 40, 48
RS_THREADS, RADIX, RS_LARGE = 256, 256, 8 << 20


def _scan_chunks(n):
    return (n + SCAN_CHUNK - 1) // SCAN_CHUNK + (1 if n == 0 else 0)


def _geom(P):
    p = max(P, 1)
    nblk = (p + PRE_BLOCK - 1) // PRE_BLOCK
    return (up(p * REC_BYTES) + up(p * 4) + up(p * 8) + 3 * up(p * 4) + up((nblk + 1) * 4) + up((nblk + 1) * BANDS * 4) +
            up(ceil64(p) * JAC_BYTES) + up((1 + BANDS) * _scan_chunks(nblk) * 8) + ALIGN)


def _sort(n):
    """Sized for 64-bit keys; 4 keys per lane below 8 Mi keys, 16 from there on; one slack block."""
    n = max(n, 1)
    per_block = RS_THREADS * (16 if n >= RS_LARGE else 4)
    return up(n * 8) + up(n * 4) + up(RADIX * ((n + per_block - 1) // per_block) * 4) + up(RADIX * 4) + ALIGN


def _tile_bin(L, T):
    if T > MAX_BIN_TILES:
        return 0
    chunk = 4096 if T <= 12288 else 16384
    chunks = (max(L, 1) + chunk - 1) // chunk
    per = (T + BANDS - 1) // BANDS
    return up(BANDS * chunks * per * 4) + up(GROUPS * per * BANDS * 4) + up((per * BANDS + BANDS * GROUPS) * 4) + ALIGN


def _bin(L, T):
    l = max(L, 1)
    return (4 * up(l * 4) + up(T * 8) + up((3 * T + 3) * 4) + up((T + 8) * 4) + max(_sort(l), _tile_bin(L, T)) + ALIGN)


def _img(W, H):
    return 2 * up(W * H * 4) + ALIGN


def _bwd(L, P):
    """Instance sums, [P,3] colour and mean gradients, the flag / counter block, the long-run worklist, the slack."""
    l, p = max(L, 1), max(P, 1)
    return up(l * INST_BYTES) + 2 * up(p * 12) + ALIGN + up((l // LONG_RUN + 2) * 8) + ALIGN


def _ws(lib, P, W, H, L):
    out = [C.c_size_t() for _ in range(4)]
    assert lib.hgs_raster_ws_sizes(P, W, H, L, *(C.byref(x) for x in out)) == 0
    return dict(zip(("geom", "bin", "img", "bwd"), (x.value for x in out)))


IMAGES = ((2048, 1536), (2064, 1536), (4096, 2048), (4112, 2048))   # T = 12288, 12384, 32768, 32896


def test_image_sizes_straddle_the_binning_switches():
    tiles = [((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE) for W, H in IMAGES]
    assert tiles[0] == 12288 < tiles[1] and tiles[2] == MAX_BIN_TILES < tiles[3]


def test_geom_bytes_keep_their_closed_form():
    lib = _lib.lib()
    for P in [0] + PS:
        assert _ws(lib, P, 67, 45, 0)["geom"] == _geom(P), P


def test_bin_bytes_keep_their_closed_form():
    lib = _lib.lib()
    for W, H in IMAGES:
        T = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)
        for L in (0, 1, 4095, 4096, 4097, 16383, 16384, 16385, 5_000_000):
            assert _ws(lib, 1, W, H, L)["bin"] == _bin(L, T), (W, H, L)


def test_img_bytes_keep_their_closed_form():
    lib = _lib.lib()
    for W, H in IMAGES + ((67, 45),):
        assert _ws(lib, 1, W, H, 0)["img"] == _img(W, H), (W, H)


def test_bwd_bytes_keep_their_closed_form():
    lib = _lib.lib()
    for L in (0, 1, 47, 48, 49, 5_000_000):
        for P in (0, 1, 21, 22, 85, 86):
            assert _ws(lib, P, 67, 45, L)["bwd"] == _bwd(L, P), (L, P)


def test_sort_bytes_keep_their_closed_form():
    lib = _lib.lib()
    for n in (0, 1, 1023, 1024, 1025, 65_535, 65_536, 65_537, RS_LARGE - 1, RS_LARGE, RS_LARGE + 1, RS_LARGE + 4096,
              RS_LARGE + 4097):
        assert lib.hgs_sort_tmp_bytes(n) == _sort(n), n


def test_hierarchy_and_knn_bytes_keep_their_closed_forms():
    """Build, align and knn end in a nested sort scratch of _sort(n) bytes (the sort's own slack included); hier_align
    has no slack of its own, the other two have.  Refit, trim, prune and reach: no slack of their own either."""
    lib = _lib.lib()
    HA_RESULT, MOM_DOUBLES, RUN = (256 + 8) * 4, 10, 256
    for P in (1, 2, 255, 256, 257, 1_048_577):
        N = 2 * P - 1
        assert lib.hgs_hier_build_tmp_bytes(P) == (up(8 * 4) + 3 * up(P * 4) + up(N * 8) + up(N * MOM_DOUBLES * 8) +
                                                   _sort(P) + ALIGN), P
        assert lib.hgs_hier_align_tmp_bytes(P) == up(HA_RESULT) + 3 * up(P * 4) + _sort(P), P
    assert lib.hgs_hier_build_tmp_bytes(0) == 0 and lib.hgs_hier_build_tmp_bytes((1 << 30) + 1) == 0
    assert lib.hgs_hier_align_tmp_bytes(0) == 0 and lib.hgs_hier_align_tmp_bytes(1 << 31) == 0
    # refit, trim, prune and reach, read off their carve functions (none has a slack block of its own): the level lists
    # of hier_levels.h behind the tool's device report, a flag byte per node, prune's two doubles per node, and the
    # workgroup sums of lod_cut.h's carve_sums with their scan chain
    LEVEL_RESULT = (256 + 2) * 4 + 8 + 8 * 4                   # counts, tally, pad; children_sum; minima
    HP_RESULT, HT_RESULT = LEVEL_RESULT + 2 * 4, 4 * 4
    lists = lambda result, N: up(result) + 3 * up(N * 4) + _sort(N)
    sums = lambda nblk, cull: up((nblk + (2 if cull else 1)) * 4) + (up(nblk * 4) if cull else 0) + up(_scan_chunks(nblk) * 8)
    for N in (1, 2, 255, 256, 257, 524_288, 524_289, 50_000_000, (1 << 31) - 1):
        nblk = (N + 255) // 256
        assert lib.hgs_hier_align_tmp_bytes(N) == lists(HA_RESULT, N), N
        assert lib.hgs_hier_refit_tmp_bytes(N) == lists(LEVEL_RESULT, N), N
        assert lib.hgs_hier_trim_tmp_bytes(N) == up(HT_RESULT) + up(N) + sums(nblk, True), N
        assert lib.hgs_hier_prune_tmp_bytes(N) == lists(HP_RESULT, N) + up(N) + 2 * up(N * 8) + sums(nblk, False), N
        for Cn in (1, 255, 256, 257, 1 << 24):
            assert lib.hgs_hier_reach_tmp_bytes(N, Cn) == up(N * 4), (N, Cn)
        assert lib.hgs_hier_reach_tmp_bytes(N, 0) == 0 and lib.hgs_hier_reach_tmp_bytes(N, (1 << 24) + 1) == 0
    for size in (lib.hgs_hier_refit_tmp_bytes, lib.hgs_hier_trim_tmp_bytes, lib.hgs_hier_prune_tmp_bytes):
        assert size(0) == 0 and size(1 << 31) == 0
    assert lib.hgs_hier_reach_tmp_bytes(0, 1) == 0 and lib.hgs_hier_reach_tmp_bytes(1 << 31, 1) == 0
    for P in (0, 1, 255, 256, 257, 2560, 2561, 1_000_003):
        p = max(P, 1)
        assert lib.hgs_knn_tmp_bytes(P) == (up(8 * 4) + 2 * up(p * 8) + 2 * up(p * 4) + up(p * 16) +
                                            up((p + RUN - 1) // RUN * 24) + _sort(p) + ALIGN), P


def test_densify_and_step_bytes_keep_their_closed_forms():
    """Neither has a slack block.  densify: [P] records, four sum arrays of one padded stride; step: a word in a block of
    its own, then a class byte per row."""
    lib = _lib.lib()
    for P in (0, 1, 255, 256, 257, 16_383, 16_384, 1_000_003):
        p = max(P, 1)
        stride = up(((P + 255) // 256 + 1) * 4)
        assert lib.hgs_densify_tmp_bytes(P) == up(p * 8) + 4 * stride, P
        assert lib.hgs_step_tmp_bytes(P) == ALIGN + up(p), P
    for bad in (-1, 1 << 31):
        assert lib.hgs_densify_tmp_bytes(bad) == 0 and lib.hgs_step_tmp_bytes(bad) == 0
