"""hgs_resid_fetch_half and hgs_resid_pack_rows (csrc/residency.hip) through the C ABI, against the numpy specification of
the half host row (hgs.residency.pack_rows_half; include/hgs.h: HGS_RESID_HOST_ROW_BYTES_HALF).  Every comparison is of
integers or of float bits.  Nothing here calls the rasterizer.

Fetch: the half rows of half_rows_cases.half_pattern_rows -- every useful half a function of (id, column) over normal
values of both signs, +-0, subnormals and 65504, NaN in every padding half and in bytes 124..127 -- into slot arrays
that start out as a sentinel between sentinel margins (the DeviceCache of test_residency_kernels_gpu.py), held against
the plain slot cache of tests/residency_model.py fed with the exact widening of the same rows.  A field from the wrong
lane, a padding half that reaches a slot, a store outside the popped slots: each shows in the bits.
Pack: device arrays that hold the tie and saturation cases of the narrowing rule in every field, into pinned rows between
sentinel bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import half_rows_cases as hc
import residency_model as rm
import test_residency_kernels_gpu as rk
import ws_guard
from hgs import _lib, residency

pytestmark = pytest.mark.gpu

G_FETCH = 300
PIN_MARGIN = 256                # sentinel bytes before and after a pinned array (a multiple of 16: keeps the alignment)
PIN_FILL = 0xC3


class Pinned:
    """``nbytes`` of pinned, device-mapped memory (hgs_host_alloc) between two margins of PIN_FILL bytes."""

    def __init__(self, nbytes):
        self.whole, self.base = residency._host_array((PIN_MARGIN + nbytes + PIN_MARGIN,), np.uint8)
        self.whole[:] = PIN_FILL
        self.arr = self.whole[PIN_MARGIN:PIN_MARGIN + nbytes]
        self.ptr = self.base + PIN_MARGIN

    def margins_intact(self):
        return bool((self.whole[:PIN_MARGIN] == PIN_FILL).all() and (self.whole[PIN_MARGIN + self.arr.size:] == PIN_FILL).all())

    def free(self):
        if self.base:
            self.whole = self.arr = None
            _lib.lib().hgs_host_free(C.c_void_p(self.base))
            self.base = self.ptr = 0


@pytest.fixture
def pinned(gpu):
    made = []

    def make(nbytes):
        made.append(Pinned(nbytes))
        return made[-1]

    yield make
    torch.cuda.synchronize()
    for h in made:
        h.free()


def _pinned_rows(pinned, rows):
    h = pinned(rows.size * rows.itemsize)
    h.arr[:] = rows.reshape(-1).view(np.uint8)
    return h


class HalfCache(rk.DeviceCache):
    """The DeviceCache of the float tests with hgs_resid_fetch_half as its fetch (``host``: Pinned half rows)."""

    def fetch(self, m, frame, free_top=None, M=None, host_ptr=None, slot_rows=None):
        p = _lib.ptr
        rc = self.lib.hgs_resid_fetch_half(p(self.miss_ids), m, p(self.free_list), self.free_top if free_top is None else free_top,
                                           p(self.slot_of), p(self.id_of_slot), p(self.stamp), frame,
                                           C.c_void_p(self.host.ptr if host_ptr is None else host_ptr),
                                           C.byref(slot_rows or self.slot_rows), self.M if M is None else M, rk._stream(),
                                           self.dev.index or 0)
        if rc == 0:
            self.free_top -= m
        return rc


# ===================================================================================================================
# fetch
# ===================================================================================================================
FETCH_ROWS = [1, 7, 8, 9, 31, 32, 33]          # one either side of a wave's eight rows and of a workgroup's 32


def _miss_list(rng, G, m):
    if m == 1:
        return np.array([G - 1])
    return rng.permutation(np.concatenate([[0, G - 1], 1 + rng.choice(G - 2, m - 2, replace=False)]))


def _fetch_case(gpu, host, host_wide, wide, M, m, spare, sh_shift):
    """m rows (unsorted, the first and the last host row among them) into a cache of m + spare slots whose free stack
    is a random permutation: every slot array, every integer and the margins against the model; the integers against
    hgs_resid_fetch on the same miss list as well."""
    rng = np.random.default_rng(1000 * M + 10 * m + spare + sh_shift)
    G, B = G_FETCH, m + spare
    model = rm.SlotCache(G, B, M, wide, sentinel=rk.SENTINEL)
    model.free_list[:] = rng.permutation(B).astype(np.int32)
    model.stamp[:] = 77
    miss = _miss_list(rng, G, m)
    frame = 0x80000005
    dc = HalfCache(gpu, G, B, M, host, cap=m, sh_shift=sh_shift)
    fl = rk.DeviceCache(gpu, G, B, M, host_wide, cap=m, sh_shift=sh_shift)
    assert dc.rows["shs"].data_ptr() % 16 == 4 * sh_shift and dc.rows["rotations"].data_ptr() % 16 == 0
    for c in (dc, fl):
        c.upload(model)
        c.miss_ids[:m].copy_(rk._i32(miss.astype(np.int32)))
    _lib.check(dc.fetch(m, frame), "hgs_resid_fetch_half")
    _lib.check(fl.fetch(m, frame), "hgs_resid_fetch")
    assert model.fetch(miss, frame=frame) == rm.OK
    what = f"M={M} m={m} B={B} shift={sh_shift}"
    s = rk.assert_same_state(dc, model, what)                       # (every float's bits, no NaN anywhere, the margins)
    ref = fl.state()
    for k in ("slot_of", "id_of_slot", "stamp"):
        assert np.array_equal(s[k], ref[k]), f"{what}: {k} differs from hgs_resid_fetch"
    rm.check_invariants(s["slot_of"], s["id_of_slot"], s["free_list"], s["free_top"], B)
    assert s["free_top"] == spare
    taken = model.slot_of[miss]
    untouched = np.setdiff1d(np.arange(B), taken)
    for k in rm.FIELDS:
        assert (rk._bits(s[k][untouched]) == rk.SENTINEL.view(np.uint32)).all(), f"{what}: {k}: an unassigned slot was written"
    assert (s["stamp"][untouched] == 77).all()


@pytest.mark.parametrize("M", range(1, 17))
def test_fetch_half_widens_every_field_into_the_popped_slots(gpu, pinned, M):
    """Every SH width, m around a wave's and a workgroup's rows, the budget filled to its last slot and not, the SH slot
    array on and 4 bytes off its 16-byte boundary: both store paths at every M with 3 M % 4 == 0, the scalar path at all."""
    rows, wide = hc.half_pattern_rows(G_FETCH, M)
    useful = rows[:, :112].view(np.uint16)[:, np.r_[0:3 * M, 48:56]]
    e = (useful >> 10) & 31
    assert (e == 0).any() and (e == 30).any() and (useful == 0x7BFF).any() and (useful == 0x8000).any() and (useful == 0).any()
    assert ((useful & 0x7FFF) < 0x0400).any() and (useful >> 15).any() and not (e == 31).any()
    host = _pinned_rows(pinned, rows)
    host_wide = rk.HostRows(wide)
    try:
        for m in FETCH_ROWS:
            for spare in (0, 5):
                for sh_shift in (0, 1):
                    _fetch_case(gpu, host, host_wide, wide, M, m, spare, sh_shift)
        torch.cuda.synchronize()
    finally:
        host_wide.free()
    assert host.margins_intact() and np.array_equal(host.arr, rows.reshape(-1)), "the fetch wrote to the host rows"


@pytest.mark.parametrize("B", [1, 33, 257])
def test_six_frames_through_mark_evict_fetch_half_remap_in_lockstep_with_the_model(gpu, pinned, B):
    G, M, frames = min(2000, 8 * B + 5), {1: 1, 33: 9, 257: 16}[B], 6
    trace = rm.random_trace(G, B, 40, seed=B)
    trace = [t for t in trace if len(rm.needed_rows(*t)) <= B][:frames]          # six frames that fit, evictions among them
    assert len(trace) == frames
    rows, wide = hc.half_pattern_rows(G, M)
    model = rm.SlotCache(G, B, M, wide, sentinel=rk.SENTINEL)
    dc = HalfCache(gpu, G, B, M, _pinned_rows(pinned, rows), cap=max(len(t[0]) for t in trace))
    dc.upload(model)
    fetched = evictions = 0
    for f, (ri, pi, w) in enumerate(trace, start=1):
        need = rm.needed_rows(ri, pi, w)
        dc.set_cut(ri, pi, w)
        rc, count = dc.mark(f)
        _lib.check(rc, "hgs_resid_mark")
        mk = model.mark(ri, pi, w, f)
        assert count == len(mk.miss), f
        miss = dc.out(dc.miss_ids, count)
        assert np.array_equal(np.sort(miss), mk.miss), f
        ro_m, po_m = mk.ro, mk.po
        if count:
            top = dc.free_top
            rc = dc.evict(f, count)
            assert rc == model.evict(f, count) == rm.OK, (f, rc, rk._last_error())
            evictions += dc.free_top > top
            model.adopt_free_order(dc.out(dc.free_list, B), top, model.free_top)
            _lib.check(dc.fetch(count, f), "hgs_resid_fetch_half")
            assert model.fetch(miss, frame=f) == rm.OK
            _lib.check(dc.remap(), "hgs_resid_remap")
            ro_m, po_m = model.remap(ri, pi, w)
            fetched += count
        ro, po = dc.out(dc.ro), dc.out(dc.po)
        assert np.array_equal(ro, ro_m) and np.array_equal(po, po_m), f
        s = rk.assert_same_state(dc, model, f"frame {f}")
        rm.check_invariants(s["slot_of"], s["id_of_slot"], s["free_list"], s["free_top"], B)
        rk.assert_slots_name_the_cut(s["id_of_slot"], ro, po, ri, pi, w)
        assert (s["stamp"][s["slot_of"][need]] == f).all(), f
        rk._assert_contents(s, wide, M, np.nonzero(s["slot_of"] >= 0)[0])       # every resident row: the exact widening
    model.check_invariants()
    assert fetched >= B and evictions >= 1, (fetched, evictions)


def test_fetch_half_refuses_what_fetch_refuses(gpu, pinned):
    G, B, M = 40, 8, 4
    rows, wide = hc.half_pattern_rows(G, M)
    model = rm.SlotCache(G, B, M, wide, sentinel=rk.SENTINEL)
    assert model.fetch([3, 4, 5], frame=1) == rm.OK
    dc = HalfCache(gpu, G, B, M, _pinned_rows(pinned, rows), cap=5)
    dc.upload(model)
    dc.miss_ids[:2].copy_(torch.tensor([20, 21], dtype=torch.int32))
    snap = rk._snapshot(dc)
    for bad_M in (0, 17):
        assert dc.fetch(2, 2, M=bad_M) == rk.ERR_INVALID and "SH coefficients per channel: 1..16" in rk._last_error()
    assert dc.fetch(2, 2, free_top=1) == _lib.ERR_CAPACITY and "1 free slots for 2 missing rows" in rk._last_error()
    rot = torch.full((B * 4 + 4,), float(rk.SENTINEL), device=gpu)
    off = _lib.ResidRows(*[C.c_void_p(rot.data_ptr() + 4 if k == "rotations" else dc.rows[k].data_ptr()) for k in rm.FIELDS])
    assert dc.fetch(2, 2, slot_rows=off) == rk.ERR_INVALID and "16-byte aligned" in rk._last_error()
    assert dc.fetch(2, 2, host_ptr=dc.host.ptr + 8) == rk.ERR_INVALID and "16-byte aligned" in rk._last_error()
    plain = np.ascontiguousarray(rows)                              # ordinary numpy memory
    assert dc.fetch(2, 2, host_ptr=plain.ctypes.data) == rk.ERR_INVALID and "hgs_host_alloc" in rk._last_error()
    assert dc.fetch(0, 2) == 0 and dc.fetch(0, 2, free_top=0, M=0) == 0
    assert dc.free_top == 5
    rk._assert_untouched(dc, snap)
    assert (rot.cpu().numpy().view(np.uint32) == rk.SENTINEL.view(np.uint32)).all()


# ===================================================================================================================
# pack
# ===================================================================================================================
def _float_rows(means3D, shs, opac, scales, rots):
    """The float host rows as BudgetedHierarchy.__init__ writes them (include/hgs.h: HGS_RESID_HOST_ROW_FLOATS)."""
    G, M = shs.shape[0], shs.shape[1]
    rows = np.zeros((G, 64), np.float32)
    rows[:, :3 * M] = shs.reshape(G, 3 * M)
    rows[:, 48:52], rows[:, 52:55], rows[:, 55:58], rows[:, 58] = rots, means3D, scales, opac.reshape(G)
    return rows


def _expected_rows(arrays, half):
    return residency.pack_rows_half(*arrays) if half else _float_rows(*arrays).view(np.uint8)


def _pack(gpu, tensors, G, M, half, host_ptr, stream=None):
    src = _lib.ResidRows(*[C.c_void_p(t.data_ptr()) for t in tensors])
    st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    return _lib.lib().hgs_resid_pack_rows(C.byref(src), G, M, int(half), C.c_void_p(host_ptr), st, gpu.index or 0)


@pytest.mark.parametrize("half", [True, False], ids=["half", "float"])
@pytest.mark.parametrize("M", [1, 4, 5, 16])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 1000])
def test_pack_rows_writes_the_specified_bytes(gpu, pinned, G, M, half):
    arrays = hc.attribute_arrays(G, M, seed=G + M)
    if G >= 63:
        for a in arrays:                                            # every case of the narrowing rule, NaN too, in every field
            assert np.isin(hc.NARROW_VALUES.view(np.uint32), a.view(np.uint32)).all()
    want = _expected_rows(arrays, half)
    tensors = [torch.from_numpy(a).to(gpu) for a in arrays]
    outs = [pinned(want.size) for _ in range(2)]
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    _lib.check(_pack(gpu, tensors, G, M, half, outs[0].ptr), "hgs_resid_pack_rows")
    _lib.check(_pack(gpu, tensors, G, M, half, outs[1].ptr, side), "hgs_resid_pack_rows")
    torch.cuda.synchronize()
    for o in outs:
        got = o.arr.reshape(want.shape)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"(row, byte) {bad[:8].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
        assert o.margins_intact(), "a store outside the pinned rows"
    if half:
        halves = want[:, :112].view(np.uint16)
        fin = [np.isfinite(a).reshape(G, -1) for a in arrays]
        src_finite = np.concatenate([fin[1], np.ones((G, 48 - 3 * M), bool), fin[4], fin[3], fin[2]], axis=1)
        assert ((halves & 0x7FFF) <= 0x7BFF)[src_finite].all(), "a finite value became an infinity or a NaN"


def test_pack_rows_refuses_unpinned_and_misaligned_rows(gpu, pinned):
    G, M = 10, 2
    tensors = [torch.from_numpy(a).to(gpu) for a in hc.attribute_arrays(G, M, seed=1)]
    out = pinned(G * 256)
    before = out.whole.copy()
    plain = np.zeros(G * 256, np.uint8)
    assert _pack(gpu, tensors, G, M, True, plain.ctypes.data) == rk.ERR_INVALID and "hgs_host_alloc" in rk._last_error()
    assert _pack(gpu, tensors, G, M, False, out.ptr + 4) == rk.ERR_INVALID and "16-byte aligned" in rk._last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out.whole, before) and not plain.any()


# ===================================================================================================================
# guard bytes
# ===================================================================================================================
@pytest.mark.parametrize("M", [1, 9, 16])
@pytest.mark.parametrize("m,B", [(1, 1), (33, 33), (257, 262)])
def test_both_calls_stay_inside_guarded_device_buffers(gpu, pinned, M, m, B):
    """Every device buffer of hgs_resid_fetch_half and of hgs_resid_pack_rows between the guards of tests/ws_guard.py,
    once filled 0x00 and once 0xFF: the guards stay intact and the results do not depend on the fill."""
    G = m + 12
    rows, wide = hc.half_pattern_rows(G, M)
    host = _pinned_rows(pinned, rows)
    rng = np.random.default_rng(m + M)
    miss, perm = _miss_list(rng, G, m), rng.permutation(B).astype(np.int32)
    arrays = hc.attribute_arrays(G, M, seed=m)
    results = []
    for fill in (0x00, 0xFF):
        gs = []

        def alloc(name, dtype, count):
            g = ws_guard.guarded(count * torch.empty(0, dtype=dtype).element_size(), gpu, fill, name)
            gs.append(g)
            return g.view(dtype)

        dc = HalfCache(gpu, G, B, M, host, cap=m, alloc=alloc)
        dc.free_list.copy_(torch.from_numpy(perm))
        dc.miss_ids[:m].copy_(rk._i32(miss.astype(np.int32)))
        _lib.check(dc.fetch(m, 3), "hgs_resid_fetch_half")
        ws_guard.check(*gs)
        s = dc.state()
        slots = perm[B - 1 - np.arange(m)]                          # miss j took free_list[free_top - 1 - j]
        assert np.array_equal(s["slot_of"][miss], slots) and np.array_equal(s["id_of_slot"][slots], miss)
        assert (s["stamp"][slots] == 3).all()
        rk._assert_contents(s, wide, M, miss)
        # pack: the five inputs in guarded buffers
        ins = []
        for k, a in zip(rm.FIELDS, arrays):
            g = ws_guard.guarded(a.nbytes, gpu, fill, "pack." + k)
            g.view(torch.float32).copy_(torch.from_numpy(a.reshape(-1)))
            gs.append(g)
            ins.append(g.view(torch.float32))
        out = pinned(G * 128)
        _lib.check(_pack(gpu, ins, G, M, True, out.ptr), "hgs_resid_pack_rows")
        ws_guard.check(*gs)
        assert np.array_equal(out.arr.reshape(G, 128), residency.pack_rows_half(*arrays)) and out.margins_intact()
        results.append({k: s[k][slots].copy() for k in rm.FIELDS})
    for k in rm.FIELDS:
        assert np.array_equal(rk._bits(results[0][k]), rk._bits(results[1][k])), k
