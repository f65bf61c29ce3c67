"""hgs_resid_fetch_half_slots (csrc/residency.hip: resid_fetch_half_slots_kernel) through the C ABI: the fetch that copies
the BITS of a 128-byte half host row into half-precision slot arrays (include/hgs.h: hgs_resid_rows_half).  It follows
tests/test_residency_kernels_gpu.py: the integer state -- which slot a row gets, the stamps, the free stack -- against the
plain slot cache of tests/residency_model.py; the slot contents against the host rows, bit for bit.  Every slot array is
allocated alone between the non-zero guards of tests/ws_guard.py, once filled 0x00 and once 0xFF: a store outside the
array shows in a guard, a store outside the assigned slots shows in the fill -- the last slot of a [B] half array whose
byte length is no multiple of 4 included (B odd).  Nothing here calls the rasterizer."""
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

BUDGETS = [1, 2, 63, 64, 65, 257]
WIDTHS = [1, 4, 16]                       # 6 M = 6, 24, 96 bytes: only M = 16 takes the 16-byte stores


def _halves(M):
    """Halves of the host row (columns of its first 56) that make up each half slot array's row."""
    return dict(shs=np.arange(0, 3 * M), opacities=np.arange(55, 56), scales=np.arange(52, 55), rotations=np.arange(48, 52))


class Pinned:
    """Host rows in pinned, device-mapped memory (hgs_host_alloc)."""

    def __init__(self, rows):
        self.arr, self.ptr = residency._host_array(rows.shape, np.uint8)
        self.arr[:] = rows

    def free(self):
        if self.ptr:
            self.arr = None
            _lib.lib().hgs_host_free(C.c_void_p(self.ptr))
            self.ptr = 0


@pytest.fixture
def pinned(gpu):
    made = []

    def make(rows):
        made.append(Pinned(rows))
        return made[-1]

    yield make
    torch.cuda.synchronize()
    for h in made:
        h.free()


class HalfSlots:
    """The integer buffers of a DeviceCache (test_residency_kernels_gpu.py) and five half slot arrays, every one of them a
    guarded allocation of its own."""

    def __init__(self, gpu, G, B, M, host, cap, fill):
        self.guards, self.fill, self.B, self.M = [], fill, B, M

        def alloc(name, dtype, count):
            g = ws_guard.guarded(count * torch.empty(0, dtype=dtype).element_size(), gpu, fill, name)
            self.guards.append(g)
            return g.view(dtype)

        self.dc = rk.DeviceCache(gpu, G, B, M, host, cap=cap, alloc=alloc)       # (its float slot arrays stay unused)
        self.rows = {"means3D": alloc("half_slot.means3D", torch.float32, B * 3)}
        for k, cols in _halves(M).items():
            self.rows[k] = alloc("half_slot." + k, torch.int16, B * len(cols))
        assert self.rows["opacities"].numel() * 2 == 2 * B and self.rows["scales"].numel() * 2 == 6 * B
        self.slot_rows = _lib.ResidRowsHalf(*[C.c_void_p(self.rows[k].data_ptr()) for k in rm.FIELDS])

    def fetch(self, m, frame, free_top=None, M=None, host_ptr=None, slot_rows=None):
        d, p = self.dc, _lib.ptr
        rc = d.lib.hgs_resid_fetch_half_slots(p(d.miss_ids), m, p(d.free_list), d.free_top if free_top is None else free_top,
                                              p(d.slot_of), p(d.id_of_slot), p(d.stamp), frame,
                                              C.c_void_p(d.host.ptr if host_ptr is None else host_ptr),
                                              C.byref(slot_rows or self.slot_rows), self.M if M is None else M,
                                              rk._stream(), d.dev.index or 0)
        if rc == 0:
            d.free_top -= m
        return rc

    def bytes_of(self):
        """Every slot array as uint8 [B, bytes per slot]."""
        torch.cuda.synchronize()
        return {k: t.view(torch.uint8).cpu().numpy().reshape(self.B, -1) for k, t in self.rows.items()}


def _expected_bytes(rows, M, ids):
    """The bytes the slots of host rows ``ids`` must hold: the host row's own."""
    halves = rows[:, :112].view(np.uint16)
    want = {k: np.ascontiguousarray(halves[ids][:, c]).view(np.uint8) for k, c in _halves(M).items()}
    want["means3D"] = np.ascontiguousarray(rows[ids][:, 112:124])
    return want


def _check(hs, model, rows, what):
    """Integers against the model, every occupied slot's bytes against its host row, every free slot against the fill,
    every guard."""
    d = hs.dc
    torch.cuda.synchronize()
    for k in ("slot_of", "id_of_slot"):
        assert np.array_equal(getattr(d, k).cpu().numpy(), getattr(model, k)), f"{what}: {k}"
    occ = np.nonzero(model.id_of_slot >= 0)[0]
    free = np.nonzero(model.id_of_slot < 0)[0]
    assert np.array_equal(d.stamp.cpu().numpy().view(np.uint32)[occ], model.stamp[occ]), f"{what}: stamp"
    assert (d.stamp.view(torch.uint8).cpu().numpy().reshape(hs.B, 4)[free] == hs.fill).all(), f"{what}: a free slot was stamped"
    assert d.free_top == model.free_top
    got, want = hs.bytes_of(), _expected_bytes(rows, hs.M, model.id_of_slot[occ])
    for k in rm.FIELDS:
        bad = np.argwhere(got[k][occ] != want[k])
        assert bad.size == 0, f"{what}: {k} differs from the host row's bits at (occupied slot, byte) {bad[:6].tolist()}"
        assert (got[k][free] == hs.fill).all(), f"{what}: {k}: a slot that was not fetched was written"
    ws_guard.check(*hs.guards)


@pytest.mark.parametrize("M", WIDTHS)
@pytest.mark.parametrize("B", BUDGETS)
def test_fetch_half_slots_copies_the_bits_into_the_popped_slots(gpu, pinned, B, M):
    """Two fetches fill the budget to its last slot: half of it first (the other slots must keep the fill), then the
    rest (the first half must keep its bits)."""
    G = 2 * B + 11
    rows, wide = hc.half_pattern_rows(G, M)
    useful = rows[:, :112].view(np.uint16)[:, np.r_[0:3 * M, 48:56]]
    assert (useful == 0x8000).any() and (useful == 0x7BFF).any() and ((useful & 0x7FFF) < 0x0400).any()
    host = pinned(rows)
    rng = np.random.default_rng(100 * B + M)
    ids = rng.permutation(np.concatenate([[0, G - 1], 1 + rng.choice(G - 2, B - 2, replace=False)]))[:B] if B > 1 else np.array([G - 1])
    first = max(1, B // 2)
    perm = rng.permutation(B).astype(np.int32)
    for fill in (0x00, 0xFF):
        model = rm.SlotCache(G, B, M, wide)
        model.free_list[:] = perm
        hs = HalfSlots(gpu, G, B, M, host, cap=B, fill=fill)
        hs.dc.free_list.copy_(torch.from_numpy(perm))
        hs.dc.slot_of.fill_(-1)
        hs.dc.id_of_slot.fill_(-1)
        for frame, part in ((0x80000005, ids[:first]), (7, ids[first:])):
            m = len(part)
            if m == 0:
                continue
            hs.dc.miss_ids[:m].copy_(rk._i32(part.astype(np.int32)))
            top = hs.dc.free_top
            _lib.check(hs.fetch(m, frame), "hgs_resid_fetch_half_slots")
            assert model.fetch(part, frame=frame) == rm.OK
            taken = model.slot_of[part]
            assert np.array_equal(taken, perm[top - 1 - np.arange(m)])            # miss j took free_list[free_top - 1 - j]
            _check(hs, model, rows, f"B={B} M={M} fill={fill:#x} frame={frame:#x}")
        rm.check_invariants(hs.dc.slot_of.cpu().numpy(), hs.dc.id_of_slot.cpu().numpy(), perm, hs.dc.free_top, B)
        assert hs.dc.free_top == 0
        assert np.array_equal(host.arr, rows), "the fetch wrote to the host rows"


def test_fetch_half_slots_with_the_sh_array_off_16_bytes_takes_the_narrow_stores(gpu, pinned):
    """M = 16 (16-byte stores possible) with the SH slot array based 2 bytes off a 16-byte boundary: no refusal, the
    same bits, nothing outside the array."""
    G, B, M = 80, 33, 16
    rows, wide = hc.half_pattern_rows(G, M)
    host = pinned(rows)
    hs = HalfSlots(gpu, G, B, M, host, cap=B, fill=0xFF)
    g = ws_guard.guarded(2 + B * 3 * M * 2, gpu, 0xFF, "half_slot.shs.shifted")
    hs.guards.append(g)
    hs.rows["shs"] = g.body[2:].view(torch.int16)
    assert hs.rows["shs"].data_ptr() % 16 == 2
    hs.slot_rows = _lib.ResidRowsHalf(*[C.c_void_p(hs.rows[k].data_ptr()) for k in rm.FIELDS])
    model = rm.SlotCache(G, B, M, wide)
    hs.dc.slot_of.fill_(-1)
    hs.dc.id_of_slot.fill_(-1)
    ids = np.arange(3, 3 + 20)
    hs.dc.miss_ids[:20].copy_(rk._i32(ids.astype(np.int32)))
    _lib.check(hs.fetch(20, 4), "hgs_resid_fetch_half_slots")
    assert model.fetch(ids, frame=4) == rm.OK
    _check(hs, model, rows, "shifted SH array")
    assert (g.body[:2].cpu().numpy() == 0xFF).all()


def test_fetch_half_slots_refuses_what_fetch_half_refuses(gpu, pinned):
    G, B, M = 40, 8, 4
    rows, _ = hc.half_pattern_rows(G, M)
    hs = HalfSlots(gpu, G, B, M, pinned(rows), cap=5, fill=0xFF)
    d = hs.dc
    d.slot_of.fill_(-1)
    d.id_of_slot.fill_(-1)
    d.miss_ids[:2].copy_(torch.tensor([20, 21], dtype=torch.int32))
    d.free_top = 5
    before = hs.bytes_of()
    ints = lambda: [t.cpu().clone() for t in (d.slot_of, d.id_of_slot, d.stamp, d.free_list)]
    ints0 = ints()
    for bad_M in (0, 17):
        assert hs.fetch(2, 2, M=bad_M) == rk.ERR_INVALID and "SH coefficients per channel: 1..16" in rk._last_error()
    assert hs.fetch(2, 2, free_top=1) == _lib.ERR_CAPACITY and "1 free slots for 2 missing rows" in rk._last_error()
    off = _lib.ResidRowsHalf(*[C.c_void_p(hs.rows[k].data_ptr() + (4 if k == "rotations" else 0)) for k in rm.FIELDS])
    assert hs.fetch(2, 2, slot_rows=off) == rk.ERR_INVALID and "aligned" in rk._last_error()
    assert hs.fetch(2, 2, host_ptr=d.host.ptr + 8) == rk.ERR_INVALID and "16-byte aligned" in rk._last_error()
    plain = np.ascontiguousarray(rows)                              # ordinary numpy memory
    assert hs.fetch(2, 2, host_ptr=plain.ctypes.data) == rk.ERR_INVALID and "hgs_host_alloc" in rk._last_error()
    null = _lib.ResidRowsHalf(*[None if k == "scales" else C.c_void_p(hs.rows[k].data_ptr()) for k in rm.FIELDS])
    assert hs.fetch(2, 2, slot_rows=null) == rk.ERR_INVALID and "null" in rk._last_error()
    p = _lib.ptr
    args = [p(d.miss_ids), 2, p(d.free_list), 5, p(d.slot_of), p(d.id_of_slot), p(d.stamp), 2, C.c_void_p(d.host.ptr),
            C.byref(hs.slot_rows), M, rk._stream(), gpu.index or 0]
    for i in (0, 2, 4, 5, 6, 8, 9):
        a = list(args)
        a[i] = None
        assert d.lib.hgs_resid_fetch_half_slots(*a) == rk.ERR_INVALID and "null" in rk._last_error(), i
    assert hs.fetch(0, 2) == 0 and hs.fetch(0, 2, free_top=0, M=0) == 0       # m = 0 returns before any check
    assert d.free_top == 5
    after = hs.bytes_of()
    for k in rm.FIELDS:
        assert np.array_equal(before[k], after[k]), f"{k} was written by a refused call"
    for x, y in zip(ints0, ints()):
        assert torch.equal(x, y)
    ws_guard.check(*hs.guards)
