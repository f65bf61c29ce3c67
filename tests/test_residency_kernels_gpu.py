"""The four residency calls of the C ABI -- hgs_resid_mark / _evict / _fetch / _remap (csrc/residency.hip) -- held
against the plain slot cache of tests/residency_model.py at tiny sizes: budgets of 1 .. 257 rows, where every frame
evicts, and every SH width, so that both store paths of the fetch kernel run.  Every comparison is of integers or of
float bits.  Nothing here calls the rasterizer.

The host rows hold id * 64 + col at (id, col) and NaN in their padding columns, the slot arrays start out as a sentinel
with a sentinel margin on either side: a field taken from the wrong lane, component or row, a padding column that
reaches a slot, a store outside the assigned slots -- each shows in the bits.  Where the header leaves an order open
(miss list, free stack) the SET is compared, then the model follows the device's order and the two stay in lockstep."""
import ctypes as C

import numpy as np
import pytest
import torch

import residency_model as rm
from hgs import _lib

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.0)
MARGIN = 64                     # floats of sentinel before and after every slot array (a multiple of 4: keeps alignment)
INT_FILL = -7                   # what miss_ids / ro / po hold before a call
ERR_INVALID = 1


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _last_error():
    msg = _lib.lib().hgs_last_error()
    return msg.decode() if msg else ""


class HostRows:
    """Packed rows in pinned, device-mapped memory (hgs_host_alloc)."""

    def __init__(self, rows):
        from hgs.residency import _host_array
        self.arr, self.ptr = _host_array(rows.shape)
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
        made.append(HostRows(rows))
        return made[-1]

    yield make
    torch.cuda.synchronize()
    for h in made:
        h.free()


def _i32(a):
    """numpy int32 / uint32 -> int32 CPU tensor (bits kept)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


class DeviceCache:
    """Device state of one budgeted hierarchy and the four C calls on it, with the caller's part of the protocol (the
    free-stack top lives on the host; fetch pops it).  ``alloc(name, dtype, count)`` supplies every buffer (the
    workspace-bounds test passes guarded allocations); by default plain tensors, the slot arrays between sentinel
    margins.  ``sh_shift``: floats by which the SH slot array is moved off its 16-byte boundary."""

    def __init__(self, dev, G, B, M, host=None, cap=1, alloc=None, sh_shift=0):
        self.dev, self.G, self.B, self.M, self.host, self.cap = dev, G, B, M, host, cap
        self.lib = _lib.lib()
        self._raw = {}
        plain = alloc is None
        alloc = alloc or (lambda name, dtype, count: torch.empty(count, dtype=dtype, device=dev))
        i32 = torch.int32
        self.slot_of = alloc("slot_of", i32, G)
        self.stamp = alloc("stamp", i32, B)                      # (the header leaves it to the calls: not initialised)
        self.id_of_slot = alloc("id_of_slot", i32, B)
        self.free_list = alloc("free_list", i32, B)
        self.counters = alloc("counters", i32, _lib.RESID_COUNTER_WORDS)
        self.miss_ids = alloc("miss_ids", i32, 2 * cap)
        self.ri, self.pi = alloc("render_indices", i32, cap), alloc("parent_indices", i32, cap)
        self.w = alloc("weights", torch.float32, cap)
        self.ro, self.po = alloc("ro", i32, cap), alloc("po", i32, cap)
        self.slot_of.fill_(-1)
        self.id_of_slot.fill_(-1)
        self.free_list.copy_(torch.arange(B - 1, -1, -1, dtype=i32))
        self.free_top = B
        self.rows = {}
        for k, cols in rm.field_columns(M).items():
            width = len(cols)
            if plain:
                raw = torch.full((MARGIN + B * width + MARGIN,), float(SENTINEL), dtype=torch.float32, device=dev)
                off = MARGIN + (sh_shift if k == "shs" else 0)
                self._raw[k] = (raw, off)
                self.rows[k] = raw[off:off + B * width].view(B, width)
            else:
                self.rows[k] = alloc("slot." + k, torch.float32, B * width).view(B, width)
        self.slot_rows = _lib.ResidRows(*[C.c_void_p(self.rows[k].data_ptr()) for k in rm.FIELDS])
        self.n, self.has_w = 0, False

    # -- state ----------------------------------------------------------------------------------------------------
    def upload(self, model):
        self.slot_of.copy_(_i32(model.slot_of))
        self.id_of_slot.copy_(_i32(model.id_of_slot))
        self.stamp.copy_(_i32(model.stamp))
        self.free_list.copy_(_i32(model.free_list))
        self.free_top = model.free_top
        for k in rm.FIELDS:
            self.rows[k].copy_(torch.from_numpy(model.rows[k]))

    def state(self):
        torch.cuda.synchronize()
        s = dict(slot_of=self.slot_of.cpu().numpy(), id_of_slot=self.id_of_slot.cpu().numpy(),
                 stamp=self.stamp.cpu().numpy().view(np.uint32), free_list=self.free_list.cpu().numpy(),
                 free_top=self.free_top)
        for k in rm.FIELDS:
            s[k] = self.rows[k].cpu().numpy()
        return s

    def margins_intact(self):
        torch.cuda.synchronize()
        for k, (raw, off) in self._raw.items():
            n = self.rows[k].numel()
            edge = torch.cat([raw[:off], raw[off + n:]]).cpu().numpy()
            assert (edge.view(np.uint32) == SENTINEL.view(np.uint32)).all(), f"{k}: a store outside the slot array"

    def set_cut(self, ri, pi, w, prefill=True):
        n = len(ri)
        assert n <= self.cap
        self.n, self.has_w = n, w is not None
        self.ri[:n].copy_(_i32(np.asarray(ri, np.int32)))
        self.pi[:n].copy_(_i32(np.asarray(pi, np.int32)))
        if w is not None:
            self.w[:n].copy_(torch.from_numpy(np.asarray(w, np.float32)))
        if prefill:
            for t in (self.miss_ids, self.ro, self.po):
                t.fill_(INT_FILL)

    def _w(self):
        return _lib.ptr(self.w) if self.has_w else None

    # -- the four calls -------------------------------------------------------------------------------------------
    def mark(self, frame):
        p, miss = _lib.ptr, C.c_uint32(0xDEAD)
        rc = self.lib.hgs_resid_mark(p(self.ri), p(self.pi), self._w(), self.n, self.G, p(self.slot_of), p(self.stamp),
                                     frame, p(self.miss_ids), p(self.counters), p(self.ro), p(self.po), C.byref(miss),
                                     _stream(), self.dev.index or 0)
        return rc, int(miss.value)

    def evict(self, frame, need):
        p, top = _lib.ptr, C.c_uint32(self.free_top)
        rc = self.lib.hgs_resid_evict(p(self.stamp), p(self.id_of_slot), p(self.slot_of), self.B, frame, need,
                                      p(self.free_list), p(self.counters), C.byref(top), _stream(), self.dev.index or 0)
        if rc != 0:
            assert top.value == self.free_top, "a refused eviction changed the free-stack top"
        self.free_top = int(top.value)
        return rc

    def fetch(self, m, frame, free_top=None, M=None, host_ptr=None, slot_rows=None):
        p = _lib.ptr
        rc = self.lib.hgs_resid_fetch(p(self.miss_ids), m, p(self.free_list), self.free_top if free_top is None else free_top,
                                      p(self.slot_of), p(self.id_of_slot), p(self.stamp), frame,
                                      C.c_void_p(self.host.ptr if host_ptr is None else host_ptr),
                                      C.byref(slot_rows or self.slot_rows), self.M if M is None else M, _stream(),
                                      self.dev.index or 0)
        if rc == 0:
            self.free_top -= m
        return rc

    def remap(self):
        p = _lib.ptr
        return self.lib.hgs_resid_remap(p(self.ri), p(self.pi), self._w(), self.n, p(self.slot_of), p(self.ro), p(self.po),
                                        _stream(), self.dev.index or 0)

    def unqueue(self, count):
        """The caller's part after a refused frame (hgs/residency.py: make_resident.unqueue)."""
        ids = self.miss_ids[:count].long()
        cur = self.slot_of[ids]
        self.slot_of[ids] = torch.where(cur == -2, torch.full_like(cur, -1), cur)

    def out(self, t, n=None):
        torch.cuda.synchronize()
        return t[:self.n if n is None else n].cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_state(dc, model, what="", free_from=0):
    """Every array of the device's state equals the model's: integers, stamps, the live part of the free stack (from
    ``free_from`` on, for a caller that did not follow the device's order below it) and every float of every slot."""
    s = dc.state()
    for k in ("slot_of", "id_of_slot", "stamp"):
        bad = np.nonzero(s[k] != getattr(model, k))[0]
        assert bad.size == 0, f"{what}: {k} differs at {bad[:8]}: {s[k][bad[:8]]} != {getattr(model, k)[bad[:8]]}"
    assert s["free_top"] == model.free_top, (what, s["free_top"], model.free_top)
    assert np.array_equal(s["free_list"][free_from:model.free_top], model.free_list[free_from:model.free_top]), what
    for k in rm.FIELDS:
        got, want = _bits(s[k]), _bits(model.rows[k])
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}: slot array {k} differs at (slot, float) {bad[:6].tolist()}: " \
                              f"{s[k][tuple(bad[0])]} != {model.rows[k][tuple(bad[0])]}"
        assert not np.isnan(s[k]).any(), f"{what}: a padding column of the host row reached {k}"
    dc.margins_intact()
    return s


def _cut_arrays(ri, pi, w):
    par = np.ones(len(ri), bool) if w is None else ~(np.asarray(w, np.float32) == np.float32(1.0))
    return np.asarray(ri, np.int64), np.asarray(pi, np.int64), par


def assert_slots_name_the_cut(id_of_slot, ro, po, ri, pi, w):
    ri, pi, par = _cut_arrays(ri, pi, w)
    assert (ro >= 0).all() and (po >= 0).all()
    assert np.array_equal(id_of_slot[ro], ri), "id_of_slot[ro[i]] != ri[i]"
    assert np.array_equal(id_of_slot[po[par]], pi[par]), "id_of_slot[po[i]] != pi[i] where the parent is needed"
    assert np.array_equal(po[~par], ro[~par]), "po != ro where the weight is exactly 1"


# ===================================================================================================================
# fetch
# ===================================================================================================================
FETCH_M = [1, 2, 4, 9, 16]                    # 3 M = 3, 6, 12, 27, 48: M = 4 and 16 take the float4 path, the others the scalar one
FETCH_ROWS = [1, 15, 16, 17, 255, 257]        # sixteen rows per workgroup


def _fetch_case(gpu, pinned, M, m, spare, sh_shift=0):
    """m rows into a cache of m + spare slots whose free stack is a random permutation; G > B; the miss list is
    unsorted and holds the first and the last host row."""
    rng = np.random.default_rng(1000 * M + m + spare)
    B, G = m + spare, 2 * m + 11
    host_np = rm.pattern_rows(G, M)
    host = pinned(host_np)
    model = rm.SlotCache(G, B, M, host_np, sentinel=SENTINEL)
    model.free_list[:] = rng.permutation(B).astype(np.int32)
    model.stamp[:] = 77
    if m == 1:
        miss = np.array([G - 1])
    else:
        miss = rng.permutation(np.concatenate([[0, G - 1], 1 + rng.choice(G - 2, m - 2, replace=False)]))
    assert len(np.unique(miss)) == m
    dc = DeviceCache(gpu, G, B, M, host, cap=m, sh_shift=sh_shift)
    assert dc.rows["shs"].data_ptr() % 16 == 4 * sh_shift and dc.rows["rotations"].data_ptr() % 16 == 0
    dc.upload(model)
    dc.miss_ids[:m].copy_(_i32(miss.astype(np.int32)))
    frame = 0x80000005                                            # (a frame number above 2^31: stamps are unsigned)
    _lib.check(dc.fetch(m, frame), "hgs_resid_fetch")
    assert model.fetch(miss, frame=frame) == rm.OK
    s = assert_same_state(dc, model, f"M={M} m={m} free_top={B}")
    rm.check_invariants(s["slot_of"], s["id_of_slot"], s["free_list"], s["free_top"], B)
    model.check_invariants()                                      # (slot contents against the host rows, field by field)
    assert s["free_top"] == spare
    taken = model.slot_of[miss]
    assert np.array_equal(taken, model.free_list[B - 1 - np.arange(m)])          # miss j took free_list[free_top - 1 - j]
    untouched = np.setdiff1d(np.arange(B), taken)
    for k in rm.FIELDS:
        assert (_bits(s[k][untouched]) == SENTINEL.view(np.uint32)).all(), f"{k}: an unassigned slot was written"
    assert (s["stamp"][untouched] == 77).all()


@pytest.mark.parametrize("m", FETCH_ROWS)
@pytest.mark.parametrize("M", FETCH_M)
def test_fetch_copies_every_field_of_the_packed_row(gpu, pinned, M, m):
    """Both template instantiations of the fetch kernel: resid_fetch_kernel<true> at M = 4, 16 and
    resid_fetch_kernel<false> at M = 1, 2, 9; with free_top == m (the budget filled to its last slot) and free_top > m."""
    _fetch_case(gpu, pinned, M, m, spare=0)
    _fetch_case(gpu, pinned, M, m, spare=5)


@pytest.mark.parametrize("m", [1, 17, 257])
def test_fetch_with_sh_array_off_16_bytes_takes_the_scalar_path(gpu, pinned, m):
    """M = 4 (3 M = 12 floats: float4 stores possible) with the SH slot array based 4 bytes off a 16-byte boundary: no
    refusal, the same bits."""
    _fetch_case(gpu, pinned, 4, m, spare=0, sh_shift=1)
    _fetch_case(gpu, pinned, 4, m, spare=3, sh_shift=1)


# ===================================================================================================================
# mark and remap
# ===================================================================================================================
MARK_N = [1, 63, 64, 65, 257, 1000]


def _mark_case(n, weights, seed):
    """A cut of n entries over a small pool (heavy duplication within ri, within pi and across both), half of the pool
    resident; with weights: shares exactly 1, one NaN, and three parents that no other entry names -- X, absent, under a
    weight of 1 (must stay absent), Y under the NaN (must be queued), and a resident one under a weight of 1 (must keep
    its old stamp)."""
    rng = np.random.default_rng(seed)
    G = 1200
    ids = rng.permutation(G)
    pool = ids[:max(2, n // 3)]
    X, Y = int(ids[-1]), int(ids[-2])
    bystanders = ids[-12:-2]                                      # resident, not in the cut: their stamps must not move
    resident = np.concatenate([pool[::2], bystanders])
    ri, pi = rng.choice(pool, n), rng.choice(pool, n)
    if n >= 4:
        ri[1], pi[2] = ri[0], ri[0]                               # the same id twice in ri, and in pi as well
    w = None
    if weights:
        w = rng.choice(np.array([1.0, 0.0, 0.5, 0.999999], np.float32), n).astype(np.float32)
        w[0], pi[0] = 1.0, X
        if n >= 2:
            w[1], pi[1] = np.nan, Y
        if n >= 4:
            w[3], pi[3] = 1.0, bystanders[0]                      # a RESIDENT parent under a weight of 1: not stamped
    B = len(pool) + len(bystanders) + 4
    return G, B, resident, ri.astype(np.int32), pi.astype(np.int32), w, X, Y


@pytest.mark.parametrize("weights", [False, True], ids=["no_weights", "weights_1_and_nan"])
@pytest.mark.parametrize("n", MARK_N)
def test_mark_fetch_remap_against_the_model(gpu, pinned, n, weights):
    M = 9 if n % 2 else 16
    G, B, resident, ri, pi, w, X, Y = _mark_case(n, weights, seed=n + 7 * weights)
    host_np = rm.pattern_rows(G, M)
    model = rm.SlotCache(G, B, M, host_np, sentinel=SENTINEL)
    assert model.fetch(resident, frame=5) == rm.OK
    dc = DeviceCache(gpu, G, B, M, pinned(host_np), cap=n)
    dc.upload(model)
    dc.set_cut(ri, pi, w)
    rc, count = dc.mark(9)
    _lib.check(rc, "hgs_resid_mark")
    mk = model.mark(ri, pi, w, 9)
    assert not mk.error
    if n >= 63:
        assert len(mk.miss) > 0 and (mk.ro >= 0).any() and (mk.ro == -2).any()       # a mix of resident and absent rows
    if weights:
        assert X not in mk.miss and model.slot_of[X] == -1
        assert n < 2 or Y in mk.miss
    assert count == len(mk.miss)
    miss_buf = dc.out(dc.miss_ids, 2 * n)
    miss = miss_buf[:count]
    assert np.array_equal(np.sort(miss), mk.miss), "the miss list is not the model's set, each id once"
    assert (miss_buf[count:] == INT_FILL).all(), "the miss list was written past its count"
    assert np.array_equal(dc.out(dc.ro), mk.ro) and np.array_equal(dc.out(dc.po), mk.po)
    s = assert_same_state(dc, model, "after mark")                # (slot_of with its -2 entries, the stamps)
    hit = np.intersect1d(rm.needed_rows(ri, pi, w), resident)
    assert (s["stamp"][model.slot_of[hit]] == 9).all()
    rest = np.setdiff1d(resident, hit)
    assert len(rest) >= 10 and (s["stamp"][model.slot_of[rest]] == 5).all()
    # fetch in the device's miss order, then remap
    _lib.check(dc.fetch(count, 9), "hgs_resid_fetch")
    assert model.fetch(miss, frame=9) == rm.OK
    _lib.check(dc.remap(), "hgs_resid_remap")
    ro_m, po_m = model.remap(ri, pi, w)
    ro, po = dc.out(dc.ro), dc.out(dc.po)
    assert np.array_equal(ro, ro_m) and np.array_equal(po, po_m)
    s = assert_same_state(dc, model, "after fetch and remap")
    rm.check_invariants(s["slot_of"], s["id_of_slot"], s["free_list"], s["free_top"], B)
    model.check_invariants()
    assert_slots_name_the_cut(s["id_of_slot"], ro, po, ri, pi, w)
    if weights:
        assert s["slot_of"][X] == -1                              # the parent under a weight of 1 was never fetched


def test_mark_reports_a_bad_index_and_the_valid_rows_it_queued(gpu, pinned):
    n, G, B, M = 65, 300, 200, 2
    rng = np.random.default_rng(3)
    host_np = rm.pattern_rows(G, M)
    model = rm.SlotCache(G, B, M, host_np, sentinel=SENTINEL)
    assert model.fetch(np.arange(0, 40, 2), frame=1) == rm.OK
    ri = rng.integers(0, 60, n).astype(np.int32)
    pi = rng.integers(0, 60, n).astype(np.int32)
    w = rng.choice(np.array([1.0, 0.5], np.float32), n)
    ri[7], ri[64] = G, -1
    pi[20], pi[33] = G + 5, -2 ** 31
    w[33] = 1.0                                                    # a bad parent under a weight of 1 is still reported
    dc = DeviceCache(gpu, G, B, M, pinned(host_np), cap=n)
    dc.upload(model)
    dc.set_cut(ri, pi, w)
    rc, count = dc.mark(2)
    assert rc == ERR_INVALID and "outside [0, 300)" in _last_error()
    mk = model.mark(ri, pi, w, 2)
    assert mk.error and count == len(mk.miss) > 0                  # the valid rows of the call were queued and are reported
    miss = dc.out(dc.miss_ids, count)
    assert np.array_equal(np.sort(miss), mk.miss)
    ro, po = dc.out(dc.ro), dc.out(dc.po)
    assert np.array_equal(ro, mk.ro) and np.array_equal(po, mk.po)
    assert ro[7] == -1 and ro[64] == -1 and po[20] == -1 and po[33] == -1
    assert_same_state(dc, model, "after the refused mark")
    dc.unqueue(count)
    model.unqueue(mk.miss)
    s = assert_same_state(dc, model, "after the caller's un-queue")
    rm.check_invariants(s["slot_of"], s["id_of_slot"], s["free_list"], s["free_top"], B)
    assert np.array_equal(np.nonzero(s["slot_of"] >= 0)[0], np.arange(0, 40, 2))


# ===================================================================================================================
# evict
# ===================================================================================================================
def _hand_state(B, ages, frame, seed=0):
    """A cache whose slot s is free (ages[s] is None) or holds a row last used ages[s] frames before ``frame``."""
    rng = np.random.default_rng(seed)
    G = B + 3
    model = rm.SlotCache(G, B, 1, sentinel=SENTINEL)
    occ = np.array([a is not None for a in ages])
    ids = rng.permutation(G)[:B].astype(np.int32)
    model.id_of_slot[:] = np.where(occ, ids, -1)
    model.slot_of[ids[occ]] = np.nonzero(occ)[0]
    model.stamp[:] = [(frame - (a or 0)) % (1 << 32) for a in ages]
    free = rng.permutation(np.nonzero(~occ)[0]).astype(np.int32)
    model.free_list[:] = -9
    model.free_list[:len(free)] = free
    model.free_top = len(free)
    model.check_invariants()
    return model


def _evict_both(gpu, model, frame, need, expect):
    """The same eviction on the device and on the model: status, freed set, top, every buffer."""
    before = model.copy()
    dc = DeviceCache(gpu, model.G, model.B, model.M)
    dc.upload(model)
    rc = dc.evict(frame, need)
    assert model.evict(frame, need) == expect
    assert rc == expect, (rc, _last_error())
    assert dc.free_top == model.free_top
    model.adopt_free_order(dc.out(dc.free_list, model.B), before.free_top, model.free_top)     # the same SET of slots
    s = assert_same_state(dc, model, f"evict(frame={frame}, need={need})")
    assert np.array_equal(s["free_list"], model.free_list)        # (the dead part of the stack too)
    freed = s["free_list"][before.free_top:s["free_top"]]
    assert (before.ages(frame)[freed] >= 1).all() and (before.id_of_slot[freed] >= 0).all()
    assert np.array_equal(s["stamp"], before.stamp)
    if expect != rm.OK or before.free_top >= need:
        for k in ("slot_of", "id_of_slot", "free_list"):
            assert np.array_equal(s[k], getattr(before, k)), k
        assert s["free_top"] == before.free_top
    else:
        assert s["free_top"] >= need
        rm.check_invariants(s["slot_of"], s["id_of_slot"], s["free_list"], s["free_top"], model.B)
    return s, freed


def test_evict_saturated_ages_go_together(gpu):
    """Stamps 70 and 200 frames old are both age 63: one slot is asked for, both go, the row of age 1 stays."""
    frame = 1000
    model = _hand_state(6, [70, 200, 1, 0, 63, 62], frame)
    s, freed = _evict_both(gpu, model, frame, 1, rm.OK)
    assert sorted(freed) == [0, 1, 4] and s["free_top"] == 3


def test_evict_takes_frame_minus_stamp_unsigned(gpu):
    """A stamp of 0xFFFFFFFE seen at frame 1 is age 3."""
    model = _hand_state(4, [3, 2, 5, 0], 1)
    assert model.stamp[0] == 0xFFFFFFFE and model.stamp[2] == 0xFFFFFFFC
    s, freed = _evict_both(gpu, model, 1, 2, rm.OK)
    assert sorted(freed) == [0, 2]                                 # ages 5 and 3; age 2 stays


def test_evict_reaches_need_only_with_age_one_and_frees_all_of_that_age(gpu):
    frame = 50
    ages = [0, 1, 1, 1, 1, 0, 2, None, 1, 0]
    model = _hand_state(len(ages), ages, frame)
    s, freed = _evict_both(gpu, model, frame, 4, rm.OK)            # one free + age 2 + two of age 1 would do: all of age 1 go
    assert sorted(freed) == [1, 2, 3, 4, 6, 8] and s["free_top"] == 7


def test_evict_refuses_a_need_it_cannot_reach_and_changes_nothing(gpu):
    frame = 50
    ages = [0, 1, 1, 0, 0, None, 7, 0]
    model = _hand_state(len(ages), ages, frame)
    _evict_both(gpu, model, frame, 5, rm.ERR_CAPACITY)             # one free + three older rows: four at the most
    assert "budget of 8 rows" in _last_error()
    _evict_both(gpu, _hand_state(len(ages), ages, frame), frame, 4, rm.OK)
    _evict_both(gpu, _hand_state(len(ages), ages, frame), frame, 1, rm.OK)        # enough is free already: a no-op


def test_evict_at_a_budget_of_one_row(gpu):
    frame = 9
    _evict_both(gpu, _hand_state(1, [0], frame), frame, 1, rm.ERR_CAPACITY)       # the row is in use this frame
    s, freed = _evict_both(gpu, _hand_state(1, [1], frame), frame, 1, rm.OK)
    assert list(freed) == [0] and s["free_top"] == 1
    _evict_both(gpu, _hand_state(1, [None], frame), frame, 1, rm.OK)              # nothing to do


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_evict_budget_sizes_around_a_workgroup(gpu, B):
    frame = 5032                                                   # (the stamp of a row 6000 frames old wraps below zero)
    rng = np.random.default_rng(B)
    ages = [None if rng.random() < 0.1 else int(a) for a in rng.choice([0, 0, 1, 1, 2, 3, 5, 62, 63, 64, 100, 6000], B)]
    ages[B - 1] = 3                                                # the last slot is occupied and old
    base = _hand_state(B, ages, frame, seed=B)
    older = sum(1 for a in ages if a)                              # occupied, age >= 1
    top = base.free_top
    for need in sorted({top, top + 1, top + max(1, older // 2), top + older}):
        s, freed = _evict_both(gpu, base.copy(), frame, need, rm.OK)
        assert need < top + older or B - 1 in freed                # (everything older than this frame: the last slot too)
    _evict_both(gpu, base.copy(), frame, top + older + 1, rm.ERR_CAPACITY)


# ===================================================================================================================
# traces
# ===================================================================================================================
@pytest.mark.parametrize("B", rm.TRACE_BUDGETS)
def test_trace_through_the_four_calls_stays_in_lockstep_with_the_model(gpu, pinned, B):
    """The random traces of test_residency_model_cpu.py through mark / evict / fetch / remap with the caller's protocol,
    the eviction asked for exactly the missing rows: after EVERY frame the device's whole state equals the model's."""
    G, M, frames = rm.trace_shape(B)
    trace = rm.random_trace(G, B, frames, seed=B)
    host_np = rm.pattern_rows(G, M)
    model = rm.SlotCache(G, B, M, host_np, sentinel=SENTINEL)
    dc = DeviceCache(gpu, G, B, M, pinned(host_np), cap=max(len(t[0]) for t in trace))
    dc.upload(model)
    fitted = refused = evictions = 0
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
            assert rc == model.evict(f, count), (f, rc, _last_error())
            if rc == rm.ERR_CAPACITY:
                assert len(need) > B, f
                refused += 1
                dc.unqueue(count)
                model.unqueue(mk.miss)
                s = assert_same_state(dc, model, f"frame {f} (refused)")
                rm.check_invariants(s["slot_of"], s["id_of_slot"], s["free_list"], s["free_top"], B)
                continue
            assert rc == rm.OK and dc.free_top == model.free_top
            evictions += dc.free_top > top
            model.adopt_free_order(dc.out(dc.free_list, B), top, model.free_top)
            _lib.check(dc.fetch(count, f), "hgs_resid_fetch")
            assert model.fetch(miss, frame=f) == rm.OK
            _lib.check(dc.remap(), "hgs_resid_remap")
            ro_m, po_m = model.remap(ri, pi, w)
        assert len(need) <= B, f
        fitted += 1
        ro, po = dc.out(dc.ro), dc.out(dc.po)
        assert np.array_equal(ro, ro_m) and np.array_equal(po, po_m), f
        s = assert_same_state(dc, model, f"frame {f}")
        rm.check_invariants(s["slot_of"], s["id_of_slot"], s["free_list"], s["free_top"], B)
        assert_slots_name_the_cut(s["id_of_slot"], ro, po, ri, pi, w)
        assert (s["stamp"][s["slot_of"][need]] == f).all(), f
        _assert_contents(s, host_np, M, np.nonzero(s["slot_of"] >= 0)[0])      # every resident row, not only this cut's
    model.check_invariants()
    assert fitted >= 20 and refused >= 20 and evictions >= 20, (fitted, refused, evictions)


def _budgeted(gpu, G, B, M, cap):
    from hgs.residency import BudgetedHierarchy
    rows = torch.from_numpy(rm.pattern_rows(G, M, pad=0.0))
    cols = {k: torch.from_numpy(c) for k, c in rm.field_columns(M).items()}
    bh = BudgetedHierarchy(rows[:, cols["means3D"]], rows[:, cols["shs"]].reshape(G, M, 3), rows[:, cols["opacities"]],
                           rows[:, cols["scales"]], rows[:, cols["rotations"]], gpu, budget_rows=B, index_capacity=cap)
    assert bh.B == B and bh.M == M
    return bh, rows.numpy()


def _bh_state(bh):
    torch.cuda.synchronize()
    s = dict(slot_of=bh.slot_of.cpu().numpy(), id_of_slot=bh.id_of_slot.cpu().numpy(),
             stamp=bh.stamp.cpu().numpy().view(np.uint32), free_list=bh.free_list.cpu().numpy(), free_top=bh.free_top)
    for k in rm.FIELDS:
        s[k] = getattr(bh, k).cpu().numpy().reshape(bh.B, -1)
    rm.check_invariants(s["slot_of"], s["id_of_slot"], s["free_list"], s["free_top"], bh.B)
    return s


def _assert_contents(s, host_np, M, ids):
    """The slot of every row of ``ids`` holds the bits of that row's fields."""
    slots = s["slot_of"][ids]
    assert (slots >= 0).all()
    for k, c in rm.field_columns(M).items():
        assert np.array_equal(_bits(s[k][slots]), _bits(host_np[ids][:, c])), k


def _to_gpu(gpu, ri, pi, w):
    t = lambda a: None if a is None else torch.from_numpy(a).to(gpu)
    return t(ri), t(pi), t(w)


@pytest.mark.parametrize("B", rm.TRACE_BUDGETS)
def test_trace_through_make_resident(gpu, B):
    """The same traces through BudgetedHierarchy.make_resident, whose batch eviction may free more than the model's:
    the properties instead of the state."""
    G, M, frames = rm.trace_shape(B)
    trace = rm.random_trace(G, B, frames, seed=B)
    bh, host_np = _budgeted(gpu, G, B, M, cap=max(len(t[0]) for t in trace))
    fitted = refused = 0
    before = _bh_state(bh)
    for f, (ri, pi, w) in enumerate(trace, start=1):
        need = rm.needed_rows(ri, pi, w)
        ok = True
        try:
            ro, po, m = bh.make_resident(*_to_gpu(gpu, ri, pi, w))
        except _lib.HgsError as e:
            assert e.code == _lib.ERR_CAPACITY, e
            ok = False
        assert ok == (len(need) <= B), (f, len(need), B)           # it succeeds exactly when the distinct rows fit
        s = _bh_state(bh)                                          # (invariants: no -2 left, stack and slots consistent)
        was = need[before["slot_of"][need] >= 0]
        if ok:
            fitted += 1
            _assert_contents(s, host_np, M, np.nonzero(s["slot_of"] >= 0)[0])
            assert (s["slot_of"][need] >= 0).all() and (s["stamp"][s["slot_of"][need]] == bh.frame).all()
            assert np.array_equal(s["slot_of"][was], before["slot_of"][was]), "a row needed this frame was evicted"
            assert m == len(need) - len(was)
            assert_slots_name_the_cut(s["id_of_slot"], ro.cpu().numpy(), po.cpu().numpy(), ri, pi, w)
        else:
            refused += 1
            assert np.array_equal(s["slot_of"], before["slot_of"]), "a refused frame changed the resident set"
            assert np.array_equal(s["id_of_slot"], before["id_of_slot"]) and s["free_top"] == before["free_top"]
        before = s
    assert fitted >= 20 and refused >= 20 and bh.stats["evictions"] > 0


@pytest.mark.parametrize("B", rm.TRACE_BUDGETS)
def test_best_effort_pass_keeps_every_row_of_the_frame(gpu, B):
    """A best-effort pass (what ``prefetch`` runs: no new frame number) after a frame: rows of that frame keep their
    slots and contents, whatever the pass could or could not bring in, and nothing is left queued."""
    G, M, _ = rm.trace_shape(B)
    trace = rm.random_trace(G, B, 120, seed=100 + B)
    bh, host_np = _budgeted(gpu, G, B, M, cap=max(len(t[0]) for t in trace))
    passes = brought = partial = 0
    for (ri, pi, w), nxt in zip(trace[0::2], trace[1::2]):
        need = rm.needed_rows(ri, pi, w)
        if len(need) > B:
            continue
        bh.make_resident(*_to_gpu(gpu, ri, pi, w))
        s0 = _bh_state(bh)
        ro, po, m = bh.make_resident(*_to_gpu(gpu, *nxt), _new_frame=False, _best_effort=True)
        s1 = _bh_state(bh)
        assert np.array_equal(s1["slot_of"][need], s0["slot_of"][need]), "the pass evicted a row of the frame"
        _assert_contents(s1, host_np, M, np.nonzero(s1["slot_of"] >= 0)[0])
        want = rm.needed_rows(*nxt)
        now = int((s1["slot_of"][want] >= 0).sum())
        assert m == now - int((s0["slot_of"][want] >= 0).sum())
        # rows stamped this frame stay; everything else may go: the pass completes exactly when both cuts fit together
        assert (ro is not None) == (len(np.union1d(need, want)) <= B)
        if ro is not None:
            assert now == len(want)
            assert_slots_name_the_cut(s1["id_of_slot"], ro.cpu().numpy(), po.cpu().numpy(), *nxt)
        else:
            partial += 1
            assert now < len(want)
        passes += 1
        brought += m > 0
    assert passes >= 10 and partial >= 1 and (brought >= 1 or B == 1), (passes, brought, partial)


# ===================================================================================================================
# refusals: status and message, before any launch
# ===================================================================================================================
def _refusal_fixture(gpu, pinned):
    G, B, M, n = 40, 8, 4, 5
    host_np = rm.pattern_rows(G, M)
    model = rm.SlotCache(G, B, M, host_np, sentinel=SENTINEL)
    assert model.fetch([3, 4, 5], frame=1) == rm.OK
    dc = DeviceCache(gpu, G, B, M, pinned(host_np), cap=n)
    dc.upload(model)
    dc.set_cut([3, 9, 9, 4, 10], [4, 4, 11, 12, 3], [0.5, 1.0, 0.0, 0.5, 1.0])
    dc.miss_ids[:2].copy_(torch.tensor([20, 21], dtype=torch.int32))
    return dc, model


def _snapshot(dc):
    torch.cuda.synchronize()
    return {k: t.cpu().clone() for k, t in dict(slot_of=dc.slot_of, stamp=dc.stamp, id_of_slot=dc.id_of_slot,
                                                free_list=dc.free_list, miss_ids=dc.miss_ids, ro=dc.ro, po=dc.po,
                                                **{"slot." + k: v for k, v in dc.rows.items()}).items()}


def _assert_untouched(dc, snap):
    now = _snapshot(dc)
    for k, v in snap.items():
        assert torch.equal(now[k].view(torch.uint8), v.view(torch.uint8)), f"{k} was written by a refused call"


def test_null_arguments_are_refused(gpu, pinned):
    dc, _ = _refusal_fixture(gpu, pinned)
    snap = _snapshot(dc)
    lib, p, dev, st = dc.lib, _lib.ptr, gpu.index or 0, _stream()
    miss, top = C.c_uint32(0), C.c_uint32(0)
    mark = [p(dc.ri), p(dc.pi), p(dc.w), dc.n, dc.G, p(dc.slot_of), p(dc.stamp), 2, p(dc.miss_ids), p(dc.counters),
            p(dc.ro), p(dc.po), C.byref(miss), st, dev]
    evict = [p(dc.stamp), p(dc.id_of_slot), p(dc.slot_of), dc.B, 2, dc.B, p(dc.free_list), p(dc.counters), C.byref(top),
             st, dev]
    fetch = [p(dc.miss_ids), 2, p(dc.free_list), dc.free_top, p(dc.slot_of), p(dc.id_of_slot), p(dc.stamp), 2,
             C.c_void_p(dc.host.ptr), C.byref(dc.slot_rows), dc.M, st, dev]
    remap = [p(dc.ri), p(dc.pi), p(dc.w), dc.n, p(dc.slot_of), p(dc.ro), p(dc.po), st, dev]
    for fn, args, nullable in ((lib.hgs_resid_mark, mark, (0, 1, 5, 6, 8, 9, 10, 11, 12)),
                               (lib.hgs_resid_evict, evict, (0, 1, 2, 6, 7, 8)),
                               (lib.hgs_resid_fetch, fetch, (0, 2, 4, 5, 6, 8, 9)),
                               (lib.hgs_resid_remap, remap, (0, 1, 4, 5, 6))):
        for i in nullable:
            a = list(args)
            a[i] = None
            assert fn(*a) == ERR_INVALID, (fn.__name__, i)
            assert "null" in _last_error(), (fn.__name__, i, _last_error())
    a = list(mark); a[4] = 0
    assert lib.hgs_resid_mark(*a) == ERR_INVALID                                   # G = 0
    a = list(evict); a[3] = 0
    assert lib.hgs_resid_evict(*a) == ERR_INVALID                                  # B = 0
    _assert_untouched(dc, snap)


def test_fetch_refuses_bad_widths_short_stacks_misaligned_rotations_and_unpinned_rows(gpu, pinned):
    dc, _ = _refusal_fixture(gpu, pinned)
    snap = _snapshot(dc)
    for M in (0, 17):
        assert dc.fetch(2, 2, M=M) == ERR_INVALID and "SH coefficients per channel: 1..16" in _last_error(), M
    assert dc.fetch(2, 2, free_top=1) == _lib.ERR_CAPACITY and "1 free slots for 2 missing rows" in _last_error()
    rot = torch.full((dc.B * 4 + 4,), float(SENTINEL), device=gpu)
    off = _lib.ResidRows(*[C.c_void_p(rot.data_ptr() + 4 if k == "rotations" else dc.rows[k].data_ptr())
                           for k in rm.FIELDS])
    assert dc.fetch(2, 2, slot_rows=off) == ERR_INVALID and "16-byte aligned" in _last_error()
    plain = np.ascontiguousarray(rm.pattern_rows(dc.G, dc.M))                     # ordinary numpy memory
    assert dc.fetch(2, 2, host_ptr=plain.ctypes.data) == ERR_INVALID and "hgs_host_alloc" in _last_error()
    assert dc.free_top == 5
    _assert_untouched(dc, snap)
    assert (rot.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()


def test_empty_calls_return_ok_and_touch_nothing(gpu, pinned):
    dc, _ = _refusal_fixture(gpu, pinned)
    snap = _snapshot(dc)
    n = dc.n
    dc.n = 0
    rc, count = dc.mark(2)
    assert rc == 0 and count == 0                                                  # (the count is written: zero)
    assert dc.remap() == 0
    dc.n = n
    assert dc.fetch(0, 2) == 0 and dc.free_top == 5
    assert dc.fetch(0, 2, free_top=0, M=0) == 0                                    # m = 0 returns before any check
    _assert_untouched(dc, snap)
