"""A plain slot cache: the contract of hgs_resid_mark / _evict / _fetch / _remap (include/hgs.h, the block above
HGS_RESID_COUNTER_WORDS) restated in sequential numpy, with no parallelism, no atomics and no queues.  A helper module
of the tests (test_residency_model_cpu.py checks it without a GPU, test_residency_kernels_gpu.py holds the HIP kernels
against it); the product never imports it.  Every quantity is an integer or a float's bits: nothing here is approximate.

Where the header leaves an order open (the miss list, the slots an eviction pushes on the free stack) the model picks
ascending order and offers ``adopt_free_order`` / an explicit miss list to ``fetch`` so that a test can follow the
order the device chose -- after it has checked that the SETS agree -- and stay in lockstep with it from then on.

One detail is taken from csrc/residency.hip rather than from the header's prose, and is marked where it occurs: a
parent index outside [0, G) raises the error flag (and reports -1) even when the entry's weight is exactly 1."""
import numpy as np

OK, ERR_INVALID, ERR_CAPACITY = 0, 1, 5
AGES = 64                       # ages saturate at AGES - 1
ROW = 64                        # floats of a packed host row (HGS_RESID_HOST_ROW_FLOATS)
ABSENT, QUEUED = -1, -2
# packed host row: [0, 3 M) SH, [48, 52) rotation, [52, 55) mean, [55, 58) scale, [58] opacity
SH0, ROT0, MEAN0, SCALE0, OPAC = 0, 48, 52, 55, 58
FIELDS = ("means3D", "shs", "opacities", "scales", "rotations")


def field_columns(M):
    """Columns of the packed row that make up each slot array's row."""
    return dict(means3D=np.arange(MEAN0, MEAN0 + 3), shs=np.arange(SH0, SH0 + 3 * M), opacities=np.arange(OPAC, OPAC + 1),
                scales=np.arange(SCALE0, SCALE0 + 3), rotations=np.arange(ROT0, ROT0 + 4))


def pattern_rows(G, M, pad=np.nan):
    """Packed host rows whose float at (id, col) is id * 64 + col -- distinct and exact in float32 up to id = 2^18 --
    with the padding columns [3 M, 48) and [59, 64) holding ``pad``: a field taken from the wrong lane, component or
    row, or a padding column that reaches a slot array, shows in the bits."""
    assert G * ROW < (1 << 24)
    rows = (np.arange(G, dtype=np.float32)[:, None] * ROW + np.arange(ROW, dtype=np.float32)[None, :]).astype(np.float32)
    rows[:, 3 * M:ROT0] = pad
    rows[:, OPAC + 1:] = pad
    return rows


def needed_rows(ri, pi, weights):
    """Distinct rows a cut needs: every ri[i], and pi[i] unless the entry's weight is exactly 1 (NaN != 1: needed)."""
    ri, pi = np.asarray(ri, np.int64), np.asarray(pi, np.int64)
    par = np.ones(len(ri), bool) if weights is None else ~(np.asarray(weights, np.float32) == np.float32(1.0))
    return np.unique(np.concatenate([ri, pi[par]]))


class MarkResult:
    def __init__(self, miss, ro, po, error):
        self.miss, self.ro, self.po, self.error = miss, ro, po, error
        self.status = ERR_INVALID if error else OK


class SlotCache:
    def __init__(self, G, B, M=16, host_rows=None, sentinel=np.float32(-12345.0)):
        self.G, self.B, self.M = int(G), int(B), int(M)
        self.slot_of = np.full(G, ABSENT, np.int32)
        self.id_of_slot = np.full(B, -1, np.int32)
        self.stamp = np.zeros(B, np.uint32)
        self.free_list = np.arange(B - 1, -1, -1, dtype=np.int32)       # slot 0 is handed out first
        self.free_top = int(B)
        self.frame = 0
        self.host_rows = host_rows
        self.cols = field_columns(M)
        self.rows = {k: np.full((B, len(c)), sentinel, np.float32) for k, c in self.cols.items()}

    def copy(self):
        c = SlotCache.__new__(SlotCache)
        c.__dict__.update(self.__dict__)
        for k in ("slot_of", "id_of_slot", "stamp", "free_list"):
            setattr(c, k, getattr(self, k).copy())
        c.rows = {k: v.copy() for k, v in self.rows.items()}
        return c

    # ---------------------------------------------------------------------------------------------------------------
    @property
    def resident(self):
        """ids of the resident rows, ascending."""
        return np.nonzero(self.slot_of >= 0)[0]

    def ages(self, frame):
        """min((frame - stamp) mod 2^32, 63) of every slot (meaningful for the occupied ones)."""
        d = (np.uint64(int(frame) & 0xFFFFFFFF) + np.uint64(1 << 32) - self.stamp.astype(np.uint64)) % np.uint64(1 << 32)
        return np.minimum(d, np.uint64(AGES - 1)).astype(np.int64)

    # ---------------------------------------------------------------------------------------------------------------
    def mark(self, ri, pi, weights, frame):
        ri, pi = np.asarray(ri, np.int64), np.asarray(pi, np.int64)
        n = len(ri)
        self.frame = int(frame)
        par = np.ones(n, bool) if weights is None else ~(np.asarray(weights, np.float32) == np.float32(1.0))
        ok_r, ok_p = (ri >= 0) & (ri < self.G), (pi >= 0) & (pi < self.G)
        error = bool((~ok_r).any() or (~ok_p).any())       # (kernel: a bad pi is flagged whatever the entry's weight)
        need = np.unique(np.concatenate([ri[ok_r], pi[ok_p & par]])).astype(np.int64)
        assert not (self.slot_of[need] == QUEUED).any(), "rows of an earlier pass are still queued"
        here = self.slot_of[need] >= 0
        self.stamp[self.slot_of[need[here]]] = np.uint32(self.frame & 0xFFFFFFFF)
        miss = need[~here]
        self.slot_of[miss] = QUEUED
        ro = np.full(n, -1, np.int32)
        ro[ok_r] = self.slot_of[ri[ok_r]]
        po = np.full(n, -1, np.int32)
        po[ok_p & par] = self.slot_of[pi[ok_p & par]]
        po[ok_p & ~par] = ro[ok_p & ~par]
        return MarkResult(miss.astype(np.int32), ro, po, error)

    def unqueue(self, miss_ids):
        """The caller's part after a refused frame: queued rows go back to absent."""
        ids = np.asarray(miss_ids, np.int64)
        q = ids[self.slot_of[ids] == QUEUED]
        self.slot_of[q] = ABSENT

    def evict(self, frame, need, free_top=None):
        if free_top is not None:
            self.free_top = int(free_top)
        need = int(need)
        if self.free_top >= need:
            return OK
        occ = self.id_of_slot >= 0
        age = self.ages(frame)
        missing = need - self.free_top
        min_age = 0
        for a in range(AGES - 1, 0, -1):
            if int((occ & (age >= a)).sum()) >= missing:
                min_age = a
                break
        if min_age == 0:
            return ERR_CAPACITY
        out = np.nonzero(occ & (age >= min_age))[0]            # ALL of them, not just enough
        self.slot_of[self.id_of_slot[out]] = ABSENT
        self.id_of_slot[out] = -1
        self.free_list[self.free_top:self.free_top + len(out)] = out
        self.free_top += len(out)
        return OK

    def adopt_free_order(self, free_list, lo, hi):
        """Entries [lo, hi) of the free stack in the order the device pushed them (the same slots: asserted)."""
        got = np.asarray(free_list[lo:hi], np.int32)
        assert np.array_equal(np.sort(got), np.sort(self.free_list[lo:hi])), "another set of slots was freed"
        self.free_list[lo:hi] = got

    def fetch(self, miss_ids, m=None, free_top=None, frame=None):
        """Miss j takes free_list[free_top - 1 - j].  Unlike the C call the model also pops the stack (the C ABI's
        caller does that: free_top -= m)."""
        miss_ids = np.asarray(miss_ids, np.int64)
        m = len(miss_ids) if m is None else int(m)
        if free_top is not None:
            self.free_top = int(free_top)
        if frame is not None:
            self.frame = int(frame)
        if m == 0:
            return OK
        if self.free_top < m:
            return ERR_CAPACITY
        for j in range(m):
            g, s = int(miss_ids[j]), int(self.free_list[self.free_top - 1 - j])
            self.slot_of[g] = s
            self.id_of_slot[s] = g
            self.stamp[s] = np.uint32(self.frame & 0xFFFFFFFF)
            if self.host_rows is not None:
                for k, c in self.cols.items():
                    self.rows[k][s] = self.host_rows[g, c]
        self.free_top -= m
        return OK

    def remap(self, ri, pi, weights):
        ri, pi = np.asarray(ri, np.int64), np.asarray(pi, np.int64)
        ro = self.slot_of[ri].astype(np.int32)
        if weights is None:
            return ro, self.slot_of[pi].astype(np.int32)
        one = np.asarray(weights, np.float32) == np.float32(1.0)
        return ro, np.where(one, ro, self.slot_of[np.where(one, 0, pi)]).astype(np.int32)

    def make_resident(self, ri, pi, weights, frame):
        """The caller's protocol with an eviction of exactly the missing rows: (status, ro, po, rows fetched)."""
        mk = self.mark(ri, pi, weights, frame)
        if mk.error:
            self.unqueue(mk.miss)
            return ERR_INVALID, mk.ro, mk.po, 0
        m = len(mk.miss)
        if m == 0:
            return OK, mk.ro, mk.po, 0
        if self.evict(frame, m) != OK:
            self.unqueue(mk.miss)
            return ERR_CAPACITY, None, None, 0
        rc = self.fetch(mk.miss, frame=frame)
        assert rc == OK
        ro, po = self.remap(ri, pi, weights)
        return OK, ro, po, m

    # ---------------------------------------------------------------------------------------------------------------
    def check_invariants(self):
        check_invariants(self.slot_of, self.id_of_slot, self.free_list, self.free_top, self.B)
        if self.host_rows is not None:
            occ = np.nonzero(self.id_of_slot >= 0)[0]
            for k, c in self.cols.items():
                want = self.host_rows[self.id_of_slot[occ]][:, c]
                assert np.array_equal(self.rows[k][occ].view(np.uint32), want.view(np.uint32)), k


def check_invariants(slot_of, id_of_slot, free_list, free_top, B):
    """slot_of / id_of_slot are inverse on the occupied slots, nothing is left queued, the free stack holds every free
    slot once and no occupied one, resident + free_top == B.  (Plain arrays: the device's state goes through it too.)"""
    slot_of, id_of_slot = np.asarray(slot_of, np.int64), np.asarray(id_of_slot, np.int64)
    assert len(id_of_slot) == B and 0 <= free_top <= B
    assert not (slot_of == QUEUED).any(), "a row is left queued"
    assert ((slot_of >= 0) | (slot_of == ABSENT)).all() and (slot_of < B).all()
    occ = np.nonzero(id_of_slot >= 0)[0]
    res = np.nonzero(slot_of >= 0)[0]
    assert (id_of_slot[occ] < len(slot_of)).all()
    assert np.array_equal(slot_of[id_of_slot[occ]], occ), "slot_of[id_of_slot[s]] != s"
    assert np.array_equal(id_of_slot[slot_of[res]], res), "id_of_slot[slot_of[g]] != g"
    assert (id_of_slot[id_of_slot < 0] == -1).all()
    free = np.asarray(free_list[:free_top], np.int64)
    assert len(np.unique(free)) == free_top, "a slot is on the free stack twice"
    assert ((free >= 0) & (free < B)).all() and (id_of_slot[free] == -1).all(), "an occupied slot is on the free stack"
    assert len(res) + free_top == B, (len(res), free_top, B)


def state_of(model):
    """The model's state under the names a device read-back uses."""
    return dict(slot_of=model.slot_of, id_of_slot=model.id_of_slot, stamp=model.stamp, free_list=model.free_list,
                free_top=model.free_top, **model.rows)


def by_id(state, ro, po):
    """A state and a cut's slot indices in a form that does not depend on which slot a row got (the orders of the miss
    list and of the free stack are open): resident ids, their stamps and slot rows in id order, the ids ro / po name."""
    res = np.nonzero(state["slot_of"] >= 0)[0]
    slots = state["slot_of"][res]
    out = dict(resident=res, stamp=state["stamp"][slots].astype(np.int64), free_top=int(state["free_top"]),
               ro_ids=state["id_of_slot"][np.asarray(ro, np.int64)], po_ids=state["id_of_slot"][np.asarray(po, np.int64)])
    for k in FIELDS:
        out[k] = np.ascontiguousarray(state[k][slots], dtype=np.float32).view(np.uint32).astype(np.int64)
    return out


# ===================================================================================================================
# traces
# ===================================================================================================================
TRACE_BUDGETS = (1, 7, 64, 257)


def trace_shape(B):
    """(G, M, frames) of the random trace at budget ``B``: G <= 2000; M covers both SH store paths of the fetch."""
    return min(2000, 8 * B + 5), {1: 1, 7: 9, 64: 4, 257: 16}[B], 300


def random_trace(G, B, frames, seed):
    """``frames`` cuts (ri, pi, weights or None) over G rows.  Each draws its entries from a pool of k consecutive rows
    (wrapping) that drifts through the hierarchy, k between 1 and ~1.3 B: most frames reuse rows of the last ones, some
    need more distinct rows than the budget holds.  Ids repeat within ri, within pi and across both; a quarter of the
    frames carry no weights, the others have shares exactly 1 and now and then a NaN."""
    rng = np.random.default_rng(seed)
    out, start = [], 0
    for _ in range(frames):
        k = int(rng.integers(1, int(1.3 * B) + 3))
        start = (start + int(rng.integers(0, max(2, k // 3)))) % G
        pool = (start + np.arange(k)) % G
        n = int(rng.integers(1, 2 * k + 2))
        ri = rng.choice(pool, n).astype(np.int32)
        pi = rng.choice(pool, n).astype(np.int32)
        if rng.random() < 0.25:
            w = None
        else:
            w = rng.choice(np.array([1.0, 1.0, 0.0, 0.25, 0.999999], np.float32), n).astype(np.float32)
            if rng.random() < 0.2:
                w[int(rng.integers(n))] = np.nan
        out.append((ri, pi, w))
    return out
