"""The plain slot cache of tests/residency_model.py -- the reference the residency kernels are held against -- checked on
its own, without a GPU: invariants over random traces at budgets where every frame evicts, "a frame fits exactly when
its distinct rows number at most B" in both directions, and the age rule at its edges (saturation at 63, unsigned
frame - stamp)."""
import numpy as np
import pytest

import residency_model as rm


@pytest.mark.parametrize("B", rm.TRACE_BUDGETS)
def test_random_traces_keep_the_invariants_and_fit_exactly_when_the_rows_do(B):
    G, M, frames = rm.trace_shape(B)
    assert G <= 2000 and frames >= 200
    host = rm.pattern_rows(G, M)
    c = rm.SlotCache(G, B, M, host)
    fitted = refused = evicting = 0
    for f, (ri, pi, w) in enumerate(rm.random_trace(G, B, frames, seed=B), start=1):
        need = rm.needed_rows(ri, pi, w)
        before = c.copy()
        rc, ro, po, m = c.make_resident(ri, pi, w, f)
        c.check_invariants()
        was_resident = need[before.slot_of[need] >= 0]
        if len(need) <= B:
            assert rc == rm.OK, (f, len(need), B)
            fitted += 1
            evicting += c.free_top + m > before.free_top                   # slots were freed on the way
            assert (c.slot_of[need] >= 0).all()
            assert (c.stamp[c.slot_of[need]] == f).all()                   # needed rows are age 0 ...
            others = np.setdiff1d(c.resident, need)
            assert (c.ages(f)[c.slot_of[others]] >= 1).all()               # ... and everything else is older
            # no row needed this frame lost its slot; what was fetched is what was missing
            assert np.array_equal(c.slot_of[was_resident], before.slot_of[was_resident])
            assert m == len(need) - len(was_resident)
            assert np.array_equal(c.id_of_slot[ro], ri)
            par = np.ones(len(ri), bool) if w is None else ~(w == np.float32(1.0))
            assert np.array_equal(c.id_of_slot[po[par]], pi[par]) and np.array_equal(po[~par], ro[~par])
        else:
            assert rc == rm.ERR_CAPACITY, (f, len(need), B)
            refused += 1
            assert np.array_equal(c.slot_of, before.slot_of) and np.array_equal(c.id_of_slot, before.id_of_slot)
            assert c.free_top == before.free_top and np.array_equal(c.free_list, before.free_list)
            for k in rm.FIELDS:
                assert np.array_equal(c.rows[k].view(np.uint32), before.rows[k].view(np.uint32))
            # the mark pass of the refused frame still stamped the rows it found
            assert (c.stamp[c.slot_of[was_resident]] == f).all()
    assert fitted >= 20 and refused >= 20 and evicting >= 20, (fitted, refused, evicting)


def _occupied(B, stamps, G=None):
    """A full cache: slot s holds row B - 1 - s, stamped stamps[s]."""
    c = rm.SlotCache(G or B, B, 1)
    c.id_of_slot[:] = np.arange(B - 1, -1, -1)
    c.slot_of[c.id_of_slot] = np.arange(B)
    c.stamp[:] = np.asarray(stamps, np.uint64).astype(np.uint32)
    c.free_top = 0
    c.check_invariants()
    return c


def test_ages_saturate_at_63_and_old_rows_go_together():
    frame = 1000
    c = _occupied(4, [frame - 70, frame - 200, frame - 1, frame])
    assert list(c.ages(frame)) == [63, 63, 1, 0]
    assert c.evict(frame, 1) == rm.OK                 # one slot is asked for: both saturated ones go, age 1 stays
    assert c.free_top == 2 and sorted(c.free_list[:2]) == [0, 1]
    assert list(c.id_of_slot) == [-1, -1, 1, 0] and list(c.slot_of) == [3, 2, -1, -1]
    c.check_invariants()


def test_frame_minus_stamp_is_unsigned():
    c = _occupied(4, [0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFC, 1])
    assert list(c.ages(1)) == [3, 2, 5, 0]
    assert c.evict(1, 2) == rm.OK                     # ages 5 and 3; age 2 stays
    assert c.free_top == 2 and sorted(c.free_list[:2]) == [0, 2]
    assert c.evict(1, 4) == rm.ERR_CAPACITY and c.free_top == 2          # one row of age >= 1 is left, two are asked for
    c.check_invariants()


def test_evict_boundaries():
    frame = 10
    c = _occupied(5, [9, 9, 9, 10, 10])               # three rows of age 1, two of age 0
    d = c.copy()
    assert d.evict(frame, 4) == rm.ERR_CAPACITY       # a row stamped this frame is never freed
    assert np.array_equal(d.slot_of, c.slot_of) and np.array_equal(d.id_of_slot, c.id_of_slot) and d.free_top == 0
    assert c.evict(frame, 3) == rm.OK and c.free_top == 3 and sorted(c.free_list[:3]) == [0, 1, 2]
    assert c.evict(frame, 3) == rm.OK and c.free_top == 3                # enough is free: nothing happens
    e = _occupied(1, [frame])
    assert e.evict(frame, 1) == rm.ERR_CAPACITY
    assert e.evict(frame + 1, 1) == rm.OK and e.free_top == 1 and e.slot_of[0] == -1


def test_mark_reports_bad_indices_and_still_queues_the_valid_rows():
    c = rm.SlotCache(10, 4, 1)
    assert c.make_resident([2, 3], [3, 3], None, 1)[0] == rm.OK
    w = np.array([0.5, 1.0, 1.0, np.nan], np.float32)
    mk = c.mark([2, 10, 5, 6], [-1, 7, 8, 6], w, 2)
    assert mk.error and mk.status == rm.ERR_INVALID
    assert list(mk.miss) == [5, 6]                                        # 7, 8: weight 1; 10, -1: outside
    assert list(mk.ro) == [0, -1, -2, -2] and list(mk.po) == [-1, -1, -2, -2]
    assert list(c.stamp[:2]) == [2, 1]                                    # row 2 was stamped, row 3 not
    c.unqueue(mk.miss)
    c.check_invariants()
    assert list(c.resident) == [2, 3]


def test_fetch_takes_slots_from_the_top_of_the_stack_and_the_fields_of_the_packed_row():
    M = 2
    host = rm.pattern_rows(6, M)
    c = rm.SlotCache(6, 3, M, host)
    assert c.fetch([4, 1], frame=7) == rm.OK
    assert list(c.slot_of) == [-1, 1, -1, -1, 0, -1] and c.free_top == 1 and list(c.stamp) == [7, 7, 0]
    assert list(c.rows["shs"][0]) == [4 * 64 + k for k in range(6)]
    assert list(c.rows["rotations"][1]) == [64 + 48 + k for k in range(4)]
    assert list(c.rows["means3D"][1]) == [64 + 52, 64 + 53, 64 + 54]
    assert list(c.rows["scales"][0]) == [4 * 64 + 55, 4 * 64 + 56, 4 * 64 + 57] and c.rows["opacities"][0, 0] == 4 * 64 + 58
    assert (c.rows["means3D"][2] == np.float32(-12345.0)).all()           # the unassigned slot keeps the sentinel
    assert not any(np.isnan(v).any() for v in c.rows.values())            # no padding column reaches a slot
    assert c.fetch([0, 2], frame=7) == rm.ERR_CAPACITY
    c.check_invariants()
