"""hgs_adam_step (csrc/adam.hip) through the C ABI, between guard bytes, against the float32 rule tests/adam_spec.py BIT
FOR BIT: all rows of param, exp_avg and exp_avg_sq of every tensor of every call -- selected rows equal the rule,
every other row keeps its initial bits -- and grad, the row list and the mask unchanged.  The rule is pinned to the header
the kernel compiles (csrc/adam_update.h) by tests/test_adam_update_on_host.py, so nothing here needs a compiler.

hgs_adam_tensor arrays are built by hand from adam_spec.tensor_constants (not through hgs.optim); in a call of several
tensors EVERY tensor has its own step size, betas, eps, weight decay and step count, so a wrong tensor lookup at a
first_block boundary changes bits.  Inputs: adam_spec.edge_inputs -- magnitudes over 1e-24..10, exact zeros on zero
moments, subnormals, +-3e19 (g^2 overflows), +-inf and NaN gradients, each of which must stay in its own element.

Preconditions kept by every case (adam_spec.selected asserts them BEFORE the launch): every listed row is in [0, P) -- a
row outside is undefined by contract and would be read and written out of bounds -- and no row is listed twice -- two
threads would race on it.  The 64-bit index instantiation (taken from 0x7fffff00 selected elements in one tensor, 34 GB)
is not run; it differs from the tested kernel in the index type only."""
import ctypes as C
import json
import time

import numpy as np
import pytest
import torch

import adam_spec as sp
import ws_guard

pytestmark = pytest.mark.gpu
MODEL = (3, 3, 45, 1, 3, 4)                          # xyz, f_dc, f_rest, opacity, scaling, rotation
EIGHT = MODEL + (1, 7)
NAMES = ("grad", "param", "exp_avg", "exp_avg_sq")   # (the order adam_spec.edge_inputs returns them in)
OUTPUTS = NAMES[1:]
MODES = ("dense", "list", "mask")
TALLY = dict(calls=0, tensors=0, elements=0, mismatches=0)


@pytest.fixture(scope="module", autouse=True)
def tally():
    t = time.perf_counter()
    yield
    res = dict(case="adam_edges", seconds=round(time.perf_counter() - t, 2), **TALLY)
    print("adam edges:", json.dumps(res))


def consts_for(k, step=0):
    """Tensor k's constants: no two tensors of a call share a step size, a beta, eps, a weight decay or a step count."""
    return sp.tensor_constants(lr=(1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3, 2e-2, 7e-4)[k],
                               betas=(0.9 - 0.04 * k, 0.999 - 0.011 * k),
                               eps=(1e-15, 1e-8, 1e-12, 3e-15, 1e-10, 1e-6, 1e-20, 1e-9)[k],
                               weight_decay=(0.0, 0.01, 1e-3, 0.1, 3e-4, 0.02, 1e-5, 0.5)[k], step=1 + 3 * k + step)


def _upload(gpu, a, name):
    a = np.ascontiguousarray(a)
    g = ws_guard.guarded(a.nbytes, gpu, 0x00, name)
    g.body.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))
    return g


def _download(g, dtype, shape):
    return g.body.cpu().numpy().view(dtype).reshape(shape)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Model:
    """Tensors [P, row_len] on both sides: `host` is what the rule says they hold, `dev` their guarded device bodies."""

    def __init__(self, gpu, P, row_lens, seed, planted=sp.PLANTED_G):
        self.gpu, self.P, self.row_lens = gpu, P, tuple(row_lens)
        rng = np.random.default_rng(seed)
        self.host = [dict(zip(NAMES, sp.edge_inputs(rng, (P, L), planted))) for L in self.row_lens]
        self.dev = [{n: _upload(gpu, a, f"tensor {k} (row_len {h['grad'].shape[1]}) {n}") for n, a in h.items()}
                    for k, h in enumerate(self.host)]

    def set_grads(self, seed, planted=sp.PLANTED_G):
        rng = np.random.default_rng(seed)
        for h, d in zip(self.host, self.dev):
            h["grad"] = sp.edge_inputs(rng, h["grad"].shape, planted)[0]
            d["grad"].body.copy_(torch.from_numpy(h["grad"].reshape(-1).view(np.uint8).copy()))

    def read(self, k, n):
        return _download(self.dev[k][n], np.float32, (self.P, self.row_lens[k]))

    def step(self, consts, what, rows=None, n_rows=None, mask=None, mask_of=None, stream=None):
        """One hgs_adam_step over all tensors, every guard checked, every row of every output compared with the rule.
        rows: int64 list (n_rows: the count passed, default all of it); mask: float32 [P]; mask_of: the mask IS tensor
        mask_of's gradient (row_len 1), the same device bytes."""
        from hgs import _lib
        P = self.P
        if mask_of is not None:
            assert self.row_lens[mask_of] == 1 and mask is None
            mask = self.host[mask_of]["grad"].reshape(-1)
        rows_np = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        listed = None if rows_np is None else rows_np[:rows_np.size if n_rows is None else n_rows]
        sel = sp.selected(P, listed, mask)                       # (asserts the preconditions before anything runs)
        guards = [g for d in self.dev for g in d.values()]
        rows_g = mask_g = None
        if rows_np is not None:
            rows_g = _upload(self.gpu, rows_np, "row list")
            guards.append(rows_g)
        if mask is not None and mask_of is None:
            mask_g = _upload(self.gpu, np.asarray(mask, dtype=np.float32), "row mask")
            guards.append(mask_g)
        mask_addr = self.dev[mask_of]["grad"].addr if mask_of is not None else (mask_g.addr if mask_g else None)
        arr = (_lib.AdamTensor * len(self.dev))(*[
            _lib.AdamTensor(param=d["param"].addr, grad=d["grad"].addr, exp_avg=d["exp_avg"].addr,
                            exp_avg_sq=d["exp_avg_sq"].addr, row_len=L, **{f: float(x) for f, x in T._asdict().items()})
            for d, L, T in zip(self.dev, self.row_lens, consts)])
        torch.cuda.synchronize()                                 # the uploads ran on the default stream
        rc = _lib.lib().hgs_adam_step(arr, len(self.dev), P, None if rows_g is None else C.c_void_p(rows_g.addr),
                                      0 if listed is None else listed.size,
                                      None if mask_addr is None else C.c_void_p(mask_addr),
                                      C.c_void_p(0 if stream is None else stream.cuda_stream), self.gpu.index or 0)
        assert rc == 0, (what, rc, _lib.lib().hgs_last_error())
        ws_guard.check(*guards)
        TALLY["calls"] += 1
        if rows_g is not None:
            assert np.array_equal(_download(rows_g, np.int64, rows_np.shape), rows_np), f"{what}: the row list changed"
        if mask_g is not None:
            assert np.array_equal(_download(mask_g, np.uint32, (P,)), _bits(np.asarray(mask, np.float32))), \
                f"{what}: the mask changed"
        for k, (h, T) in enumerate(zip(self.host, consts)):
            name = f"{what}, tensor {k} of {len(self.host)} (row_len {self.row_lens[k]}, P {P})"
            assert np.array_equal(_bits(self.read(k, "grad")), _bits(h["grad"])), f"{name}: grad changed"
            want = dict(zip(OUTPUTS, sp.step(T, h["param"], h["grad"], h["exp_avg"], h["exp_avg_sq"], rows=listed,
                                             mask=None if listed is not None else mask)))
            TALLY["tensors"] += 1
            for n in OUTPUTS:
                got = self.read(k, n)
                TALLY["elements"] += got.size
                TALLY["mismatches"] += int((~sp.same_bits(got, want[n])).sum())
                sp.assert_same_bits(got[~sel], h[n][~sel], f"{name}, {n}, UNSELECTED rows (numbered among them)", exact=True)
                sp.assert_same_bits(got, want[n], f"{name}, {n}")
            for n in OUTPUTS:
                h[n] = want[n]
        return sel


def _selection(mode, P, rng):
    """rows / mask keywords of a call by mode: an unsorted list of about half the rows, or a mask half zero."""
    if mode == "list":
        return dict(rows=rng.permutation(P)[:max(1, (P + 1) // 2)])
    if mode == "mask":
        m = rng.normal(size=P).astype(np.float32)
        m[rng.random(P) < 0.5] = 0
        return dict(mask=m)
    return {}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("row_len", (1, 3, 4, 45))
def test_grid_edges_of_one_tensor(gpu, row_len, mode):
    """Element counts on both sides of a 256-thread block: row_len 3 at P 85 / 86 is 255 / 258, row_len 45 at P 5 / 6 is
    225 / 270 (and from P = 6 a row lies across a block boundary), row_len 4 at P 64 is one block with no idle lane."""
    rng = np.random.default_rng(row_len * 10 + MODES.index(mode))
    for P in (1, 5, 6, 63, 64, 65, 85, 86, 255, 256, 257, 1000):
        m = Model(gpu, P, (row_len,), seed=P * 100 + row_len)
        m.step([consts_for(P % 8)], f"{mode}, one tensor", **_selection(mode, P, rng))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", (1, 64, 256, 257))
@pytest.mark.parametrize("n", (2, 6, 8))
def test_tensor_seams(gpu, n, P, mode):
    """Several tensors in one call, each with constants of its own.  P = 256 ends the row_len 1 tensor exactly on a block
    boundary, with another tensor behind it."""
    row_lens = (1, 45) if n == 2 else EIGHT[:n]
    m = Model(gpu, P, row_lens, seed=n * 1000 + P)
    m.step([consts_for(k) for k in range(n)], f"{mode}, {n} tensors",
           **_selection(mode, P, np.random.default_rng(n + P + MODES.index(mode))))


@pytest.mark.parametrize("mode", MODES)
def test_eight_tensors_of_one_element(gpu, mode):
    m = Model(gpu, 1, (1,) * 8, seed=8, planted=())
    sel = dict(rows=[0]) if mode == "list" else dict(mask=np.array([-3.0], np.float32)) if mode == "mask" else {}
    m.step([consts_for(k) for k in range(8)], f"{mode}, eight single elements", **sel)


@pytest.fixture(scope="module")
def big(gpu):
    return Model(gpu, 100_003, MODEL, seed=100_003)


def test_model_shaped_call_dense_then_by_row_list(big):
    """Six tensors of 100 003 rows: about 17 600 blocks for f_rest, every first_block far from zero.  The second call
    runs on the first one's outputs."""
    consts = [consts_for(k) for k in range(6)]
    big.step(consts, "dense, model at 100003 rows")
    big.set_grads(seed=7)
    rows = np.random.default_rng(5).permutation(big.P)[:40_000]
    sel = big.step([consts_for(k, step=1) for k in range(6)], "list, model at 100003 rows", rows=rows)
    assert sel.sum() == 40_000


@pytest.mark.parametrize("row_len", (3, 45))
def test_row_lists(gpu, row_len):
    P = 257
    rng = np.random.default_rng(row_len)
    lists = {"one row": [128], "first and last row": [0, P - 1], "all rows ascending": np.arange(P),
             "all rows descending": np.arange(P)[::-1], "random unsorted 40 %": rng.permutation(P)[:103]}
    for what, rows in lists.items():
        m = Model(gpu, P, (row_len,), seed=len(what) + row_len)
        sel = m.step([consts_for(2)], what, rows=rows)
        assert sel.sum() == len(rows)
    # n_rows == 0 with a list pointer that is not null: HGS_OK and nothing changes
    m = Model(gpu, P, (row_len, 1), seed=99)
    before = [{n: a.copy() for n, a in h.items()} for h in m.host]
    sel = m.step([consts_for(0), consts_for(1)], "an empty list at a non-null pointer", rows=[5, 6], n_rows=0)
    assert not sel.any()
    for k, h in enumerate(before):
        for n, a in h.items():
            assert np.array_equal(_bits(m.read(k, n)), _bits(a)), (k, n)


MASK_VALUES = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, np.nan, np.inf, -np.inf, 0.5, -2.0, 0.0, 3e-39, 1e-20],
                       dtype=np.float32)
MASK_SELECTS = np.array([0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1], dtype=bool)


def _mask_257():
    idx = np.random.default_rng(257).integers(0, MASK_VALUES.size, size=257)
    idx[:MASK_VALUES.size] = np.arange(MASK_VALUES.size)
    return MASK_VALUES[idx], MASK_SELECTS[idx]


def test_mask_values(gpu):
    """+0.0 and -0.0 skip the row; subnormals of either sign, NaN, the infinities and ordinary values select it."""
    mask, selects = _mask_257()
    assert np.array_equal(mask != 0, selects)                    # (numpy's != states the rule)
    m = Model(gpu, 257, MODEL, seed=257)
    sel = m.step([consts_for(k) for k in range(6)], "mask values", mask=mask)
    assert np.array_equal(sel, selects)


def test_the_mask_is_a_gradient_of_the_same_call(gpu):
    """As step_masked(opacity.grad) does: the mask pointer is tensor 3's gradient (row_len 1), read in both roles."""
    mask, selects = _mask_257()
    m = Model(gpu, 257, MODEL, seed=258)
    m.host[3]["grad"] = mask.reshape(257, 1).copy()
    m.dev[3]["grad"].body.copy_(torch.from_numpy(mask.view(np.uint8).copy()))
    sel = m.step([consts_for(k) for k in range(6)], "the mask is opacity's gradient", mask_of=3)
    assert np.array_equal(sel, selects)


@pytest.mark.parametrize("P", (65, 1003))
def test_thirty_steps_chained(gpu, P):
    """Fresh gradients every step, modes cycling dense / list / mask, the step count (so both bias corrections) advancing;
    the outputs of step k are the inputs of step k + 1 on both sides, and the bits agree after every step."""
    m = Model(gpu, P, MODEL, seed=P)
    rng = np.random.default_rng(P + 1)
    for it in range(30):
        if it:
            m.set_grads(seed=P * 100 + it, planted=sp.PLANTED_G if it % 10 == 5 else ())
        mode = MODES[it % 3]
        m.step([consts_for(k, step=it) for k in range(6)], f"step {it + 1} of 30 ({mode})", **_selection(mode, P, rng))
    finite = np.mean([np.isfinite(h["param"]).mean() for h in m.host])
    assert finite > 0.9, finite                                  # (the chain did not drown in NaN)


def test_two_calls_give_the_same_bits_also_on_a_second_stream(gpu):
    side = torch.cuda.Stream(device=gpu)
    outs = []
    for stream in (None, None, side):
        m = Model(gpu, 1003, MODEL, seed=77)
        m.step([consts_for(k) for k in range(6)], "repeat" if stream is None else "second stream",
               stream=stream, **_selection("list", 1003, np.random.default_rng(3)))
        outs.append([_bits(m.read(k, n)).copy() for k in range(6) for n in OUTPUTS])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)
