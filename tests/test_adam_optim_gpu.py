"""hgs.optim.Adam's own logic on the GPU -- chunking above HGS_ADAM_MAX_TENSORS, two row counts, parameters without a
gradient, a learning rate changed between steps, views, the `relevant` variants, a step issued in parts, 0- and 1-dim
parameters, state edited as densification edits it -- against the float32 rule tests/adam_spec.py with
adam_spec.tensor_constants, BIT FOR BIT (tests/test_adam_update_on_host.py pins that rule to the header the kernel
compiles; tests/test_adam_edges_gpu.py holds the kernel itself to it through the C ABI)."""
import numpy as np
import pytest
import torch

import adam_spec as sp

pytestmark = pytest.mark.gpu
BETAS, EPS = (0.9, 0.999), 1e-15


class Twin:
    """One parameter on both sides: the torch Parameter the optimizer steps, and what the rule says it and its state hold."""

    def __init__(self, gpu, shape, lr, seed, wd=0.0):
        self.rng = np.random.default_rng(seed)
        self.shape, self.lr, self.wd, self.t = tuple(shape), lr, wd, 0
        g, p, _, _ = sp.edge_inputs(self.rng, self._2d(), planted=())
        self.p, self.m, self.v = p, np.zeros_like(p), np.zeros_like(p)
        self.param = torch.nn.Parameter(torch.from_numpy(p.reshape(self.shape).copy()).to(gpu))
        self.new_grad()

    def _2d(self):
        rows = self.shape[0] if self.shape else 1
        return rows, int(np.prod(self.shape, dtype=np.int64)) // rows

    def new_grad(self):
        self.g = sp.edge_inputs(self.rng, self._2d())[0]
        self.param.grad = torch.from_numpy(self.g.reshape(self.shape).copy()).to(self.param.device)

    def expect(self, rows=None, mask=None, lr=None):
        self.t += 1
        T = sp.tensor_constants(self.lr if lr is None else lr, BETAS, EPS, self.wd, self.t)
        self.p, self.m, self.v = sp.step(T, self.p, self.g, self.m, self.v, rows=rows, mask=mask)

    def check(self, opt, what):
        torch.cuda.synchronize()
        st = opt.state[self.param]
        assert float(st["step"]) == self.t, (what, float(st["step"]), self.t)
        for name, got, want in (("param", self.param.detach(), self.p), ("exp_avg", st["exp_avg"], self.m),
                                ("exp_avg_sq", st["exp_avg_sq"], self.v)):
            assert tuple(got.shape) == self.shape, (what, name)
            sp.assert_same_bits(got.cpu().numpy().reshape(want.shape), want, f"{what}: {name} {self.shape}")


def _opt(twins, **kw):
    from hgs.optim import Adam
    return Adam([dict(params=[t.param], lr=t.lr, weight_decay=t.wd, name=str(i)) for i, t in enumerate(twins)], lr=0.0,
                betas=BETAS, eps=EPS, **kw)


def _model(gpu, P, seed, n=6):
    shapes = ((P, 3), (P, 1, 3), (P, 15, 3), (P, 1), (P, 3), (P, 4), (P,), (P, 7), (P, 2, 2), (P, 5))[:n]
    return [Twin(gpu, s, lr=10.0 ** -(1 + i % 4) * (1 + i), seed=seed + i, wd=(0.0, 0.01)[i % 2])
            for i, s in enumerate(shapes)]


def test_ten_parameters_take_a_chunk_of_eight_and_one_of_two(gpu):
    from hgs import _lib
    assert _lib.ADAM_MAX_TENSORS == 8
    P = 70
    twins = _model(gpu, P, seed=10, n=10)
    opt = _opt(twins)
    rows = np.random.default_rng(1).permutation(P)[:31]
    mask = twins[3].g.reshape(-1)
    for what, kw, call in (("dense", {}, lambda: opt.step(None)),
                           ("list", dict(rows=rows), lambda: opt.step(torch.from_numpy(rows).to(gpu))),
                           ("mask", dict(mask=mask), lambda: opt.step_masked(twins[3].param.grad))):
        call()
        for i, t in enumerate(twins):
            t.expect(**kw)
            t.check(opt, f"{what}, parameter {i} of 10")


def test_two_row_counts_in_one_optimizer(gpu):
    """A model of P rows plus a table of 7 in one optimizer, as _launch defines it: step(None) steps every group;
    step(relevant) hands the SAME list to every row count (so every index must be inside the smallest); step_masked
    raises on the group whose row count is not the mask's length -- after the parameters of the matching row count, listed
    before it, were stepped, and with every step count already advanced."""
    P = 40
    a, b = Twin(gpu, (P, 3), 1e-2, seed=1), Twin(gpu, (7, 3), 1e-3, seed=2)
    opt = _opt([a, b])
    opt.step(None)
    for t in (a, b):
        t.expect()
        t.check(opt, "dense, two row counts")
    rows = np.array([6, 0, 3])
    opt.step(torch.from_numpy(rows).to(gpu))
    for t in (a, b):
        t.expect(rows=rows)
        t.check(opt, "one list for both row counts")
    mask = np.zeros(P, np.float32)
    mask[::3] = 1
    with pytest.raises(RuntimeError, match="row mask has 40 entries, parameter has 7 rows"):
        opt.step_masked(torch.from_numpy(mask).to(gpu))
    a.expect(mask=mask)
    a.check(opt, "masked, the matching row count")
    b.t += 1                                                     # counted, not stepped
    b.check(opt, "masked, the other row count")


def test_a_parameter_without_a_gradient_is_left_alone(gpu):
    twins = _model(gpu, 33, seed=20, n=3)
    opt = _opt(twins)
    opt.step(None)
    for t in twins:
        t.expect()
    idle = twins[1]
    for t in twins:
        t.new_grad()
    idle.param.grad = None
    opt.step(None)
    twins[0].expect(), twins[2].expect()
    for i, t in enumerate(twins):
        t.check(opt, f"parameter {i}, the second has no gradient")        # idle: same bits, step still 1
    # and one that never had a gradient gets no state at all
    fresh = _model(gpu, 33, seed=30, n=2)
    fresh[0].param.grad = None
    opt2 = _opt(fresh)
    opt2.step_masked(fresh[1].param.grad[:, 0, 0].contiguous())
    fresh[1].expect(mask=fresh[1].g[:, 0])
    fresh[1].check(opt2, "the stepped one")
    assert len(opt2.state[fresh[0].param]) == 0
    assert np.array_equal(fresh[0].param.detach().cpu().numpy().view(np.uint32), fresh[0].p.view(np.uint32))


def test_a_learning_rate_changed_between_steps_is_used(gpu):
    twins = _model(gpu, 50, seed=40, n=6)
    opt = _opt(twins)
    opt.step(None)
    for t in twins:
        t.expect()
    for group in opt.param_groups:                               # as update_learning_rate does
        if group["name"] == "0":
            group["lr"] = 3.3e-5
    twins[0].lr = 3.3e-5
    for t in twins:
        t.new_grad()
    opt.step(None)
    for i, t in enumerate(twins):
        t.expect()
        t.check(opt, f"parameter {i} after the change of lr")


def test_a_gradient_that_is_a_transposed_view(gpu):
    t = Twin(gpu, (37, 3), 1e-2, seed=50)
    view = torch.from_numpy(np.ascontiguousarray(t.g.T)).to(gpu).t()
    assert not view.is_contiguous() and tuple(view.shape) == (37, 3)
    t.param.grad = view
    opt = _opt([t])
    rows = np.array([36, 2, 17])
    opt.step(torch.from_numpy(rows).to(gpu))
    t.expect(rows=rows)
    t.check(opt, "transposed gradient")
    assert np.array_equal(view.cpu().numpy().view(np.uint32), t.g.view(np.uint32))


def test_relevant_as_int32_as_a_column_and_empty(gpu):
    twins = _model(gpu, 45, seed=60, n=6)
    opt = _opt(twins)
    rows = np.array([44, 0, 9, 10, 31])
    for what, rel, kw in (("int32", torch.from_numpy(rows.astype(np.int32)).to(gpu), dict(rows=rows)),
                          ("[n, 1]", torch.from_numpy(rows[::-1].copy()).to(gpu).reshape(-1, 1), dict(rows=rows[::-1])),
                          ("empty means dense", torch.empty(0, dtype=torch.int64, device=gpu), {}),
                          ("empty on the host means dense", torch.empty(0), {})):
        opt.step(rel)
        for i, t in enumerate(twins):
            t.expect(**kw)
            t.check(opt, f"relevant {what}, parameter {i}")
            t.new_grad()


def test_a_masked_step_in_two_parts_is_one_masked_step(gpu):
    P = 61
    parts, whole = _model(gpu, P, seed=70), _model(gpu, P, seed=70)
    opt_p, opt_w = _opt(parts), _opt(whole)
    for it in range(2):
        g = parts[3].param.grad
        opt_p.step_masked(g, params=[t.param for t in parts[:2]])
        opt_p.step_masked(g, params=[t.param for t in parts[2:]])
        opt_w.step_masked(whole[3].param.grad)
        mask = parts[3].g.reshape(-1)
        for i, (a, b) in enumerate(zip(parts, whole)):
            a.expect(mask=mask)
            a.check(opt_p, f"in two parts, step {it + 1}, parameter {i}")        # (every step advanced exactly once)
            b.expect(mask=mask)
            b.check(opt_w, f"in one part, step {it + 1}, parameter {i}")
            sa, sb = opt_p.state[a.param], opt_w.state[b.param]
            for x, y in ((a.param, b.param), (sa["exp_avg"], sb["exp_avg"]), (sa["exp_avg_sq"], sb["exp_avg_sq"])):
                assert torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32))
            a.new_grad(), b.new_grad()


def test_a_scalar_and_a_vector_parameter(gpu):
    s, v = Twin(gpu, (), 1e-2, seed=80), Twin(gpu, (300,), 1e-3, seed=81, wd=0.01)
    opt = _opt([s, v])
    for it in range(3):
        opt.step(None)
        for t in (s, v):
            t.expect()
            t.check(opt, f"step {it + 1}")
            t.new_grad()


def test_state_replaced_by_larger_tensors_keeps_its_step(gpu):
    """As densification does (scene/gaussian_model.py: cat_tensors_to_optimizer): a longer parameter takes the group's
    place, its moments are the old ones with zero rows appended, and the stored step count goes on."""
    P, extra = 30, 11
    t = Twin(gpu, (P, 3), 1e-2, seed=90)
    opt = _opt([t])
    for _ in range(2):
        opt.step(None)
        t.expect()
        t.new_grad()
    t.check(opt, "before the growth")
    stored = opt.state.pop(t.param)
    new_rows = sp.edge_inputs(t.rng, (extra, 3), planted=())[1]
    t.p = np.concatenate([t.p, new_rows])
    t.m, t.v = (np.concatenate([x, np.zeros((extra, 3), np.float32)]) for x in (t.m, t.v))
    t.shape = (P + extra, 3)
    t.param = torch.nn.Parameter(torch.from_numpy(t.p.copy()).to(gpu))
    stored["exp_avg"] = torch.from_numpy(t.m.copy()).to(gpu)
    stored["exp_avg_sq"] = torch.from_numpy(t.v.copy()).to(gpu)
    opt.param_groups[0]["params"][0] = t.param
    opt.state[t.param] = stored
    t.new_grad()
    opt.step(None)
    t.expect()
    assert t.t == 3
    t.check(opt, "after the growth")
