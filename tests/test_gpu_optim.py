"""GPU: xpoint_amd.training.Adam (csrc/optim.hip) against the float64 restatement tests/optim_f64.py — parity of parameters,
both moments and the gradient norm, determinism, independence of a tensor's result from its place and alignment, the device-side guard against
non-finite gradients, clipping, and train_step with it against the same steps with torch.optim.Adam.

Bar: max |got - ref| <= TOL x the largest magnitude of each tensor, TOL = STEPS x 8 x 2^-24 = 2.4e-6: an element of p, m or v takes at most eight
float32 roundings of quantities no larger than the tensor's largest per step (m: the two products and the sum on top of the three of g'; v: four on
top of them; p: its own subtraction, the update being lr-small next to it), and the errors of STEPS steps add.  Every comparison prints err / scale."""
import numpy as np
import pytest
import torch

from tests import optim_f64 as O
from tests.training_cases import AUG_CFG, LOSS_CFG, TOL as MODEL_TOL, _bits

pytestmark = pytest.mark.gpu

TOL = O.STEPS * 8 * 2.0 ** -24
assert TOL < 1e-4          # never looser than the project's f32 bar

# the shared set: the nine sizes, then 300 tensors of 7.  Tensor NONE never gets a gradient; tensor STRIDED is (65, 63) with a transposed
# (non-contiguous) gradient; tensor OFFSET is a view one float into its storage (a parameter off the 16-byte grid)
SIZES = O.SIZES + (O.MANY[1],) * O.MANY[0]
NONE, STRIDED, OFFSET = 4, 5, 3
assert SIZES[NONE] == 65 and SIZES[STRIDED] == 4095 and SIZES[OFFSET] == 5


@pytest.fixture(scope="module")
def shared():
    return O.case(SIZES)


def _params(params, only=None):
    out = []
    for i, p in enumerate(params):
        if only is not None and i not in only:
            continue
        t = torch.from_numpy(p.copy()).cuda()
        if i == STRIDED:
            t = t.view(65, 63)
        if i == OFFSET:
            base = torch.zeros(p.size + 1, device="cuda")
            base[1:] = t
            t = base[1:]
            assert t.data_ptr() % 16 == 4
        out.append(torch.nn.Parameter(t))
    return out


def _set_grads(ps, step_grads, only=None, poison=None):
    """poison = (tensor index, element, value): one non-finite element in one gradient"""
    idx = list(range(len(step_grads))) if only is None else sorted(only)
    for p, i in zip(ps, idx):
        if i == NONE:
            p.grad = None
            continue
        g = step_grads[i].copy()
        if poison is not None and poison[0] == i:
            g[poison[1]] = poison[2]
        t = torch.from_numpy(g).cuda()
        p.grad = t.view(63, 65).t() if i == STRIDED else t.view_as(p)
        if i == STRIDED:                                   # the same VALUES in the parameter's order, for the restatement
            assert not p.grad.is_contiguous()


def _ref_grads(step_grads, poison=None):
    out = []
    for i, g in enumerate(step_grads):
        if i == NONE:
            out.append(None)
            continue
        g = g.copy()
        if poison is not None and poison[0] == i:
            g[poison[1]] = poison[2]
        out.append(g.reshape(63, 65).T.reshape(-1) if i == STRIDED else g)
    return out


def _state(opt, ps):
    return [(p.detach().clone().reshape(-1), opt.state[p]["exp_avg"].clone().reshape(-1), opt.state[p]["exp_avg_sq"].clone().reshape(-1)) for p in ps]


def _close(got, ref, what, tol=TOL):
    got, ref = got.detach().cpu().double().numpy(), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert err <= tol * max(scale, 1e-30), (what, err, scale)
    return err / max(scale, 1e-300)


def _compare(state, ref, what, only=None):
    idx = list(range(len(ref.p))) if only is None else sorted(only)
    worst = 0.0
    for (p, m, v), i in zip(state, idx):
        for name, got, want in (("p", p, ref.p[i]), ("exp_avg", m, ref.m[i]), ("exp_avg_sq", v, ref.v[i])):
            worst = max(worst, _close(got, want, f"{what}: tensor {i} ({SIZES[i]} elements) {name}"))
    print(f"{what}: worst err / scale = {worst:.2e} (bound {TOL:.2e})")


def _run(shared, steps=O.STEPS, only=None, **kw):
    from xpoint_amd import training as T
    params, grads = shared
    ps = _params(params, only)
    opt = T.Adam(ps, **kw)
    for s in range(steps):
        _set_grads(ps, grads[s], only)
        opt.step()
    return ps, opt


@pytest.mark.parametrize("weight_decay", [0.0, 5e-4])
def test_parity_with_the_restatement(gpu_lib, shared, weight_decay):
    params, grads = shared
    ref = O.AdamF64(params, lr=1e-3, weight_decay=weight_decay)
    for s in range(O.STEPS):
        assert ref.step(_ref_grads(grads[s]))
    ps, opt = _run(shared, lr=1e-3, weight_decay=weight_decay)
    last = opt.last_step()
    assert last["step"] == O.STEPS and not last["skipped"] and last["skipped_steps"] == 0
    rel = abs(last["grad_norm"] - ref.grad_norm) / ref.grad_norm
    print(f"grad_norm {last['grad_norm']!r} vs {ref.grad_norm!r}: rel {rel:.2e}")
    assert rel <= 1e-12          # f64 sums of exact squares, some two thousand terms per lane and slot: a few ulp of f64
    _compare(_state(opt, ps), ref, f"weight_decay {weight_decay}")
    # the tensor without a gradient is left out, as torch leaves it: parameter untouched, moments zero
    assert torch.equal(ps[NONE].detach().cpu(), torch.from_numpy(params[NONE])) and not bool(opt.state[ps[NONE]]["exp_avg_sq"].any())


def test_two_runs_are_bit_identical_and_a_tensor_does_not_depend_on_its_place(gpu_lib, shared):
    a_ps, a = _run(shared, steps=3, lr=1e-3, weight_decay=5e-4)
    b_ps, b = _run(shared, steps=3, lr=1e-3, weight_decay=5e-4)
    for x, y in zip(_state(a, a_ps), _state(b, b_ps)):
        assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(x, y))
    assert a.last_step() == b.last_step()
    # alone, a tensor sits at flat offset 0 of a one-entry table; among the 309 it sits at another offset, in another table, after odd-sized tensors
    offsets = set()
    for i in (0, OFFSET, STRIDED, 7, 8, 9, 9 + 130, len(SIZES) - 1):
        one_ps, one = _run(shared, steps=3, only={i}, lr=1e-3, weight_decay=5e-4)
        offsets.add(a._offsets[i] % 4)
        for u, v in zip(_state(one, one_ps)[0], _state(a, a_ps)[i]):
            assert torch.equal(_bits(u), _bits(v)), f"tensor {i}: stepped alone it differs from stepped among {len(SIZES)}"
    assert offsets == {0, 1, 2, 3}, offsets          # every alignment of the moment views took part


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_the_guard_skips_a_nonfinite_step(gpu_lib, shared, value):
    params, grads = shared
    poison = (9 + 77, 3, value)          # one element of one of the 300 small tensors
    ref = O.AdamF64(params, lr=1e-3, weight_decay=5e-4)
    ps, opt = _run(shared, steps=2, lr=1e-3, weight_decay=5e-4)
    for s in range(2):
        ref.step(_ref_grads(grads[s]))
    before = [[_bits(t).clone() for t in st] for st in _state(opt, ps)]
    flat = (_bits(opt._exp_avg).clone(), _bits(opt._exp_avg_sq).clone())
    _set_grads(ps, grads[2], poison=poison)
    opt.step()
    assert not ref.step(_ref_grads(grads[2], poison=poison))
    last = opt.last_step()
    assert last["skipped"] and last["step"] == 2 and last["skipped_steps"] == 1 and not np.isfinite(last["grad_norm"])
    for i, (st, was) in enumerate(zip(_state(opt, ps), before)):
        assert all(torch.equal(_bits(u), w) for u, w in zip(st, was)), f"tensor {i} changed under a skipped step"
    assert torch.equal(_bits(opt._exp_avg), flat[0]) and torch.equal(_bits(opt._exp_avg_sq), flat[1])
    # the next finite step is the restatement's step 3, not step 4
    _set_grads(ps, grads[2])
    opt.step()
    assert ref.step(_ref_grads(grads[2])) and ref.t == 3
    last = opt.last_step()
    assert not last["skipped"] and last["step"] == 3 and last["skipped_steps"] == 1
    _compare(_state(opt, ps), ref, f"the step after a skipped one ({value})")
    late = O.AdamF64(params, lr=1e-3, weight_decay=5e-4)          # what a counter that had advanced would give: outside the bar
    for s in (0, 1):
        late.step(_ref_grads(grads[s]))
    late.t += 1
    late.step(_ref_grads(grads[2]))
    assert float(np.abs(late.p[8] - ref.p[8]).max()) > 10 * TOL * float(np.abs(ref.p[8]).max())


def test_without_the_guard_the_update_is_applied(gpu_lib, shared):
    params, grads = shared
    ps, opt = _run(shared, steps=1, lr=1e-3, skip_nonfinite=False)
    _set_grads(ps, grads[1], poison=(7, 100, float("nan")))
    opt.step()
    last = opt.last_step()
    assert not last["skipped"] and last["step"] == 2 and last["skipped_steps"] == 0
    assert bool(torch.isnan(ps[7].detach().reshape(-1)[100])) and bool(torch.isnan(opt.state[ps[7]]["exp_avg"].reshape(-1)[100]))


@pytest.mark.parametrize("max_norm", [0.05, 1e3])          # below the norm of the set's gradients (about 8.7) and above it
def test_clipping(gpu_lib, shared, max_norm):
    params, grads = shared
    ref = O.AdamF64(params, lr=1e-3, weight_decay=5e-4, max_norm=max_norm)
    for s in range(2):
        ref.step(_ref_grads(grads[s]))
    assert (ref.grad_norm > max_norm) == (max_norm < 1.0)
    ps, opt = _run(shared, steps=2, lr=1e-3, weight_decay=5e-4, max_norm=max_norm)
    assert abs(opt.last_step()["grad_norm"] - ref.grad_norm) <= 1e-12 * ref.grad_norm
    _compare(_state(opt, ps), ref, f"max_norm {max_norm}")
    if max_norm > 1.0:          # the coefficient is exactly 1: the bits of the run without clipping
        off_ps, off = _run(shared, steps=2, lr=1e-3, weight_decay=5e-4)
        for x, y in zip(_state(opt, ps), _state(off, off_ps)):
            assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(x, y))


def test_train_step_with_training_adam(gpu_lib):
    """three train_steps of the whole model (tests/xpoint_train_f64.py's case) with training.Adam: the loss follows the same steps with
    torch.optim.Adam within the model's bar, and two runs are bit-identical"""
    from tests import xpoint_train_f64 as Xp
    from tests.test_gpu_xpoint_training import _model, _pair_batch
    from xpoint_amd import losses, training as T
    data = _pair_batch(2, 64, 96, AUG_CFG)
    loss_fn = losses.XPointLoss(LOSS_CFG)

    def run(make):
        model = _model()
        optimizer = make(model.parameters())
        out = []
        for step in range(4):          # the fourth loss is the loss AFTER three steps
            torch.manual_seed(3)
            loss, _ = T.train_step(model, data, loss_fn, optimizer, seed=step)
            out.append(loss)
        return torch.stack(out), [_bits(v.float()) for v in model.state_dict().values()], optimizer

    mine, state, opt = run(lambda p: T.Adam(p, lr=1e-4, weight_decay=5e-4))
    again, state2, _ = run(lambda p: T.Adam(p, lr=1e-4, weight_decay=5e-4))
    theirs, _, _ = run(lambda p: torch.optim.Adam(p, lr=1e-4, weight_decay=5e-4))
    assert opt.last_step()["step"] == 4 and opt.last_step()["skipped_steps"] == 0
    print("losses:", mine.tolist(), "torch.optim.Adam:", theirs.tolist())
    assert torch.equal(_bits(mine), _bits(again)) and all(torch.equal(a, b) for a, b in zip(state, state2))
    err = float((mine[3] - theirs[3]).abs()) / float(theirs[3].abs())
    print(f"loss after three steps: rel {err:.2e}")
    assert err <= MODEL_TOL and not torch.equal(mine[3], mine[0])
    assert Xp.CASE == "S"
