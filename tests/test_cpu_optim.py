"""CPU (-m "not gpu"): the float64 restatement of the optimiser step (tests/optim_f64.py) against torch.optim.Adam in float64 (what the reference's
train.py runs), with torch.nn.utils.clip_grad_norm_ in front when clipping; the new exports, the argument errors of the three entry points, the
state_dict exchange between training.Adam and torch.optim.Adam, the refusals of training.Adam / training.fit that need no GPU, and `cli train`'s
place in --help."""
import ctypes

import numpy as np
import pytest
import torch

from tests import optim_f64 as O
from xpoint_amd import _lib

RTOL = 1e-12


def _torch_run(params, grads, weight_decay, max_norm=None, lr=1e-3):
    ps = [torch.nn.Parameter(torch.from_numpy(np.asarray(p, np.float64).copy())) for p in params]
    opt = torch.optim.Adam(ps, lr=lr, weight_decay=weight_decay)
    norms = []
    for step in grads:
        for p, g in zip(ps, step):
            p.grad = None if g is None else torch.from_numpy(np.asarray(g, np.float64).copy())
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
    return ps, opt, norms


def _rel(got, ref):
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / max(np.abs(np.asarray(ref)).max(), 1e-300))


@pytest.mark.parametrize("weight_decay", [0.0, 5e-4])
def test_restatement_is_torch_adam_f64(weight_decay):
    params, grads = O.case()
    ps, opt, _ = _torch_run(params, grads, weight_decay)
    mine = O.AdamF64(params, lr=1e-3, weight_decay=weight_decay)
    for step in grads:
        assert mine.step(step)
    assert mine.t == O.STEPS
    for i, p in enumerate(ps):
        st = opt.state[p]
        for what, got, ref in (("p", mine.p[i], p.detach().numpy()), ("exp_avg", mine.m[i], st["exp_avg"].numpy()),
                               ("exp_avg_sq", mine.v[i], st["exp_avg_sq"].numpy())):
            assert _rel(got, ref) <= RTOL, (i, what, _rel(got, ref))


@pytest.mark.parametrize("max_norm", [0.05, 1e3])          # below the case's norm (about 8.3), and above it: the coefficient is exactly 1
def test_restatement_clip_is_clip_grad_norm(max_norm):
    params, grads = O.case()
    ps, opt, norms = _torch_run(params, grads, 5e-4, max_norm=max_norm)
    mine = O.AdamF64(params, lr=1e-3, weight_decay=5e-4, max_norm=max_norm)
    for step, norm in zip(grads, norms):
        mine.step(step)
        assert abs(mine.grad_norm - norm) <= RTOL * norm
        assert (mine.grad_norm > max_norm) == (max_norm < 1.0)
    for i, p in enumerate(ps):
        assert _rel(mine.p[i], p.detach().numpy()) <= RTOL and _rel(mine.v[i], opt.state[p]["exp_avg_sq"].numpy()) <= RTOL, i


def test_restatement_skips_a_nonfinite_step_and_leaves_out_absent_gradients():
    params, grads = O.case(sizes=(5, 3, 4), steps=2)
    a, b = O.AdamF64(params), O.AdamF64(params)
    bad = [g.copy() for g in grads[0]]
    bad[1][2] = np.inf
    assert not a.step(bad) and a.t == 0 and a.skipped == 1 and not np.isfinite(a.grad_norm)
    assert all(np.array_equal(x, np.asarray(y, np.float64)) for x, y in zip(a.p, params)) and not any(m.any() for m in a.m)
    a.step(grads[0]); b.step(grads[0])
    assert a.t == 1 and all(np.array_equal(x, y) for x, y in zip(a.p, b.p))
    b.step([grads[1][0], None, grads[1][2]])
    ps, opt, _ = _torch_run(params, [grads[0], [grads[1][0], None, grads[1][2]]], 0.0)
    assert all(_rel(x, p.detach().numpy()) <= RTOL for x, p in zip(b.p, ps))


def test_exports_declared_and_bound():
    names = set(_lib._SIGNATURES) | set(_lib._SIZE_QUERIES)
    for n in ("xp_optim_grad_sumsq", "xp_optim_step_header", "xp_optim_adam_apply", "xp_optim_workspace_bytes", "xp_optim_header_bytes"):
        assert n in names and n in _lib.exported_symbols(), n
    lib = _lib.load()
    assert lib.xp_version() == 100
    assert lib.xp_optim_header_bytes() == 64
    assert lib.xp_optim_workspace_bytes(0, 10) == 0 and lib.xp_optim_workspace_bytes(3, 0) == 0
    # an upper bound of one f64 per workgroup of 8192 elements: 300 tensors of 7, and the shared case
    assert lib.xp_optim_workspace_bytes(300, 2100) >= 300 * 8
    assert lib.xp_optim_workspace_bytes(len(O.SIZES), sum(O.SIZES)) >= 8 * sum((n + 8191) // 8192 for n in O.SIZES)
    from xpoint_amd import training
    for n in ("Adam", "fit"):
        assert n in training.__all__ and hasattr(training, n), n


def test_null_pointers_and_bad_counts_return_an_error():
    lib = _lib.load()
    parts = ctypes.c_int64(0)
    one = (ctypes.c_void_p * 1)(256)
    cnt, bad, off = (ctypes.c_int64 * 1)(4), (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(0)
    ws = ctypes.c_void_p(256)
    assert lib.xp_optim_grad_sumsq(None, cnt, 1, ws, 256, ctypes.byref(parts), None) < 0 and b"null" in lib.xp_last_error()
    assert lib.xp_optim_grad_sumsq(one, cnt, 1, None, 0, ctypes.byref(parts), None) < 0 and b"null" in lib.xp_last_error()
    assert lib.xp_optim_grad_sumsq(one, bad, 1, ws, 256, ctypes.byref(parts), None) < 0 and b"bad count" in lib.xp_last_error()
    assert lib.xp_optim_grad_sumsq(one, cnt, 0, ws, 256, ctypes.byref(parts), None) < 0
    assert lib.xp_optim_grad_sumsq(one, cnt, 1, ws, 4, ctypes.byref(parts), None) < 0 and b"workspace" in lib.xp_last_error()
    assert lib.xp_optim_step_header(None, 1, ws, 0.9, 0.999, 0.0, 1, None) < 0 and b"null" in lib.xp_last_error()
    assert lib.xp_optim_step_header(ws, 0, ws, 0.9, 0.999, 0.0, 1, None) < 0 and b"n_partials" in lib.xp_last_error()
    assert lib.xp_optim_step_header(ws, 1, ws, 1.0, 0.999, 0.0, 1, None) < 0 and b"betas" in lib.xp_last_error()
    with pytest.raises(_lib.XPointHipError, match="null"):
        _lib.call("xp_optim_adam_apply", None, one, off, cnt, 1, ws, ws, 4, ws, 1e-3, 0.0, 0.9, 0.999, 1e-8, None)
    with pytest.raises(_lib.XPointHipError, match="bad count"):
        _lib.call("xp_optim_adam_apply", one, one, off, bad, 1, ws, ws, 4, ws, 1e-3, 0.0, 0.9, 0.999, 1e-8, None)
    with pytest.raises(_lib.XPointHipError, match="leave the buffers"):          # moments [0, 4) in buffers of 3 elements
        _lib.call("xp_optim_adam_apply", one, one, off, cnt, 1, ws, ws, 3, ws, 1e-3, 0.0, 0.9, 0.999, 1e-8, None)


def test_cpu_parameters_are_refused():
    from xpoint_amd import training
    p = torch.nn.Parameter(torch.zeros(4))
    opt = training.Adam([p], lr=1e-3)
    p.grad = torch.ones(4)
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        opt.step()
    assert not bool(p.detach().any())
    with pytest.raises(ValueError, match="one parameter group"):
        training.Adam([{"params": [p]}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    with pytest.raises(TypeError, match="float32"):
        training.Adam([torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))])


def test_state_dict_exchange_with_torch_adam():
    """torch.optim.Adam's state loads into training.Adam and comes back: keys, shapes, values, the step counter, the group's hyperparameters"""
    from xpoint_amd import training
    shapes = [(3, 5), (7,), (2, 2, 4)]
    ps = [torch.nn.Parameter(torch.from_numpy(O.uniform(f"sd/{i}", int(np.prod(s))).reshape(s))) for i, s in enumerate(shapes)]
    theirs = torch.optim.Adam(ps, lr=3e-4, weight_decay=5e-4)
    for k in range(2):
        for i, p in enumerate(ps):
            p.grad = torch.from_numpy(O.uniform(f"sd/g{k}/{i}", p.numel()).reshape(p.shape))
        theirs.step()
    sd = theirs.state_dict()
    mine = training.Adam(ps, lr=1.0)
    assert mine.state_dict()["state"] == {}          # as torch: no state before the first step
    mine.load_state_dict(sd)
    assert mine.param_groups[0]["lr"] == 3e-4 and mine.param_groups[0]["weight_decay"] == 5e-4 and mine.param_groups[0]["max_norm"] is None
    assert mine.last_step()["step"] == 2
    back = mine.state_dict()
    assert set(back) == set(sd) and set(back["state"]) == set(sd["state"]) == {0, 1, 2}
    for i in sd["state"]:
        assert set(back["state"][i]) == set(sd["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(back["state"][i]["step"]) == 2.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert back["state"][i][k].shape == sd["state"][i][k].shape and torch.equal(back["state"][i][k], sd["state"][i][k]), (i, k)
    # the moments are views of the two flat buffers, in one piece
    assert mine._exp_avg.numel() == sum(p.numel() for p in ps)
    assert all(mine.state[p]["exp_avg"].untyped_storage().data_ptr() == mine._exp_avg.untyped_storage().data_ptr() for p in ps)
    again = torch.optim.Adam(ps, lr=1.0)
    again.load_state_dict(back)
    for p in ps:
        assert torch.equal(again.state[p]["exp_avg_sq"], theirs.state[p]["exp_avg_sq"]) and float(again.state[p]["step"]) == 2.0
    assert again.param_groups[0]["lr"] == 3e-4
    for i, p in enumerate(ps):          # and torch's optimiser steps on from the state it got back
        p.grad = torch.ones_like(p)
    again.step()
    # torch's lr_schedulers drive the group's lr unchanged
    sched = torch.optim.lr_scheduler.ExponentialLR(mine, gamma=0.5)
    sched.step()
    assert mine.param_groups[0]["lr"] == pytest.approx(1.5e-4)


def test_cli_help_mentions_train(capsys):
    from xpoint_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["--help"])
    h = capsys.readouterr().out
    assert "train" in h and "--weight-file" in h and "e<N>.optim" in h
    assert "export" in h and "--chunk" in h and "HDF5" in h and "labels.npz" in h


def _fit_config(tmp_path, **model_over):
    from xpoint_amd import synth
    mcfg = synth.xpoint_exp1_config(64, 96, vssm={"EMBED_DIM": 32, "DEPTHS": [1, 1, 1, 1]})
    mcfg["mixed_precision"] = False          # the inference configuration ships with it on
    mcfg.update(model_over)
    return {"model": mcfg, "loss": {}, "dataset": {"foldername": str(tmp_path / "none")},
            "training": {"output_directory": str(tmp_path / "out"), "n_epochs": 1, "learningrate": 1e-4, "weight_decay": 0.0, "batchsize": 2,
                         "save_every_n_epoch": 1, "mixed_precision": False, "use_writer": False, "scheduler": {"use_scheduler": False},
                         "validation": {"compute_validation_loss": False}}}


def test_fit_refusals(tmp_path):
    from xpoint_amd import training
    cfg = _fit_config(tmp_path)
    cfg["training"]["mixed_precision"] = True
    with pytest.raises(NotImplementedError, match="mixed_precision.*is not built"):
        training.fit(cfg)
    cfg = _fit_config(tmp_path, mixed_precision=True)
    with pytest.raises(NotImplementedError, match="mixed_precision.*is not built"):
        training.fit(cfg)
    cfg = _fit_config(tmp_path)
    cfg["model"]["use_attention"]["check"] = False
    with pytest.raises(NotImplementedError, match="conv-encoder training is not built"):
        training.fit(cfg)
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        training.fit(_fit_config(tmp_path), device="cpu")
    assert not (tmp_path / "out").exists()          # a refused run writes nothing
