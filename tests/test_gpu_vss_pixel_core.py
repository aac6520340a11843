"""GPU: the wiring of the pixel-layout SS2D core into training — VSSBlock with ss2d_core = "pixel" against the float64 restatement
and the real reference's results, determinism under stochastic depth, one XPointNet train_step and a short training.fit under "pixel", the default
setting's launches, and the memory the form saves.  Bar: max |got - ref| <= 1e-4 x the scale of each tensor; every comparison prints err / scale."""
import copy

import pytest
import torch

from tests import vss_f64 as V, xpoint_train_f64 as Xp
from tests.training_cases import AUG_CFG, LOSS_CFG, _bits, _close
from xpoint_amd import synth

pytestmark = pytest.mark.gpu
KEYS = ["out", "grad/x"] + ["grad/" + k for k in V.LEAVES]
NEW = ("xp_ss2d_train_fwd", "xp_ss2d_train_bwd")


def _block(case, core, drop_path=0.0):
    from xpoint_amd import training as T
    (_, _, _, C), R, _, stage = V.CASES[case]
    blk = T.VSSBlock(C, dt_rank=R, drop_path=drop_path, stage=stage, block=0)
    blk.load_state_dict({V.prefix(case) + k: v for k, v in V.block_state(case, torch.float32).items()})
    return T.set_ss2d_core(blk, core).cuda().train()


def _step(blk, x, Rw, **kw):
    blk.zero_grad(set_to_none=True)
    x = x.detach().cuda().clone().requires_grad_(True)
    out = blk(x, **kw)
    (out * Rw.cuda()).sum().backward()
    res = {"out": out.detach(), "grad/x": x.grad}
    res.update({"grad/" + k: blk.t(k).grad for k in V.LEAVES})
    return res


@pytest.fixture
def calls(monkeypatch):
    """The names of the library calls made while the fixture lives"""
    from xpoint_amd import _lib
    seen, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    return seen


@pytest.mark.parametrize("case", list(V.CASES))
def test_block_step_pixel(gpu_lib, case, calls):
    x, Rw = V.case_inputs(case)
    got = _step(_block(case, "pixel"), x, Rw)
    assert calls.count(NEW[0]) == 1 and calls.count(NEW[1]) == 1 and "xp_cross_scan" not in calls and "xp_selective_scan_bwd_typed" not in calls
    ref = V.case_reference(case)
    for k in KEYS:
        assert got[k] is not None, k
        _close(got[k], ref[k], f"pixel {case}/{k} vs the restatement")
    if case in V.GOLDEN_CASES:
        golden = V.golden()
        for k in KEYS:
            _close(got[k], golden[f"{case}/{k}"], f"pixel {case}/{k} vs the reference")


def test_default_setting_launches_the_composition(gpu_lib, calls):
    x, Rw = V.case_inputs("A")
    blk = _block("A", "routes")
    assert blk.ss2d_core == "routes"
    _step(blk, x, Rw)
    assert not any(n.startswith("xp_ss2d_train") for n in calls), "the default path called the pixel-layout core"
    assert calls.count("xp_cross_scan") == 4 and calls.count("xp_cross_merge") == 4 and calls.count("xp_selective_scan_bwd_typed") == 1
    # eval forwards are the same under both settings: the same launches, the same bits
    a = blk.eval()(x.cuda())
    from xpoint_amd import training as T
    n = len(calls)
    b = T.set_ss2d_core(blk, "pixel").eval()(x.cuda())
    assert not any(m.startswith("xp_ss2d_train") for m in calls[n:]) and torch.equal(_bits(a), _bits(b))


def test_two_steps_with_stochastic_depth_are_bit_identical(gpu_lib):
    x, Rw = V.case_inputs("A")
    blk = _block("A", "pixel", drop_path=0.3)
    a = {k: v.clone() for k, v in _step(blk, x, Rw, seed=5).items()}
    b = _step(blk, x, Rw, seed=5)
    for k in KEYS:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_train_step_pixel_against_routes(gpu_lib, calls):
    """one XPointNet train_step at the smallest configuration of tests/test_gpu_xpoint_training.py, the same weights, data and seeds under both forms"""
    from tests.test_gpu_xpoint_training import _model, _pair_batch
    from xpoint_amd import losses, training as T
    data = _pair_batch(2, 64, 96, AUG_CFG)
    loss_fn = losses.XPointLoss(LOSS_CFG)
    res = {}
    for core in ("routes", "pixel"):
        model = T.set_ss2d_core(_model(drop_path_rate=0.2), core)
        torch.manual_seed(3)                                    # the detector loss draws its label noise from torch's generator
        n = len(calls)
        loss, _ = T.train_step(model, data, loss_fn, torch.optim.SGD(model.parameters(), lr=0.0), seed=5)
        assert (NEW[0] in calls[n:]) == (core == "pixel") and (NEW[1] in calls[n:]) == (core == "pixel")
        res[core] = (loss, {k: p.grad.clone() for k, p in model.named_parameters()})
    _close(res["pixel"][0], res["routes"][0], "train_step: loss, pixel vs routes")
    assert list(res["pixel"][1]) == list(res["routes"][1])
    routes = {"grad/" + k: g.cpu() for k, g in res["routes"][1].items()}
    for k, g in res["routes"][1].items():          # the heads' 3.bias / 4.bias gradients are zero in exact arithmetic: on their sibling weight's scale (Xp.tensor_scale)
        _close(res["pixel"][1][k], g, f"train_step: grad/{k}, pixel vs routes", scale=Xp.tensor_scale(routes, "grad/" + k))


def test_fit_with_the_pixel_core(gpu_lib, tmp_path, calls):
    import yaml
    from tests.test_gpu_fit import H, W, _folder
    from xpoint_amd import training as T
    folder, labels = _folder(tmp_path / "data", "train")
    mcfg = synth.xpoint_exp1_config(H, W, vssm={"EMBED_DIM": 32, "DEPTHS": [1, 1, 1, 1]})
    mcfg["mixed_precision"] = False
    torch.save(synth.make_torch_state_dict(mcfg), tmp_path / "start.model")
    cfg = {"model": mcfg, "loss": dict(LOSS_CFG, type="XPointLoss"),
           "dataset": {"type": "ImagePairDataset", "foldername": folder, "keypoints_filename": labels, "height": H, "width": W,
                       "augmentation": copy.deepcopy(AUG_CFG)},
           "training": {"output_directory": str(tmp_path / "out"), "n_epochs": 2, "learningrate": 1e-4, "batchsize": 2, "save_every_n_epoch": 0,
                        "ss2d_core": "pixel"}}
    h = T.fit(copy.deepcopy(cfg), weight_file=str(tmp_path / "start.model"), seed=3)
    assert h["epoch"] == [1, 2] and all(torch.isfinite(torch.tensor(h["loss"]))) and h["skipped_steps"] == [0, 0]
    assert yaml.safe_load(open(tmp_path / "out" / "params.yaml"))["training"]["ss2d_core"] == "pixel"
    assert calls.count(NEW[0]) == calls.count(NEW[1]) > 0
    cfg["training"].pop("ss2d_core")
    cfg["training"].update(output_directory=str(tmp_path / "default"), n_epochs=1)
    n = len(calls)
    T.fit(cfg, weight_file=str(tmp_path / "start.model"), seed=3)
    assert yaml.safe_load(open(tmp_path / "default" / "params.yaml"))["training"]["ss2d_core"] == "routes"
    assert not any(m.startswith("xp_ss2d_train") for m in calls[n:])


def test_peak_memory_falls_by_a_route_tensor(gpu_lib):
    """(2, 32, 32, 96): the composition keeps two (B, 4, C, L) route tensors for the backward (xs, dts); the pixel form keeps none (dtp is recomputed in
    the backward) and adds only the chunk states.  From the shapes: the peak of a block step falls by at least B 4 C L 4 bytes."""
    from xpoint_amd import training as T
    B, H, W, C = 2, 32, 32, 96
    x = torch.from_numpy(synth.uniform("vss_pixel/mem/x", (B, H, W, C), -1.0, 1.0)).cuda()
    blk = T.VSSBlock(C).cuda().train()
    peak = {}
    for core in ("routes", "pixel", "routes", "pixel"):          # twice: the second round runs on a warm allocator
        T.set_ss2d_core(blk, core)
        blk.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        xin = x.clone().requires_grad_(True)
        blk(xin).sum().backward()
        torch.cuda.synchronize()
        peak[core] = torch.cuda.max_memory_allocated() - base
        del xin
    route = B * 4 * C * H * W * 4
    print(f"peak over one block step: routes {peak['routes']} B, pixel {peak['pixel']} B, a route tensor {route} B")
    assert peak["routes"] - peak["pixel"] >= route
