"""CPU: the float64 restatement of the homography head in training mode (tests/regnet_f64.py) pinned against the real reference's results
(tests/golden/g31_regnet_training.npz; the reference's module runs in float64 there, tools/make_golden_regnet_training.py) at 1e-5 of each
tensor's scale — the bar tests/test_cpu_head_training.py uses — and the host side of xpoint_amd.training.RegNetHead: the reference's names, the
refusals that need no device, the new exports."""
import numpy as np
import pytest
import torch

from tests import regnet_f64 as Rg

TOL = 1e-5


def _close(got, ref, what, tol=TOL, scale=None):
    got, ref = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, sc = float((got - ref).abs().max()), float(ref.abs().max()) if scale is None else scale
    print(f"{what}: err / scale = {err / max(sc, 1e-30):.3e}")
    assert err <= tol * max(sc, 1e-30), (what, err, sc)


@pytest.mark.parametrize("case", Rg.CASES)
def test_restatement_matches_reference(case):
    golden = Rg.golden()
    _, (m1, m2), ref = Rg.case_reference(case)
    B = Rg.SHAPES[case][0]
    assert m1.shape == (B, 256) and m2.shape == (B, 64) and m1.dtype == torch.uint8 and 0.3 < float(m1.float().mean()) < 0.7
    keys = [k[len(case) + 1:] for k in golden.files if k.startswith(case + "/") and "/mask" not in k]
    assert len(keys) == 1 + 10 + 6, keys              # the output, 10 parameter gradients, 2 BatchNorms x 3 buffers
    for k in keys:
        got = ref[k]
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(golden[f"{case}/{k}"]) == 2          # layer1 runs once per image
            continue
        _close(Rg.golden_view(k, got), golden[f"{case}/{k}"], f"{case}/{k}", scale=Rg.tensor_scale(ref, k))


def test_imposed_gates_leave_the_forward_alone():
    """the restatement under its OWN decisions, imposed through `gates`, is the restatement: same values, same gradients"""
    case = Rg.CASES[0]
    (enc1, enc2, R), (m1, m2), ref = Rg.case_reference(case)
    own = [Rg.gates_of(ref["y1"][i], ref["y2"][i]) for i in range(2)]
    gates = {"relu1": [g[0] for g in own], "relu2": [g[1] for g in own], "pool": [g[2] for g in own]}
    res = Rg.regnet_f64(Rg.head_state(), enc1, enc2, m1, m2, R, gates=gates)
    assert torch.equal(res["hm"], ref["hm"])
    for k in ref:
        if k.startswith("grad/"):
            _close(res[k], ref[k], f"{case}/{k} under its own gates", tol=1e-12)
    # a flipped gate changes the gradient and nothing in the forward pass
    gates["relu1"][0] = ~gates["relu1"][0]
    flipped = Rg.regnet_f64(Rg.head_state(), enc1, enc2, m1, m2, R, gates=gates)
    assert torch.equal(flipped["hm"], ref["hm"]) and torch.equal(flipped[Rg.HM + "layer1.4.running_var"], ref[Rg.HM + "layer1.4.running_var"])
    assert not torch.allclose(flipped["grad/" + Rg.HM + "layer1.0.weight"], ref["grad/" + Rg.HM + "layer1.0.weight"], rtol=1e-3, atol=0.0)


def test_regnet_head_host_side():
    from xpoint_amd import _lib, synth, training
    head = training.RegNetHead()
    want = [(k, tuple(v.shape)) for k, v in synth.make_torch_state_dict(Rg.model_config()).items() if k.startswith(Rg.HM)]
    assert len(want) == 16
    assert [(k, tuple(v.shape)) for k, v in head.state_dict().items()] == want          # the reference's names, in its order
    head.load_state_dict(Rg.head_state())
    assert torch.equal(head.t(Rg.HM + "layer1.4.running_var"), Rg.head_state()[Rg.HM + "layer1.4.running_var"])
    for name in ("RegNetHead", "conv3x3_wgrad_zero_pad", "conv3x3_dgrad", "relu_bwd", "maxpool2_relu_bwd", "costvolume_mean_bwd", "dropout_rows"):
        assert name in training.__all__ and hasattr(training, name), name
    z = torch.zeros(1, 32, 32, 48)
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        head(z, z)
    head.eval()
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        head(z, z)
    for call in (lambda: training.conv3x3_wgrad_zero_pad(torch.zeros(1, 2, 2, 4), torch.zeros(1, 2, 2, 8)),
                 lambda: training.conv3x3_dgrad(torch.zeros(1, 2, 2, 8), torch.zeros(8, 3, 3, 4)),
                 lambda: training.relu_bwd(torch.zeros(4), torch.zeros(4)),
                 lambda: training.maxpool2_relu_bwd(torch.zeros(1, 1, 1, 4), torch.zeros(1, 2, 2, 4)),
                 lambda: training.costvolume_mean_bwd(torch.zeros(1, 5, 3), torch.zeros(1, 5, 3), torch.zeros(1, 5)),
                 lambda: training.dropout_rows(torch.zeros(2, 4))):
        with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
            call()

    class NoHead:
        def state_dict(self):
            return {"detector_head_convolutions.1.weight": torch.zeros(1)}
    with pytest.raises(RuntimeError, match="holds no"):
        training.RegNetHead.from_model(NoHead())


def test_new_exports_are_bound():
    from xpoint_amd import _lib
    names = set(_lib._SIGNATURES) | set(_lib._SIZE_QUERIES)
    for n in ("xp_conv3x3_zp_wgrad_h2", "xp_conv3x3_dgrad_h2", "xp_conv3x3_dgrad_h2_workspace_bytes", "xp_relu_fwd", "xp_relu_bwd", "xp_maxpool2_relu_bwd",
              "xp_costvolume_mean_bwd", "xp_dropout_rows"):
        assert n in names and n in _lib.exported_symbols(), n
