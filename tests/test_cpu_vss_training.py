"""CPU: the float64 restatement of a VSS encoder block (tests/vss_f64.py) pinned against the real reference's results
(tests/golden/g32_vss_training.npz; the reference's block runs as a float64 module there, tools/make_golden_vss_training.py) at 1e-5 of each tensor's
scale — the bar of tests/test_cpu_regnet_training.py — and by gradcheck; and the host side of xpoint_amd.training.VSSBlock: the reference's names,
shapes and order, the from_model / load_state_dict round trip, the refusals that need no device, the drop-path rate table, the new exports.

The reference's scan runs in float32 inside the float64 module, so a tensor behind it could miss 1e-5 through the reference's own rounding; measured,
none does: the largest disagreement over both fixture cases and all 20 tensors is 2.3e-7 of the tensor's scale (grad/op.dt_projs_weight, case B), so
every tensor keeps the 1e-5 bar and no widened bar is in use."""
import numpy as np
import pytest
import torch

from tests import vss_f64 as V

TOL = 1e-5


def _close(got, ref, what, tol=TOL):
    got, ref = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, sc = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: err / scale = {err / max(sc, 1e-30):.3e}")
    assert err <= tol * max(sc, 1e-30), (what, err, sc)


@pytest.mark.parametrize("case", V.GOLDEN_CASES)
def test_restatement_matches_reference(case):
    golden = V.golden()
    ref = V.case_reference(case)
    keys = [k[len(case) + 1:] for k in golden.files if k.startswith(case + "/")]
    assert sorted(keys) == sorted(["out", "grad/x"] + ["grad/" + k for k in V.LEAVES])          # the output, the input gradient, 18 parameter gradients
    for k in keys:
        assert float(np.abs(golden[f"{case}/{k}"]).max()) > 0.0, k
        _close(ref[k], golden[f"{case}/{k}"], f"{case}/{k}")


def _tiny_params(C=4, R=1, H4=8):
    u = lambda n, s, lo=-0.5, hi=0.5: torch.from_numpy(V.synth.uniform("vss/tiny/" + n, s, lo, hi)).double()          # noqa: E731
    return {"norm.weight": u("n1w", (C,), 0.8, 1.2), "norm.bias": u("n1b", (C,), -0.1, 0.1), "op.x_proj_weight": u("xp", (4, R + 2, C)),
            "op.A_logs": u("al", (4 * C, 1)), "op.Ds": u("ds", (4 * C,), 0.5, 1.5), "op.dt_projs_weight": u("dtw", (4, C, R), -1.0, 1.0),
            "op.dt_projs_bias": u("dtb", (4, C), -3.0, -1.0), "op.out_norm.weight": u("onw", (C,), 0.8, 1.2), "op.out_norm.bias": u("onb", (C,), -0.1, 0.1),
            "op.in_proj.weight": u("in", (C, C)), "op.conv2d.weight": u("cv", (C, 1, 3, 3)), "op.out_proj.weight": u("out", (C, C)),
            "norm2.weight": u("n2w", (C,), 0.8, 1.2), "norm2.bias": u("n2b", (C,), -0.1, 0.1), "mlp.fc1.weight": u("f1", (H4, C)),
            "mlp.fc1.bias": u("f1b", (H4,)), "mlp.fc2.weight": u("f2", (C, H4)), "mlp.fc2.bias": u("f2b", (C,))}


def test_restatement_gradcheck():
    """the analytic scan backward inside the restatement, and the composition around it, against finite differences — with per-sample factors"""
    p = _tiny_params()
    assert list(p) == list(V.LEAVES)
    x = torch.from_numpy(V.synth.uniform("vss/tiny/x", (2, 2, 3, 4), -1.0, 1.0)).double().requires_grad_(True)
    leaves = [p[k].requires_grad_(True) for k in V.LEAVES]
    s1, s2 = torch.tensor([1.25, 0.0], dtype=torch.float64), torch.tensor([0.5, 1.25], dtype=torch.float64)
    fn = lambda xx, *ps: V.vss_block64(dict(zip(V.LEAVES, ps)), xx, s1, s2)          # noqa: E731
    assert torch.autograd.gradcheck(fn, (x, *leaves), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_vss_block_host_side():
    from xpoint_amd import _lib, models, synth, training
    for case in ("A", "C"):
        (_, _, _, C), R, E, stage = V.CASES[case]
        cfg = V.model_config(E)
        pre = V.prefix(case)
        want = [(k, shape) for k, (shape, _) in synth.xpoint_state_spec(cfg).items() if k.startswith(pre)]
        assert len(want) == 18
        blk = training.VSSBlock(C, stage=stage, block=0)
        assert [(k, tuple(v.shape)) for k, v in blk.state_dict().items()] == want          # the reference's names and shapes, in its order
        assert blk.dt_rank == R and [k for k, _ in blk.named_parameters()] == [k for k, _ in want]
    # from_model / load_state_dict round trip
    cfg = V.model_config(32)
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    blk = training.VSSBlock.from_model(net, stage=1, block=0)
    assert blk.dim == 64 and blk.prefix == "encoder.layers.1.blocks.0."
    for k, v in blk.state_dict().items():
        assert torch.equal(v, net.state_dict()[k]), k
    with torch.no_grad():
        blk.t("op.Ds").add_(1.0)
    res = net.load_state_dict(blk.state_dict(), strict=False)
    assert list(res.unexpected_keys) == [] and len(res.missing_keys) == len(net.state_dict()) - 18
    assert torch.equal(net.state_dict()["encoder.layers.1.blocks.0.op.Ds"], blk.t("op.Ds").detach())
    with pytest.raises(RuntimeError, match="holds no"):
        training.VSSBlock.from_model(net, stage=0, block=1)
    # the multispectral prefixes
    ms = training.VSSBlock(32, encoder="encoder_thermal.")
    assert next(iter(ms.state_dict())) == "encoder_thermal.layers.0.blocks.0.norm.weight"
    with pytest.raises(ValueError):
        training.VSSBlock(32, encoder="backbone.")
    with pytest.raises(ValueError, match="multiple of 4"):
        training.VSSBlock(30)
    for name in ("VSSBlock", "layernorm_bwd", "dwconv3x3_silu_bwd", "gelu_fwd", "gelu_bwd", "add_scaled_rows", "scale_grad"):
        assert name in training.__all__ and hasattr(training, name), name


def test_no_cpu_fallback():
    from xpoint_amd import _lib, training
    blk = training.VSSBlock(32)
    z = torch.zeros(1, 2, 3, 32)
    for mode in (blk.train, blk.eval):
        mode()
        with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
            blk(z)
    for call in (lambda: training.layernorm_bwd(torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(8)),
                 lambda: training.dwconv3x3_silu_bwd(torch.zeros(1, 2, 2, 4), torch.zeros(9, 4), torch.zeros(1, 2, 2, 4)),
                 lambda: training.gelu_fwd(torch.zeros(5)),
                 lambda: training.gelu_bwd(torch.zeros(5), torch.zeros(5)),
                 lambda: training.add_scaled_rows(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4), torch.zeros(2)),
                 lambda: training.add_scaled_rows(None, torch.zeros(2, 3, 4), torch.zeros(2)),
                 lambda: training.scale_grad(torch.zeros(7))):
        with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
            call()


def test_drop_path_rate_table():
    """block i of sum(DEPTHS) gets linspace(0, DROP_PATH_RATE, sum(DEPTHS))[i] (VMamba.py:1289): DEPTHS [2, 2, 2, 2], rate 0.2"""
    from xpoint_amd import models, synth, training
    want = [0.2 * i / 7 for i in range(8)]
    assert training.drop_path_rates([2, 2, 2, 2], 0.2) == pytest.approx(want, abs=1e-7)
    cfg = synth.xpoint_exp1_config(256, 256, vssm={"EMBED_DIM": 32})
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    got = [training.VSSBlock.from_model(net, s, j).drop_path for s in range(4) for j in range(2)]
    assert got == pytest.approx(want, abs=1e-7) and got[0] == 0.0
    assert training.VSSBlock(32).drop_path == 0.0 and training.VSSBlock(32, drop_path=0.1).drop_path == 0.1
    with pytest.raises(ValueError):
        training.VSSBlock(32, drop_path=1.0)
    # host draws: keyed by (seed, sample id, branch), never by the position in the batch
    a = training.vss._drop_path_draws(0.5, 7, [0, 1, 2, 3, 4, 5, 6, 7], 0)
    b = training.vss._drop_path_draws(0.5, 7, [7, 6, 5, 4, 3, 2, 1, 0], 0)
    assert a == b[::-1] and set(a) == {0.0, 2.0}
    assert a != training.vss._drop_path_draws(0.5, 7, range(8), 1) or a != training.vss._drop_path_draws(0.5, 8, range(8), 0)


def test_new_exports_are_bound():
    from xpoint_amd import _lib
    names = set(_lib._SIGNATURES) | set(_lib._SIZE_QUERIES)
    for n in ("xp_layernorm_bwd", "xp_layernorm_bwd_workspace_bytes", "xp_dwconv3x3_silu_bwd", "xp_dwconv3x3_silu_bwd_workspace_bytes", "xp_gelu_fwd",
              "xp_gelu_bwd", "xp_add_scaled_rows", "xp_scale_grad", "xp_scale_grad_workspace_bytes"):
        assert n in names and n in _lib.exported_symbols(), n
    lib = _lib.load()
    assert lib.xp_scale_grad_workspace_bytes() == 4352 and lib.xp_layernorm_bwd_workspace_bytes(0, 32) == 0
    assert lib.xp_layernorm_bwd_workspace_bytes(35, 32) % 256 == 0 and lib.xp_dwconv3x3_silu_bwd_workspace_bytes(2, 5, 7, 32) >= 4352 + 2 * 5 * 7 * 32 * 4
