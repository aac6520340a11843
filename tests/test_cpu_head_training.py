"""CPU: the float64 restatement of the heads in training mode (tests/heads_f64.py) pinned against the real reference's results
(tests/golden/g30_head_training.npz; the reference's head modules run in float64 there, tools/make_golden_heads.py says why) at 1e-5 of each
tensor's scale — the bar tests/test_cpu_losses.py uses —
the ReLU floor of every end-to-end case table the GPU tests use, and the host side of xpoint_amd.training (imports without a GPU, the
reference's names, the refusals that need no device)."""
import os

import numpy as np
import pytest
import torch

from tests import heads_f64 as Hd

TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g30_head_training.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _close(got, ref, what, tol=TOL, scale=None):
    got, ref = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, sc = float((got - ref).abs().max()), float(ref.abs().max()) if scale is None else scale
    print(f"{what}: err / scale = {err / max(sc, 1e-30):.3e}")
    assert err <= tol * max(sc, 1e-30), (what, err, sc)


@pytest.mark.parametrize("case", Hd.CASES)
def test_case_meets_relu_floor(case, golden):
    """The fairness floor of the end-to-end table: asserted on the seed the golden file was written with, which is the seed the GPU tests use."""
    seed, _, ref = Hd.case_reference(case)
    assert seed == int(golden[f"{case}/seed"])
    margin = Hd.relu_margin(ref["pre"])
    print(f"{case}: seed {seed}, min |pre| / max |pre| = {margin:.3e} over {ref['pre'].numel()} trunk outputs")
    assert margin >= Hd.RELU_FLOOR
    assert ref["pre"].numel() <= 1.4e5          # the size up to which one of eight seeds meets the floor


@pytest.mark.parametrize("case", Hd.CASES)
def test_restatement_matches_reference(case, golden):
    _, _, ref = Hd.case_reference(case)
    keys = [k[len(case) + 1:] for k in golden.files if k.startswith(case + "/") and not k.endswith("/seed")]
    assert len(keys) == 2 + 16 + 12, keys             # outputs, 16 parameter gradients, 4 BatchNorms x 3 buffers
    for k in keys:
        got = ref[k]
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(golden[f"{case}/{k}"]) == 1
            continue
        _close(Hd.golden_view(k, got), golden[f"{case}/{k}"], f"{case}/{k}", scale=Hd.tensor_scale(ref, k))


def test_training_module_host_side():
    from xpoint_amd import _lib, training
    heads = training.XPointHeads(in_channels=48, descriptor_size=256)
    assert list(heads.state_dict()) == list(Hd.head_state("vmamba"))          # the reference's names, in its order
    for k, v in Hd.head_state("vmamba").items():
        assert tuple(heads.state_dict()[k].shape) == tuple(v.shape), k
    conv = training.XPointHeads(in_channels=128, descriptor_size=64)
    assert [tuple(v.shape) for v in conv.state_dict().values()] == [tuple(v.shape) for v in Hd.head_state("conv").values()]
    heads.load_state_dict(Hd.head_state("vmamba"))
    assert torch.equal(heads.t(Hd.DSC + "5.running_var"), Hd.head_state("vmamba")[Hd.DSC + "5.running_var"])
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        heads(torch.zeros(1, 2, 2, 48))
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        training.gemm_tn(torch.zeros(4, 3), torch.zeros(4, 5))
    sources = sorted(f for f in os.listdir(os.path.dirname(training.__file__)) if f.endswith(".py"))
    assert {"__init__.py", "ops.py", "heads.py", "regnet.py", "vss.py"} <= set(sources)
    for f in sources:          # every file of the package
        assert "oracle" not in open(os.path.join(os.path.dirname(training.__file__), f)).read().replace("no import of oracle", ""), f


def test_new_exports_are_bound():
    from xpoint_amd import _lib
    names = set(_lib._SIGNATURES) | set(_lib._SIZE_QUERIES)
    for n in ("xp_gemm_tn_h2", "xp_gemm_tn_h2_workspace_bytes", "xp_conv3x3_wgrad_h2", "xp_bn_workspace_bytes", "xp_bn_train_fwd", "xp_bn_train_bwd",
              "xp_colsum_rows", "xp_l2norm_rows_bwd"):
        assert n in names and n in _lib.exported_symbols(), n
