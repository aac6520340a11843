"""CPU: the float64 restatement of one training step of the whole VMamba XPoint (tests/xpoint_train_f64.py) pinned against the real reference's results
(tests/golden/g34_xpoint_training.npz; the reference runs as a float64 module there, tools/make_golden_xpoint_training.py) at 1e-5 of each tensor's
scale — the bar of tests/test_cpu_encoder_training.py —, the fold identity that xp_conv3x3_rp_dgrad_h2 computes against float64 autograd of
reflection pad + conv2d, and the host side of xpoint_amd.training.XPointNet: the new exports, the reference's names for a single-encoder and a
multispectral configuration, and the refusals that need no device.

Two tests here pin the TEST HELPERS, not the library, and so pass on a tree without the feature's library code: test_fold_identity (the arithmetic the
kernel implements, stated with torch) and test_heads_restatement_is_heads_f64 (the restated heads against heads_f64).  Every other test needs the
feature."""
import numpy as np
import pytest
import torch

from tests import encoder_f64 as En, heads_f64 as Hd, xpoint_train_f64 as Xp

TOL = 1e-5


def _close(got, ref, what, tol=TOL, scale=None):
    got, ref = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, sc = float((got - ref).abs().max()), float(ref.abs().max()) if scale is None else scale
    print(f"{what}: err / scale = {err / max(sc, 1e-30):.3e}")
    assert err <= tol * max(sc, 1e-30), (what, err, sc)
    return err / max(sc, 1e-30)


def _golden_part(name, t):
    """The part of the restatement's tensor `name` the golden file stores: strided head tensors, leading output channels of a large encoder gradient."""
    if name.startswith(("grad/" + Hd.DET, "grad/" + Hd.DSC, "desc/")):
        return Hd.golden_view(name.split("/")[0] if name.startswith("desc/") else name, t)
    return t


def test_restatement_matches_reference():
    golden = Xp.golden()
    ref = Xp.case_reference()
    assert int(golden["seed"]) == Xp.case_seed()
    keys = [k for k in golden.files if k != "seed"]
    heads = [k for k in Xp.model_state() if k.startswith((Hd.DET, Hd.DSC)) and Xp.is_parameter(k)]
    enc = [k for k in keys if k.startswith("grad/" + En.PRE)]
    assert sorted(keys) == sorted([f"{w}/{sp}" for w in ("logits", "desc", "denc") for sp in Xp.SPECTRA] + ["grad/" + k for k in heads] + enc)
    assert len(heads) == 16 and len(enc) == 68          # g33's 69 arrays without `out`
    worst = ("", 0.0)
    for k in keys:
        g = golden[k]
        assert float(np.abs(g).max()) > 0.0, k
        part = _golden_part(k, ref[k])
        e = _close(part[:g.shape[0]], g, k, scale=Xp.tensor_scale(ref, k) if k.startswith("grad/") else None)
        worst = max(worst, (k, e), key=lambda t: t[1])
    print(f"largest disagreement: {worst[0]} {worst[1]:.3e}")
    for sp in Xp.SPECTRA:
        margin = Hd.relu_margin(ref['pre/' + sp])
        print(f"seed {Xp.case_seed()}, ReLU margin {sp}: {margin:.3e}")
        assert margin >= Hd.RELU_FLOOR


def test_heads_restatement_is_heads_f64():
    """heads64 (on the caller's tensors, differentiable in the encoder output) against heads_f64.heads_f64 on one of its cases"""
    case = "vmamba/3x9x7"
    _, (enc, r1, r2), ref = Hd.case_reference(case)
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in Hd.head_state("vmamba").items() if Xp.is_parameter(k)}
    logits, desc, pre = Xp.heads64(p, enc.double())
    ((logits * r1.double()).sum() + (desc * r2.double()).sum()).backward()
    assert torch.equal(logits.detach(), ref["logits"]) and torch.equal(desc.detach(), ref["desc"]) and torch.equal(pre, ref["pre"])
    for k, v in p.items():
        assert torch.equal(v.grad, ref["grad/" + k]), k


@pytest.mark.parametrize("hw", Xp.FOLD_SHAPES)
def test_fold_identity(hw):
    """dx of the reflection-padded convolution = the zero-padded input gradient on the padded frame, its frame folded onto rows / columns 1 and n - 2"""
    H, W = hw
    u = lambda n, s: torch.from_numpy(En.synth.uniform(f"xpt/fold/{n}/{H}x{W}", s, -1.0, 1.0)).double()          # noqa: E731
    dy, w = u("dy", (2, 5, H, W)), u("w", (5, 3, 3, 3))
    want = Xp.reflect_dgrad_autograd(dy, w)
    got = Xp.reflect_dgrad_by_fold(dy, w)
    assert _close(got, want, f"fold identity {H}x{W}", tol=1e-13) <= 1e-13
    g = Xp.zero_pad_dgrad_on_frame(dy, w)
    inner = torch.nn.functional.conv2d(dy, w.flip(2, 3).transpose(0, 1), padding=1)          # the zero-padded convolution's own input gradient
    _close(g[:, :, 1:-1, 1:-1], inner, f"the frame's interior is the zero-padded input gradient {H}x{W}", tol=1e-13)
    if min(H, W) > 4:          # away from rows / columns 1 and n - 2 nothing is added
        assert torch.equal(got[:, :, 2:-2, 2:-2], g[:, :, 3:-3, 3:-3])
        assert torch.equal(got[:, :, 0, 2:-2], g[:, :, 1, 3:-3])


def test_new_symbols_are_declared_exported_and_bound():
    from xpoint_amd import _lib
    names = set(_lib._SIGNATURES) | set(_lib._SIZE_QUERIES)
    for n in ("xp_conv3x3_rp_dgrad_h2", "xp_conv3x3_rp_dgrad_h2_workspace_bytes"):
        assert n in names and n in _lib.exported_symbols(), n
    lib = _lib.load()
    assert lib.xp_version() == 100
    for bad in ((0, 4, 4, 8, 8), (1, 1, 4, 8, 8), (1, 4, 1, 8, 8)):          # reflection needs H, W >= 2
        assert lib.xp_conv3x3_rp_dgrad_h2_workspace_bytes(*bad) == 0
    # the zero-padded launch's workspace, then the frame's: the rearranged weight (Ci, 12 slices of 32 columns at Co = 32), its split, the three tap
    # planes of g on the frame
    up = lambda n: (n + 255) // 256 * 256          # noqa: E731
    want = lib.xp_conv3x3_dgrad_h2_workspace_bytes(2, 5, 7, 8, 32) + up(8 * 384 * 4) + up(lib.xp_split_weights_h2_bytes(8, 384)) + up(3 * 2 * (2 * 9 + 2 * 5) * 8 * 4)
    assert lib.xp_conv3x3_rp_dgrad_h2_workspace_bytes(2, 5, 7, 8, 32) == want


def test_new_names_are_exported():
    from xpoint_amd import training
    for name in ("conv3x3_dgrad_reflect", "XPointNet", "train_step"):
        assert name in training.__all__ and hasattr(training, name), name


def _net(**over):
    from xpoint_amd import models, synth
    cfg = Xp.model_config(**over)
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    return net


def _pair(n=2, flags=None):
    data = {sp: {"image": torch.zeros(n, 1, 64, 96)} for sp in Xp.SPECTRA}
    if flags is not None:
        for sp, f in zip(Xp.SPECTRA, flags):
            data[sp]["is_optical"] = torch.tensor(f).view(n, 1)
    return data


def test_cpu_tensors_are_refused():
    from xpoint_amd import _lib, training
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        training.conv3x3_dgrad_reflect(torch.zeros(1, 4, 4, 8), torch.zeros(8, 3, 3, 4))
    model = training.XPointNet.from_model(_net())
    for mode in (model.train, model.eval):
        mode()
        with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
            model(_pair())
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        training.train_step(model, _pair(), None, torch.optim.SGD(model.parameters(), lr=0.1))


@pytest.mark.parametrize("multispectral", [False, True])
def test_state_dict_names(multispectral):
    """the reference's checkpoint names: the model's state loads into the inference model with nothing unexpected, and every encoder / head tensor of
    the inference model is there"""
    from xpoint_amd import training
    net = _net(multispectral=multispectral)
    model = training.XPointNet.from_model(net)
    sd, want = model.state_dict(), net.state_dict()
    prefixes = ("encoder_thermal.", "encoder_optical.") if multispectral else ("encoder.",)
    assert {k.split(".")[0] + "." for k in sd} == set(prefixes) | {Hd.DET, Hd.DSC}
    assert [k for k in want if k not in sd] == [] and all(torch.equal(sd[k], want[k]) for k in want)
    assert [k for k in sd if k not in want and not k.endswith("num_batches_tracked")] == []
    assert [k for k, _ in model.named_parameters()] == [k for k in want if Xp.is_parameter(k) or k.startswith(prefixes)]
    assert len(list(model.parameters())) == len({id(p) for p in model.parameters()}) == (20 + 18 * 4) * len(prefixes) + 16
    r = net.load_state_dict(sd, strict=False)
    assert list(r.unexpected_keys) == [] and list(r.missing_keys) == []
    # the parts and the model hold the same tensors, and a mode change reaches the parts
    assert model._part["heads"].t(Hd.DET + "1.weight") is model.get_parameter(Hd.DET + "1.weight")
    assert all(p.training for p in model._parts()) and not any(p.training for p in model.eval()._parts())


def test_refusals():
    from xpoint_amd import models, synth, training
    with pytest.raises(NotImplementedError, match="mixed_precision"):
        training.XPointNet.from_model(_net(mixed_precision=True))
    cfg = synth.multipoint_config()
    conv = models.XPoint(cfg)
    conv.load_state_dict({k: torch.from_numpy(np.array(v, copy=True)) for k, v in synth.make_conv_xpoint_state_dict(cfg).items()})
    with pytest.raises(NotImplementedError, match="use_attention"):
        training.XPointNet.from_model(conv)
    model = training.XPointNet.from_model(_net(multispectral=True))
    with pytest.raises(ValueError, match="mixes is_optical"):
        model(_pair(flags=([True, False], [False, False])))
    with pytest.raises(ValueError, match="mixes is_optical"):
        model(_pair(flags=([True, True], [False, True])))
    with pytest.raises(RuntimeError, match="needs is_optical"):
        model(_pair())
