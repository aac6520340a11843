"""GPU: training of the whole VMamba XPoint on the HIP library (xpoint_amd.training.XPointNet / train_step) — the input gradient
of the reflection-padded 3x3 convolution (xp_conv3x3_rp_dgrad_h2) against float64 torch autograd, the heads' input gradient against the float64
restatement, the model end to end against tests/xpoint_train_f64.py and the real reference's results (tests/golden/g34_xpoint_training.npz), the eval
forward against the inference model, determinism, the two-encoder routing, the detach in front of the homography head, a short optimisation run and
the way back into the inference model.  Bar: max |got - ref| <= 1e-4 x the scale of each tensor (tests.training_cases.TOL); every comparison prints
err / scale."""
import numpy as np
import pytest
import torch

from tests import heads_f64 as Hd, xpoint_train_f64 as Xp
from tests.training_cases import AUG_CFG, AUG_CFG_HM, LOSS_CFG, LOSS_CFG_HM, _bits, _close
from xpoint_amd import synth

pytestmark = pytest.mark.gpu

# (B, H, W, Ci, Co)
DGRAD_SHAPES = [(1, 2, 2, 8, 32),          # n = 2: both pixels of an axis take a frame term
                (1, 3, 3, 16, 32),         # n = 3: pixel 1 takes both
                (2, 2, 9, 8, 32), (1, 9, 2, 8, 32),
                (1, 4, 5, 48, 96),
                (3, 9, 7, 48, 512), (2, 8, 16, 128, 512),          # the trunk's channels, VMamba and conv encoder (both tile widths of the frame GEMM)
                (2, 33, 32, 8, 24),        # Co % 16 != 0, and the rows cross an M tile
                (1, 6, 5, 72, 20)]


def _u(name, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform("xpt_gpu/" + name, shape, lo, hi))


def _dgrad_case(shape):
    B, H, W, Ci, Co = shape
    w, dy = _u(f"w{shape}", (Co, 3, 3, Ci), -0.5, 0.5), _u(f"dy{shape}", (B, H, W, Co)) * 1e-2
    gx = Xp.reflect_dgrad_autograd(dy.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2))
    return w, dy, gx.permute(0, 2, 3, 1)


def _composition(T, dy, w, dy_scale=None):
    """What the existing operators could do: the zero-padded input gradient of dy embedded in a zero (H + 2) x (W + 2) frame is g on the padded frame;
    torch folds the frame back."""
    B, H, W, Co = dy.shape
    frame = torch.zeros((B, H + 2, W + 2, Co), dtype=dy.dtype, device=dy.device)
    frame[:, 1:-1, 1:-1] = dy
    g = T.conv3x3_dgrad(frame, w, dy_scale=dy_scale)
    for axis, n in ((1, H), (2, W)):
        inner = g.narrow(axis, 1, n).clone()
        inner.narrow(axis, 1, 1).add_(g.narrow(axis, 0, 1))
        inner.narrow(axis, n - 2, 1).add_(g.narrow(axis, n + 1, 1))
        g = inner
    return g


# ---------------------------------------------------------------------------------------------------------------- the new kernel
@pytest.mark.parametrize("shape", DGRAD_SHAPES)
def test_conv3x3_dgrad_reflect(gpu_lib, shape):
    from xpoint_amd import training as T
    B, H, W, Ci, Co = shape
    w, dy, gx = _dgrad_case(shape)
    wg, dyg = w.cuda(), dy.cuda()
    dx = T.conv3x3_dgrad_reflect(dyg, wg)
    assert dx.shape == (B, H, W, Ci)
    _close(dx, gx, f"conv3x3_dgrad_reflect {shape}")
    assert torch.equal(_bits(dx), _bits(T.conv3x3_dgrad_reflect(dyg, wg))), "two calls differ"
    gs, sc = T.scale_grad(dyg)
    shared = T.conv3x3_dgrad_reflect(gs, wg, dy_scale=sc)
    _close(shared, gx, f"conv3x3_dgrad_reflect {shape}, dy_scale given")
    for b in range(B):          # one S shared: nothing else crosses a sample boundary
        one = T.conv3x3_dgrad_reflect(gs[b:b + 1].contiguous(), wg, dy_scale=sc)
        assert torch.equal(_bits(one[0]), _bits(shared[b])), f"sample {b}: dx depends on the batch neighbours"
    for f in (2.0 ** 40, 2.0 ** -40):
        _close(T.conv3x3_dgrad_reflect(dyg * f, wg), gx * f, f"conv3x3_dgrad_reflect {shape}, dy x {f:g}")
    assert not bool(T.conv3x3_dgrad_reflect(torch.zeros_like(dyg), wg).any()), "an all-zero dy must give exact zeros"
    _close(_composition(T, dyg, wg), gx, f"the composition of existing operators {shape}")
    _close(dx, _composition(T, dyg, wg), f"conv3x3_dgrad_reflect {shape} vs the composition")


def test_conv3x3_dgrad_reflect_refusals(gpu_lib):
    from xpoint_amd import _lib, training as T
    z = lambda *s: torch.zeros(*s, device="cuda")          # noqa: E731
    with pytest.raises(_lib.XPointHipError, match="reflection needs H, W >= 2"):
        T.conv3x3_dgrad_reflect(z(1, 1, 4, 8), z(8, 3, 3, 4))
    with pytest.raises(_lib.XPointHipError, match="reflection needs H, W >= 2"):
        T.conv3x3_dgrad_reflect(z(1, 4, 1, 8), z(8, 3, 3, 4))
    with pytest.raises(_lib.XPointHipError, match="Co must be a multiple of 4"):
        T.conv3x3_dgrad_reflect(z(1, 4, 4, 6), z(6, 3, 3, 4))
    with pytest.raises(ValueError):
        T.conv3x3_dgrad_reflect(z(1, 4, 4, 8), z(4, 3, 3, 4))
    with pytest.raises(TypeError, match="float32"):
        T.conv3x3_dgrad_reflect(z(1, 4, 4, 8).double(), z(8, 3, 3, 4))


# ---------------------------------------------------------------------------------------------------------------- the heads pass the gradient on
def _heads(kind):
    from xpoint_amd import training as T
    sd = Hd.head_state(kind)
    heads = T.XPointHeads(in_channels=sd[Hd.DET + "1.weight"].shape[1], descriptor_size=sd[Hd.DSC + "4.weight"].shape[0])
    heads.load_state_dict(sd)
    return heads.cuda().train()


@pytest.mark.parametrize("case", Hd.CASES)
def test_heads_input_gradient(gpu_lib, case):
    kind = case.split("/")[0]
    seed, (enc, r1, r2), ref = Hd.case_reference(case)
    margin = Hd.relu_margin(ref["pre"])
    print(f"{case}: seed {seed}, ReLU margin {margin:.3e}")
    assert margin >= Hd.RELU_FLOOR                              # on the CPU, before any kernel runs
    p = {k: v.detach().double() for k, v in Hd.head_state(kind).items() if Xp.is_parameter(k)}
    x = enc.double().requires_grad_(True)
    logits, desc, _ = Xp.heads64(p, x)
    (want,) = torch.autograd.grad((logits * r1.double()).sum() + (desc * r2.double()).sum(), [x])

    def run(through):
        heads = _heads(kind)
        e = enc.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(through)
        out = heads._forward(e) if through else heads(e)
        ((out["logits"] * r1.cuda()).sum() + (out["desc"] * r2.cuda()).sum()).backward()
        return e.grad, [out["logits"], out["desc"]] + [q.grad for q in heads.parameters()] + [v.float() for v in heads.state_dict().values()]

    denc, a = run(True)
    none, b = run(False)
    assert none is None
    _close(denc, want.permute(0, 2, 3, 1), f"{case}: the gradient of enc vs f64")
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(_bits(u), _bits(v)), f"{case}: tensor {i} differs from the public frozen path"


# ---------------------------------------------------------------------------------------------------------------- the model
def _net(**over):
    from xpoint_amd import models
    cfg = Xp.model_config(**over)
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    return net.to("cuda").eval()


def _model(**over):
    from xpoint_amd import training as T
    return T.XPointNet.from_model(_net(**over)).cuda().train()


def _case_data(flags=None):
    inputs = Xp.case_inputs()
    data = {sp: {"image": inputs[sp][0].cuda()} for sp in Xp.SPECTRA}
    if flags is not None:
        for sp, f in zip(Xp.SPECTRA, flags):
            data[sp]["is_optical"] = torch.full((inputs[sp][0].shape[0], 1), f, device="cuda")
    return inputs, data


def _scalar(pred, inputs, spectra=Xp.SPECTRA):
    return sum((pred[sp]["logits"] * inputs[sp][1].cuda()).sum() + (pred[sp]["desc"] * inputs[sp][2].cuda()).sum() for sp in spectra)


def _step(model, flags=None, spectra=Xp.SPECTRA):
    inputs, data = _case_data(flags)
    model.zero_grad(set_to_none=True)
    out = model(data)
    pred = dict(zip(Xp.SPECTRA, out[:2]))
    _scalar(pred, inputs, spectra).backward()
    res = {f"{w}/{sp}": pred[sp][w].detach() for w in ("logits", "desc") for sp in Xp.SPECTRA}
    res.update({"grad/" + k: p.grad for k, p in model.named_parameters()})
    return res, pred


def test_model_step(gpu_lib):
    ref = Xp.case_reference()
    for sp in Xp.SPECTRA:
        assert Hd.relu_margin(ref["pre/" + sp]) >= Hd.RELU_FLOOR          # on the CPU, before any kernel runs
    model = _model()
    got, pred = _step(model)
    for sp in Xp.SPECTRA:
        assert not pred[sp]["encoder_output"].requires_grad and pred[sp]["encoder_output"].shape == (2, 16, 8, 12)
    keys = [k for k in ref if not k.startswith(("pre/", "denc/"))]
    assert sorted(keys) == sorted(got)
    for k in keys:
        assert got[k] is not None, k
        _close(got[k], ref[k], f"{k} vs the restatement", scale=Xp.tensor_scale(ref, k) if k.startswith("grad/") else None)
    golden = Xp.golden()
    assert int(golden["seed"]) == Xp.case_seed()
    for k in golden.files:
        if k == "seed" or k.startswith("denc/"):
            continue
        part = Hd.golden_view(k.split("/")[0] if k.startswith("desc/") else k, got[k]) if k.startswith(("desc/", "grad/" + Hd.DET, "grad/" + Hd.DSC)) else got[k]
        _close(part[:golden[k].shape[0]], golden[k], f"{k} vs the reference", scale=Xp.tensor_scale(ref, k) if k.startswith("grad/") else None)
    assert int(model.get_buffer(Hd.DET + "3.num_batches_tracked")) == 2          # once per spectrum


def test_encoder_gradient_is_the_encoders_under_the_heads_gradient(gpu_lib):
    """the gradient of an encoder parameter is non-zero, matches the float64 gradient of enc on the way, and equals what VSSEncoder gives when it is
    fed the gradient of enc that the heads return"""
    from xpoint_amd import training as T
    ref = Xp.case_reference()
    model = _model()
    got, _ = _step(model)
    inputs, _ = _case_data()
    net = _net()
    heads, enc = T.XPointHeads.from_model(net).cuda().train(), T.VSSEncoder.from_model(net).cuda().train()
    for sp in Xp.SPECTRA:
        x = enc(inputs[sp][0].cuda())
        leaf = x.detach().requires_grad_(True)
        out = heads._forward(leaf)
        ((out["logits"] * inputs[sp][1].cuda()).sum() + (out["desc"] * inputs[sp][2].cuda()).sum()).backward()
        _close(leaf.grad, ref["denc/" + sp], f"the gradient of enc, {sp}, vs the restatement")
        _close(leaf.grad, Xp.golden()["denc/" + sp], f"the gradient of enc, {sp}, vs the reference")
        x.backward(leaf.grad)          # accumulates over the two spectra, as the model's one backward does
    for k, p in enc.named_parameters():
        assert bool(p.grad.any()), k
        assert torch.equal(_bits(got["grad/" + k]), _bits(p.grad)), f"{k}: the model's gradient is not VSSEncoder's under the heads' gradient"


def test_eval_forward_is_the_inference_model(gpu_lib):
    net = _net()
    inputs, data = _case_data()
    from xpoint_amd import training as T
    model = T.XPointNet.from_model(net).cuda().eval()
    pred = dict(zip(Xp.SPECTRA, model(data)[:2]))
    for sp in Xp.SPECTRA:
        raw = net.forward_raw(data[sp]["image"], want_logits=True)
        assert not pred[sp]["logits"].requires_grad
        _close(pred[sp]["encoder_output"].permute(0, 2, 3, 1), raw["enc_nhwc"], f"eval {sp}: enc vs the inference model")
        _close(pred[sp]["logits"].permute(0, 2, 3, 1), raw["logits_nhwc"], f"eval {sp}: logits vs the inference model")
        _close(pred[sp]["desc"].permute(0, 2, 3, 1), raw["desc_nhwc"], f"eval {sp}: desc vs the inference model")


def _pair_batch(B, h, w, aug_cfg, **kw):
    from xpoint_amd import augmentation as aug
    rng = np.random.default_rng(0)
    batch = synth.to_torch(synth.make_pair_batch(0, B, h, w), "cuda")
    for k, flag in (('optical', True), ('thermal', False)):
        batch[k] = {'image': batch[k]['image'].float().contiguous(), 'valid_mask': torch.ones((B, 1, h, w), dtype=torch.bool, device="cuda"),
                    'is_optical': torch.full((B, 1), flag, device="cuda"), 'keypoints': torch.from_numpy(rng.random((B, h, w)) < 0.02).cuda()}
    return aug.augment_pair_batch({'optical': batch['optical'], 'thermal': batch['thermal']}, aug_cfg, np.random.default_rng(1), seed=7, **kw)


def test_two_train_steps_are_bit_identical(gpu_lib):
    from xpoint_amd import losses, training as T
    data = _pair_batch(2, 64, 96, AUG_CFG)
    loss_fn = losses.XPointLoss(LOSS_CFG)
    runs = []
    for _ in range(2):
        model = _model(drop_path_rate=0.2)
        torch.manual_seed(3)                                    # the detector loss draws its label noise from torch's generator
        loss, _ = T.train_step(model, data, loss_fn, torch.optim.Adam(model.parameters(), lr=1e-4), seed=5)
        runs.append([_bits(loss.reshape(1))] + [_bits(v.float()) for v in model.state_dict().values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_multispectral_routing(gpu_lib):
    """an optical batch reaches `encoder_optical.*` only — by its flags, whichever side of the pair carries it"""
    model = _model(multispectral=True)
    for flags, spectrum, prefix in (((True, False), "optical", "encoder_optical."), ((True, False), "thermal", "encoder_thermal."),
                                    ((False, True), "optical", "encoder_thermal.")):
        got, _ = _step(model, flags=flags, spectra=(spectrum,))
        enc = {k: v for k, v in got.items() if k.startswith("grad/encoder")}
        assert len(enc) == 2 * 92
        for k, v in enc.items():
            if k.startswith("grad/" + prefix):
                assert v is not None and bool(v.any()), (flags, spectrum, k)
            else:
                assert v is None or not bool(v.any()), (flags, spectrum, k)


def test_homography_head_reads_detached_maps(gpu_lib):
    """with the regression term, `hm_regressor.*` takes gradients and every other gradient keeps its bits: the detach of XPoint.py:305/309"""
    import random
    from xpoint_amd import losses, models, training as T
    cfg = Xp.training_config(synth.xpoint_exp1_config(256, 256, hm_head=True, vssm={"DEPTHS": [1, 1, 1, 1]}))
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    np.random.seed(5); random.seed(5)
    data = _pair_batch(2, 256, 256, AUG_CFG_HM, warp_optical=[True, False])
    assert data['hfour_points'].shape == (2, 4, 2)
    grads = []
    for loss_cfg in (LOSS_CFG_HM, LOSS_CFG):
        model = T.XPointNet.from_model(net).cuda().train()
        assert any(k.startswith("hm_regressor.") for k in model.state_dict())
        torch.manual_seed(3)
        pred, pred2, pred_hm = model(data, seed=1)
        assert pred_hm.shape == (2, 8)
        loss, comp = losses.XPointLoss(loss_cfg)({'data': data, 'pred': pred, 'pred2': pred2, 'pred_hm': pred_hm})
        assert ('homography_regression_loss' in comp) == (loss_cfg is LOSS_CFG_HM)
        loss.backward()
        grads.append({k: p.grad for k, p in model.named_parameters()})
    with_hm, without = grads
    for k in with_hm:
        if k.startswith("hm_regressor."):
            assert with_hm[k] is not None and bool(with_hm[k].any()) and without[k] is None, k
        else:
            assert with_hm[k] is not None and torch.equal(_bits(with_hm[k]), _bits(without[k])), k
    assert bool(with_hm["encoder.patch_embed.0.weight"].any())
    r = net.load_state_dict(model.state_dict(), strict=False)
    assert list(r.unexpected_keys) == []


def test_learning_and_the_way_back(gpu_lib):
    """twenty Adam steps of train_step on one augmented batch lower the loss; the tuned state changes the inference model"""
    from xpoint_amd import losses, training as T
    net = _net()
    data = _pair_batch(2, 64, 96, AUG_CFG)
    images = torch.cat([data['optical']['image'], data['thermal']['image']], 0)
    before = {k: v.clone() for k, v in net.forward_raw(images, want_logits=True).items() if k in ("enc_nhwc", "logits_nhwc", "desc_nhwc")}
    model = T.XPointNet.from_model(net).cuda().train()
    start = {k: p.detach().clone() for k, p in model.named_parameters()}
    loss_fn = losses.XPointLoss(LOSS_CFG)
    optimizer = torch.optim.Adam(model.parameters(), lr=2e-4)
    history = []
    for step in range(20):
        torch.manual_seed(3)                                    # the detector loss draws its label noise from torch's generator
        loss, comp = T.train_step(model, data, loss_fn, optimizer, seed=step)
        assert bool(torch.isfinite(loss)) and 'descriptor_loss' in comp
        history.append(float(loss))
    print("losses:", " ".join(f"{v:.5f}" for v in history))
    assert history[-1] < history[0], history
    assert int(model.get_buffer(Hd.DET + "3.num_batches_tracked")) == 40          # once per spectrum and step
    for k, p in model.named_parameters():          # the heads' 3.bias / 4.bias: a zero gradient in exact arithmetic, nothing to ask of them
        assert bool(torch.isfinite(p).all()) and (Xp.zero_gradient_bias(k) or not torch.equal(p.detach(), start[k])), k
    r = net.load_state_dict(model.state_dict(), strict=False)
    assert list(r.unexpected_keys) == []
    net.to("cuda")
    after = net.forward_raw(images, want_logits=True)
    for k, v in before.items():
        assert not torch.equal(after[k], v), f"{k}: the tuned state has not changed the inference model"
    pred, pred2, _ = model.eval()({'optical': {'image': images[:2]}, 'thermal': {'image': images[2:]}})
    _close(torch.cat([pred["logits"], pred2["logits"]], 0).permute(0, 2, 3, 1), after["logits_nhwc"], "the tuned model's eval logits vs the inference model")
