"""GPU: training of the homography head on the HIP library (xpoint_amd.training.RegNetHead, csrc/train_dense.hip, csrc/train_dgrad.hip, csrc/train_regnet.hip, DESIGN.md
section 15) — the new operators one by one, the head end to end against the float64 restatement of tests/regnet_f64.py and the real reference's results
(tests/golden/g31_regnet_training.npz), and a short fine-tuning run.  Bar: max |got - ref| <= 1e-4 x the scale of each tensor (the project's f32 bar);
every comparison prints err / scale.  Gates, masks, repeatability and the eval path are compared exactly.

End to end the gradients are compared CONDITIONED ON THE GPU'S OWN DECISIONS: a case has 3e5 to 1e6 ReLU / max-pool decisions, a handful of which lie
closer to the jump than f32 resolves, so the restatement is evaluated with the gates the GPU took (read from its BatchNorm outputs), after checking that
every gate that differs from the restatement's own sits within 1e-5 of the layer's scale of the jump and that such gates are at most 1e-4 of all."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import regnet_f64 as Rg
from tests.training_cases import AUG_CFG_HM as AUG_CFG, LOSS_CFG_HM as LOSS_CFG, _bits, _close, _im2col_zero, _net, _rand

pytestmark = pytest.mark.gpu
CHUNK = 256           # XP_WGRAD_CHUNK of include/xpoint_hip.h
GATE_MARGIN = 1e-5    # of the layer's scale: how close to the jump a decision must be for the two sides to be allowed to differ
GATE_SHARE = 1e-4     # of all decisions


# ---------------------------------------------------------------------------------------------------------------- zero-pad convolution gradients
CONV_SHAPES = [(1, 1, 1, 4, 8), (3, 9, 7, 12, 20), (1, 257, 1, 8, 4), (2, 16, 16, 96, 192)]


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_zero_pad_wgrad_and_dgrad(gpu_lib, shape):
    """(1, 1, 1, ..): every tap but the centre is outside; (1, 257, 1, ..): 257 rows cross one chunk of the weight gradient and W = 1 puts every
    horizontal neighbour outside; (2, 16, 16, 96, 192): the head's second convolution."""
    from xpoint_amd import training as T
    B, H, W, Ci, Co = shape
    assert shape != (1, 257, 1, 8, 4) or B * H * W == CHUNK + 1
    x = _rand((B, H, W, Ci), 21, -2.0, 2.0).cuda()
    w = _rand((Co, 3, 3, Ci), 22, -0.5, 0.5).cuda()
    dy = (_rand((B, H, W, Co), 23) * 1e-5).cuda()
    # float64 autograd of F.conv2d(padding=1)
    a = x.cpu().double().permute(0, 3, 1, 2).requires_grad_(True)
    k = w.cpu().double().permute(0, 3, 1, 2).requires_grad_(True)
    gx, gw = torch.autograd.grad(F.conv2d(a, k, padding=1), [a, k], dy.cpu().double().permute(0, 3, 1, 2))
    gx, gw = gx.permute(0, 2, 3, 1), gw.permute(0, 2, 3, 1)

    dw = T.conv3x3_wgrad_zero_pad(x, dy)
    assert dw.shape == (Co, 3, 3, Ci)
    via = T.gemm_tn(dy.view(-1, Co), _im2col_zero(x))
    assert torch.equal(_bits(dw.view(Co, 9 * Ci)), _bits(via)), "implicit and materialised zero-padded im2col differ"
    _close(dw, gw, f"zero-pad wgrad {shape}")
    assert torch.equal(_bits(T.conv3x3_wgrad_zero_pad(x, dy)), _bits(dw)), "wgrad: two calls differ"

    dx = T.conv3x3_dgrad(dy, w)
    assert dx.shape == (B, H, W, Ci)
    _close(dx, gx, f"zero-pad dgrad {shape}")
    assert torch.equal(_bits(T.conv3x3_dgrad(dy, w)), _bits(dx)), "dgrad: two calls differ"

    for f in (1e-20, 1e+20):            # any finite gradient range, found here (NULL) or supplied as {S, 1 / S}
        dyf = dy * f
        _close(T.conv3x3_wgrad_zero_pad(x, dyf), gw * f, f"zero-pad wgrad {shape} x {f:g}")
        _close(T.conv3x3_dgrad(dyf, w), gx * f, f"zero-pad dgrad {shape} x {f:g}")
        e = 13 - int(np.floor(np.log2(float(dyf.abs().max()))))            # max |dy| 2^e in [2^13, 2^14)
        S = torch.tensor([2.0 ** e, 2.0 ** -e], dtype=torch.float64).float().cuda()
        assert 2.0 ** 13 <= float((dyf.double() * 2.0 ** e).abs().max()) < 2.0 ** 14
        dys = (dyf.double() * 2.0 ** e).float()
        _close(T.conv3x3_wgrad_zero_pad(x, dys, dy_scale=S), gw * f, f"zero-pad wgrad {shape} x {f:g}, supplied scale")
        _close(T.conv3x3_dgrad(dys, w, dy_scale=S), gx * f, f"zero-pad dgrad {shape} x {f:g}, supplied scale")


def test_dgrad_refusals(gpu_lib):
    from xpoint_amd import _lib, training as T
    with pytest.raises(_lib.XPointHipError, match="Co must be a multiple of 4"):
        T.conv3x3_dgrad(torch.zeros(1, 4, 4, 6, device="cuda"), torch.zeros(6, 3, 3, 4, device="cuda"))
    with pytest.raises(TypeError, match="float32"):
        T.conv3x3_dgrad(torch.zeros(1, 4, 4, 8, device="cuda").double(), torch.zeros(8, 3, 3, 4, device="cuda"))
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        T.conv3x3_wgrad_zero_pad(torch.zeros(1, 4, 4, 4, device="cuda"), torch.zeros(1, 4, 4, 8))
    # the reflection-padded entry point keeps its contract: zero padding goes through the new one
    with pytest.raises(_lib.XPointHipError, match="only stride 1 with reflection padding 1"):
        T.conv3x3_wgrad(torch.zeros(1, 4, 4, 4, device="cuda"), torch.zeros(1, 4, 4, 8, device="cuda"), reflect_pad=0)


# ---------------------------------------------------------------------------------------------------------------- ReLU / max-pool backward
def _pool_relu_autograd(y_nhwc, dpool_nhwc):
    y = y_nhwc.cpu().permute(0, 3, 1, 2).clone().requires_grad_(True)
    out = F.max_pool2d(F.relu(y), 2)
    (g,) = torch.autograd.grad(out, y, dpool_nhwc.cpu().permute(0, 3, 1, 2))
    return g.permute(0, 2, 3, 1).contiguous()


def _pool_cases():
    cases = {"2x6x8x5": _rand((2, 6, 8, 5), 31), "1x5x7x3 (odd)": _rand((1, 5, 7, 3), 32), "all negative": -_rand((1, 4, 4, 3), 33, 0.1, 1.0)}
    t = _rand((1, 4, 4, 2), 34)
    t[0, 0:2, 0:2, 0] = torch.tensor([[-0.5, 0.75], [0.75, 0.75]])            # a positive tie: the first index (0, 1) must win
    t[0, 2:4, 2:4, 1] = torch.tensor([[0.0, -1.0], [0.0, -2.0]])              # a tie at 0: closed by the ReLU
    t[0, 0:2, 2:4, 1] = 0.25                                                  # all four equal
    cases["ties"] = t
    return cases


@pytest.mark.parametrize("name", list(_pool_cases()))
def test_maxpool2_relu_bwd(gpu_lib, name):
    from xpoint_amd import training as T
    y = _pool_cases()[name]
    B, H, W, C = y.shape
    dpool = _rand((B, H // 2, W // 2, C), 35, 0.5, 1.5)            # no zero: a misplaced gradient cannot hide
    want = _pool_relu_autograd(y, dpool)
    got = T.maxpool2_relu_bwd(dpool.cuda(), y.cuda())
    assert torch.equal(got.cpu(), want), name
    if name == "ties":
        assert float(got[0, 0, 1, 0]) == float(dpool[0, 0, 0, 0]) and float(got[0, 1, 0, 0]) == 0.0 and float(got[0, 0, 2, 1]) == float(dpool[0, 0, 1, 1])
        assert float(got[0, 2:4, 2:4, 1].abs().max()) == 0.0
    if name == "all negative":
        assert float(got.abs().max()) == 0.0


def test_relu_bwd(gpu_lib):
    from xpoint_amd import training as T
    y = _rand((3, 7, 5), 36)
    y[0, 0, :3] = torch.tensor([0.0, -0.0, 1e-45])
    dr = _rand((3, 7, 5), 37, 0.5, 1.5)
    got = T.relu_bwd(dr.cuda(), y.cuda())
    assert torch.equal(got.cpu(), torch.where(y > 0, dr, torch.zeros_like(dr)))
    assert got[0, 0, :3].tolist() == [0.0, 0.0, float(dr[0, 0, 2])]


# ---------------------------------------------------------------------------------------------------------------- cost volume
@pytest.mark.parametrize("shape", [(1, 5, 3), (3, 256, 192), (2, 70, 65)])
def test_costvolume_mean_bwd(gpu_lib, shape):
    from xpoint_amd import training as T
    B, hw, C = shape
    a, b, dv = _rand(shape, 41), _rand(shape, 42), _rand((B, hw), 43)
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    v = (a64 * b64.mean(1, keepdim=True)).sum(-1)
    ga, gb = torch.autograd.grad(v, [a64, b64], dv.double())
    da, db = T.costvolume_mean_bwd(a.cuda(), b.cuda(), dv.cuda())
    _close(da, ga, f"costvolume_mean_bwd {shape} da")
    _close(db, gb, f"costvolume_mean_bwd {shape} db")
    da2, db2 = T.costvolume_mean_bwd(a.cuda(), b.cuda(), dv.cuda())
    assert torch.equal(_bits(da2), _bits(da)) and torch.equal(_bits(db2), _bits(db)), "two calls differ"


# ---------------------------------------------------------------------------------------------------------------- dropout
def test_dropout_rows(gpu_lib):
    from xpoint_amd import training as T
    x = _rand((3, 256), 51, 0.5, 1.5).cuda()
    ids = torch.tensor([11, 5, 29], dtype=torch.int32, device="cuda")
    y0, m0 = T.dropout_rows(x, p=0.0, seed=9, sample_ids=ids)
    assert torch.equal(_bits(y0), _bits(x)) and bool(m0.all()), "p = 0 is the identity"
    y, m = T.dropout_rows(x, p=0.5, seed=9, sample_ids=ids)
    assert m.dtype == torch.uint8 and m.shape == x.shape and set(m.unique().tolist()) <= {0, 1}
    assert torch.equal(_bits(y), _bits(torch.where(m.bool(), 2.0 * x, torch.zeros_like(x)))), "kept values are 2 x, dropped ones 0"
    n, kept = m.numel(), int(m.sum())
    print(f"kept {kept} of {n}")
    assert abs(kept / n - 0.5) <= 4.0 * 0.5 / np.sqrt(n)          # four standard deviations of a fair coin over 3 x 256 draws
    for i in range(3):                                            # a sample's mask does not depend on its batch neighbours
        yi, mi = T.dropout_rows(x[i:i + 1], p=0.5, seed=9, sample_ids=ids[i:i + 1])
        assert torch.equal(mi[0], m[i]) and torch.equal(_bits(yi[0]), _bits(y[i])), i
    assert not torch.equal(T.dropout_rows(x, p=0.5, seed=10, sample_ids=ids)[1], m), "another seed draws another mask"
    assert not torch.equal(T.dropout_rows(x, p=0.5, seed=9, sample_ids=ids, tag=1)[1], m), "another tag draws another mask"
    given = (torch.arange(3 * 256, device="cuda").view(3, 256) % 3 == 0).to(torch.uint8)
    yr, mr = T.dropout_rows(x, p=0.5, mask=given)
    assert torch.equal(mr, given) and torch.equal(_bits(yr), _bits(torch.where(given.bool(), 2.0 * x, torch.zeros_like(x)))), "use_mask replays a given mask"


# ---------------------------------------------------------------------------------------------------------------- the head, end to end
def _head(train=True):
    from xpoint_amd import training as T
    head = T.RegNetHead()
    head.load_state_dict(Rg.head_state())
    return head.cuda().train(train)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _run(case, masks=True):
    """one forward + backward of a fresh head on the case's inputs with the golden's dropout masks -> (head, hm, {name: grad})"""
    (enc1, enc2, R), (m1, m2), _ = Rg.case_reference(case)
    head = _head()
    hm = head(_nhwc(enc1), _nhwc(enc2), dropout_masks=(m1.cuda(), m2.cuda()), keep_taps=True)
    (hm * R.cuda()).sum().backward()
    return head, hm.detach(), {k: p.grad.detach().clone() for k, p in head.named_parameters()}


def _margins(y1, y2):
    """float64 distance of every decision from its jump: (|y1|, |window maximum|, the window's top-two gap)"""
    win = Rg.windows(y2).sort(-1, descending=True).values
    return y1.abs(), win[..., 0].abs(), win[..., 0] - win[..., 1]


@pytest.mark.parametrize("case", Rg.CASES)
def test_regnet_training_step(gpu_lib, case):
    g = Rg.golden()
    (enc1, enc2, R), (m1, m2), ref = Rg.case_reference(case)
    head, hm, grads = _run(case)
    # 1. the forward pass: output, the BatchNorm outputs before the two ReLUs, the buffers
    _close(hm, ref["hm"], f"{case} hm")
    _close(hm, g[f"{case}/hm"], f"{case} hm vs the reference")
    taps = {k: [t.detach().cpu().permute(0, 3, 1, 2).contiguous() for t in head.last_taps[k]] for k in ("y1", "y2")}
    for k in ("y1", "y2"):
        for i in range(2):
            _close(taps[k][i], ref[k][i], f"{case} {k} of image {i + 1}")
    for k, v in head.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref[k]) == int(g[f"{case}/{k}"]) == 2, k
        elif "running_" in k:
            _close(v, ref[k], f"{case} {k}")
            _close(v, g[f"{case}/{k}"], f"{case} {k} vs the reference")
    # 2. the decisions the GPU took against the restatement's own
    gates = {"relu1": [], "relu2": [], "pool": []}
    differing = total = 0
    for i in range(2):
        gpu = Rg.gates_of(taps["y1"][i], taps["y2"][i])
        own = Rg.gates_of(ref["y1"][i], ref["y2"][i])
        scales = (float(ref["y1"][i].abs().max()), float(ref["y2"][i].abs().max()), float(ref["y2"][i].abs().max()))
        for name, a, b, margin, scale in zip(("relu1", "relu2", "pool"), gpu, own, _margins(ref["y1"][i], ref["y2"][i]), scales):
            diff = a != b
            n = int(diff.sum())
            worst = float(margin[diff].max()) / scale if n else 0.0
            print(f"{case} image {i + 1} {name}: {n} of {diff.numel()} decisions differ, largest float64 margin among them {worst:.2e} of scale")
            assert worst < GATE_MARGIN, (name, i, worst)
            differing += n; total += diff.numel()
            gates[name].append(a)
    print(f"{case}: {differing} of {total} decisions differ ({differing / total:.2e} of all)")
    assert differing <= GATE_SHARE * total
    # 3. every parameter gradient against the restatement evaluated with the GPU's decisions; against the reference where none differed
    cond = Rg.regnet_f64(Rg.head_state(), enc1, enc2, m1, m2, R, gates=gates)
    assert torch.equal(cond["hm"], ref["hm"])
    assert len(grads) == 10
    for k, got in grads.items():
        _close(got, cond["grad/" + k], f"{case} grad {k} (the GPU's gates)")
        if differing == 0:
            _close(Rg.golden_view(k, got), g[f"{case}/grad/{k}"], f"{case} grad {k} vs the reference", scale=Rg.tensor_scale(ref, "grad/" + k))


def test_regnet_training_is_repeatable(gpu_lib):
    case = "3x16x64"
    head_a, hm_a, grads_a = _run(case)
    head_b, hm_b, grads_b = _run(case)
    assert torch.equal(_bits(hm_a), _bits(hm_b))
    for k in grads_a:
        assert torch.equal(_bits(grads_a[k]), _bits(grads_b[k])), k
    for (k, a), b in zip(head_a.state_dict().items(), head_b.state_dict().values()):
        assert torch.equal(a, b), k


def test_regnet_seeded_dropout(gpu_lib):
    """without given masks the draws come from the seed: the same seed repeats the step bit for bit, another seed does not"""
    enc1, enc2, _ = Rg.case_inputs("3x16x64")
    a, b = _nhwc(enc1), _nhwc(enc2)
    hm1 = _head()(a, b, seed=5)
    assert torch.equal(_bits(hm1), _bits(_head()(a, b, seed=5))) and not torch.equal(hm1, _head()(a, b, seed=6))
    assert hm1.requires_grad and hm1.shape == (3, 8)


def test_eval_head_is_the_inference_path(gpu_lib):
    from xpoint_amd import convmodels, training as T
    enc1, enc2, R = Rg.case_inputs("2x64x16")
    a, b = _nhwc(enc1), _nhwc(enc2)
    head = _head(train=False)
    out = head(a, b)
    want = convmodels.regnet_forward(convmodels.regnet_weights(Rg.head_state(), "cuda"), a, b)
    assert out.shape == (2, 8) and not out.requires_grad and torch.equal(_bits(out), _bits(want))
    assert int(head.t(Rg.HM + "layer1.1.num_batches_tracked")) == 0
    # one optimizer step, then the inference model with the tuned head
    net = _net()
    head = T.RegNetHead.from_model(net).cuda().train()
    for k, v in Rg.head_state().items():
        assert torch.equal(head.state_dict()[k].cpu(), v), k
    opt = torch.optim.SGD(head.parameters(), lr=1e-2)
    images = _rand((4, 1, 256, 256), 61, 0.0, 1.0).cuda()
    with torch.no_grad():
        enc = net.forward_raw(images, want_prob=False, want_desc=False, is_optical=[True, True, False, False] if net.config["multispectral"] else None)["enc_nhwc"]
    assert enc.shape[1:] == (32, 32, 48)
    (head(enc[:2], enc[2:], seed=1) * R.cuda()).sum().backward()
    before = head.t(Rg.HM + "fc.4.weight").detach().clone()
    opt.step()
    assert not torch.equal(before, head.t(Rg.HM + "fc.4.weight"))
    r = net.load_state_dict(head.state_dict(), strict=False)
    assert not r.unexpected_keys
    net.to("cuda")
    assert torch.equal(_bits(net.predict_homography(images[:2], images[2:])), _bits(head.eval()(enc[:2], enc[2:])))


def test_regnet_refusals(gpu_lib):
    from xpoint_amd import _lib
    head = _head()
    z = torch.zeros(1, 32, 32, 48, device="cuda")
    with pytest.raises(NotImplementedError, match="encoder is frozen"):
        head(z.clone().requires_grad_(True), z)
    with pytest.raises(NotImplementedError, match="encoder is frozen"):
        head(z, z.clone().requires_grad_(True))
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        head(z.cpu(), z)
    with pytest.raises(RuntimeError, match="mat1 and mat2 shapes cannot be multiplied"):
        head(torch.zeros(1, 16, 16, 48, device="cuda"), torch.zeros(1, 16, 16, 48, device="cuda"))
    with pytest.raises(RuntimeError, match="mat1 and mat2 shapes cannot be multiplied"):
        head.eval()(torch.zeros(1, 16, 16, 48, device="cuda"), torch.zeros(1, 16, 16, 48, device="cuda"))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        head.train()(torch.zeros(1, 1, 1, 48, device="cuda"), torch.zeros(1, 1, 1, 48, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- one fine-tuning run
STEPS, LR = 3, 1e-3


def test_finetune_with_the_homography_head(gpu_lib):
    import random
    from xpoint_amd import augmentation as aug, losses, synth, training as T
    net = _net()
    B, h, w = 2, 256, 256
    rng = np.random.default_rng(0)
    batch = synth.to_torch(synth.make_pair_batch(0, B, h, w), "cuda")
    for k, flag in (('optical', True), ('thermal', False)):
        batch[k] = {'image': batch[k]['image'].float().contiguous(), 'valid_mask': torch.ones((B, 1, h, w), dtype=torch.bool, device="cuda"),
                    'is_optical': torch.full((B, 1), flag, device="cuda"), 'keypoints': torch.from_numpy(rng.random((B, h, w)) < 0.02).cuda()}
    np.random.seed(5); random.seed(5)
    data = aug.augment_pair_batch({'optical': batch['optical'], 'thermal': batch['thermal']}, AUG_CFG, np.random.default_rng(1), seed=7,
                                  warp_optical=[True, False])
    assert data['hfour_points'].shape == (B, 4, 2)
    loss_fn = losses.XPointLoss(LOSS_CFG)

    def run(with_regnet):
        heads = T.XPointHeads.from_model(net).cuda().train()
        regnet = T.RegNetHead.from_model(net).cuda().train() if with_regnet else None
        params = list(heads.parameters()) + (list(regnet.parameters()) if with_regnet else [])
        optimizer = torch.optim.Adam(params, lr=LR)
        start = {k: p.detach().clone() for k, p in regnet.named_parameters()} if with_regnet else None
        # without a prediction the loss must not ask for one: the run without the head uses the same configuration with the term switched off
        fn = loss_fn if with_regnet else losses.XPointLoss(dict(LOSS_CFG, homography_regression_loss={'check': False, 'gamma': 1.0}))
        for step in range(STEPS):
            torch.manual_seed(3)                                    # the detector loss draws its label noise from torch's generator
            loss, comp = T.finetune_step(net, heads, data, fn, optimizer, regnet=regnet, seed=step)
            print(f"{'with' if with_regnet else 'without'} the head, step {step}: loss {float(loss):.6f} {comp}")
            assert bool(torch.isfinite(loss))
            assert ('homography_regression_loss' in comp) == with_regnet
        return heads, regnet, start

    heads_a, regnet, start = run(True)
    heads_b, _, _ = run(False)
    for k, p in regnet.named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), start[k]), f"{k} has not moved"
    assert int(regnet.t(Rg.HM + "layer1.4.num_batches_tracked")) == 2 * STEPS
    # the encoder is frozen: the extra loss term reaches the homography head alone
    for (k, a), b in zip(heads_a.state_dict().items(), heads_b.state_dict().values()):
        assert torch.equal(a, b), k
