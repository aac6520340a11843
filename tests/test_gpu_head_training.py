"""GPU: head training on the HIP library (xpoint_amd.training, csrc/train_dense.hip) — the dense backward operators one by
one, the heads end to end against the float64 restatement of tests/heads_f64.py and the real reference's results (tests/golden/g30_head_training.npz),
and one fine-tuning run.  Bar: max |got - ref| <= 1e-4 x the scale of each tensor (the project's f32 bar); every comparison prints err / scale.
Bit-level properties (repeatability, the output window, the power-of-two operand scale, exact zeros) are exact."""
import numpy as np
import pytest
import torch

from tests import heads_f64 as Hd
from tests.training_cases import AUG_CFG, LOSS_CFG, _bits, _close, _im2col, _net, _rand

pytestmark = pytest.mark.gpu
CHUNK = 256           # XP_WGRAD_CHUNK of include/xpoint_hip.h (pinned by test_chunk_constant)


def test_chunk_constant():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "xpoint_hip.h")).read()
    assert int(re.search(r"#define XP_WGRAD_CHUNK (\d+)", hdr).group(1)) == CHUNK


# ---------------------------------------------------------------------------------------------------------------- weight-gradient GEMM
@pytest.mark.parametrize("IJ", [(65, 256), (8, 4), (512, 432), (256, 256)])
@pytest.mark.parametrize("M", [1, 31, 33, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17])
def test_gemm_tn(gpu_lib, M, IJ):
    from xpoint_amd import training as T
    I, J = IJ
    P = (_rand((M, I), 1000 + M) * 3e-6).cuda()              # a gradient-sized operand
    Q = _rand((M, J), 2000 + M, -4.0, 4.0).cuda()
    big = torch.full((I + 2, J + 5), float("nan"), device="cuda")
    out = T.gemm_tn(P, Q, out=big[1:1 + I, 2:2 + J])
    inside = torch.zeros_like(big, dtype=torch.bool); inside[1:1 + I, 2:2 + J] = True
    assert bool(torch.isnan(big[~inside]).all()), "written outside the output window"
    assert bool(torch.isfinite(big[inside]).all())
    _close(out, P.double().t() @ Q.double(), f"gemm_tn M={M} I={I} J={J}")
    again = T.gemm_tn(P, Q)
    assert torch.equal(_bits(again), _bits(out)), "two calls differ"
    for k in (-30, 10):                                       # one power of two per call, undone exactly
        assert torch.equal(_bits(T.gemm_tn(P * 2.0 ** k, Q)), _bits(again * 2.0 ** k)), k
    assert float(again.abs()[again != 0].min()) * 2.0 ** -30 > 1.2e-38          # no output of the scaled runs is an f32 subnormal
    z = T.gemm_tn(torch.zeros_like(P), Q)
    assert torch.equal(_bits(z), torch.zeros_like(_bits(z))), "an all-zero operand must give exact zeros"


def test_gemm_tn_column_slices(gpu_lib):
    """the descriptor 1x1 layer: Q = columns 256..511 of a 512-wide activation, P a slice of a padded gradient"""
    from xpoint_amd import training as T
    M = CHUNK + 1
    wide = _rand((M, 512), 5, -2.0, 2.0).cuda()
    Pw = (_rand((M, 68), 6) * 1e-4).cuda()
    out = T.gemm_tn(Pw[:, :65], wide[:, 256:])
    _close(out, Pw[:, :65].double().t() @ wide[:, 256:].double(), "gemm_tn ldp=68 ldq=512")
    assert torch.equal(_bits(out), _bits(T.gemm_tn(Pw[:, :65].contiguous(), wide[:, 256:].contiguous()))), "a slice and its copy differ"
    # an operand that arrives scaled, with its {S, 1 / S}
    S = torch.tensor([2.0 ** 20, 2.0 ** -20], device="cuda")
    _close(T.gemm_tn((Pw * 2.0 ** 20)[:, :65], wide[:, 256:], p_scale=S), Pw[:, :65].double().t() @ wide[:, 256:].double(), "gemm_tn with p_scale")


# ---------------------------------------------------------------------------------------------------------------- convolution weight gradient
@pytest.mark.parametrize("shape", [(1, 2, 2, 4, 8), (1, 3, 5, 48, 32), (3, 9, 7, 48, 512), (2, 33, 32, 48, 64)])
def test_conv3x3_wgrad(gpu_lib, shape):
    """(1, 2, 2, 4, 8): both reflected indices fold onto the same image; (2, 33, 32, ..): 1056 rows per image, no multiple of the chunk length: chunk boundaries fall
    inside both images."""
    from xpoint_amd import training as T
    B, H, W, Ci, Co = shape
    assert shape != (2, 33, 32, 48, 64) or ((H * W) % CHUNK != 0 and H * W > CHUNK)          # a chunk boundary inside every image
    x = _rand((B, H, W, Ci), 11, -2.0, 2.0).cuda()
    dy = (_rand((B, H, W, Co), 12) * 1e-5).cuda()
    dw = T.conv3x3_wgrad(x, dy)
    assert dw.shape == (Co, 3, 3, Ci)
    cols = _im2col(x)
    via = T.gemm_tn(dy.view(-1, Co), cols)
    assert torch.equal(_bits(dw.view(Co, 9 * Ci)), _bits(via)), "implicit and materialised im2col differ"
    _close(dw.view(Co, 9 * Ci), dy.view(-1, Co).double().t() @ cols.double(), f"conv3x3_wgrad {shape}")
    a = x.detach().cpu().double().permute(0, 3, 1, 2)
    w = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(torch.nn.functional.pad(a, (1, 1, 1, 1), mode="reflect"), w)
    (g,) = torch.autograd.grad(y, w, dy.cpu().double().permute(0, 3, 1, 2))
    _close(dw.permute(0, 3, 1, 2), g, f"conv3x3_wgrad {shape} vs autograd")
    assert torch.equal(_bits(T.conv3x3_wgrad(x, dy)), _bits(dw)), "two calls differ"


def test_operator_wrappers_check_every_operand(gpu_lib):
    from xpoint_amd import _lib, training as T
    a, b = torch.zeros(4, 3, device="cuda"), torch.zeros(4, 5, device="cuda")
    g = torch.ones(3, device="cuda")
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        T.gemm_tn(a, b.cpu())
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        T.bn_train_fwd(a, g.cpu(), g)
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        T.l2norm_rows_bwd(a, a.cpu())
    with pytest.raises(TypeError, match="float32"):
        T.gemm_tn(a, b.double())
    with pytest.raises(TypeError, match="float32"):
        T.bn_train_fwd(a, g.double(), g)


def test_conv3x3_wgrad_refusals(gpu_lib):
    from xpoint_amd import _lib, training as T
    x, dy = torch.zeros(1, 4, 4, 4, device="cuda"), torch.zeros(1, 4, 4, 8, device="cuda")
    with pytest.raises(_lib.XPointHipError, match="only stride 1 with reflection padding 1"):
        T.conv3x3_wgrad(x, dy, stride=2)
    with pytest.raises(_lib.XPointHipError, match="only stride 1 with reflection padding 1"):
        T.conv3x3_wgrad(x, dy, reflect_pad=0)


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
def _bn64(x, gamma, beta, dy, mask):
    x, gamma, beta, dy = (t.detach().cpu().double() for t in (x, gamma, beta, dy))
    rows = x.shape[0]
    mean, var = x.mean(0), x.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    xh = (x - mean) * invstd
    dg, db = (dy * xh).sum(0), dy.sum(0)
    dx = gamma * invstd * (dy - db / rows - xh * dg / rows)
    if mask:
        dx = dx * (x > 0)
    return dict(y=xh * gamma + beta, mean=mean, var=var, invstd=invstd, dgamma=dg, dbeta=db, dx=dx)


def _bn_case(rows, C, mean=0.0, dev=1.0, relu=False):
    from xpoint_amd import training as T
    x = (_rand((rows, C), 31 + rows, -1.7, 1.7) * dev + mean)
    if relu:
        x = torch.relu(x)
    x = x.cuda()
    gamma, beta = _rand((C,), 32, 0.5, 1.5).cuda(), _rand((C,), 33).cuda()
    dy = (_rand((rows, C), 34 + rows) * 1e-3).cuda()
    ref = _bn64(x, gamma, beta, dy, relu)
    y, sm, si, var = T.bn_train_fwd(x, gamma, beta)
    tag = f"bn rows={rows} C={C} mean={mean} relu={relu}"
    _close(y, ref["y"], tag + " y")
    _close(sm[0].double() + sm[1].double(), ref["mean"], tag + " mean", scale=max(float(ref["mean"].abs().max()), dev))
    _close(si, ref["invstd"], tag + " invstd")
    _close(var, ref["var"], tag + " var")
    y2, sm2, si2, var2 = T.bn_train_fwd(x, gamma, beta)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in ((y, y2), (sm, sm2), (si, si2), (var, var2))), "forward not repeatable"
    dx, dg, db, none = T.bn_train_bwd(dy, x, gamma, sm, si, relu_mask=relu)
    assert none is None
    _close(dx, ref["dx"], tag + " dx")
    _close(dg, ref["dgamma"], tag + " dgamma")
    _close(db, ref["dbeta"], tag + " dbeta")
    _close(T.colsum_rows(dy), ref["dbeta"], tag + " colsum")
    dxs, dg2, db2, scale = T.bn_train_bwd(dy, x, gamma, sm, si, relu_mask=relu, scaled=True)
    assert torch.equal(_bits(dg), _bits(dg2)) and torch.equal(_bits(db), _bits(db2)), "backward not repeatable"
    S, inv = float(scale[0]), float(scale[1])
    assert S * inv == 1.0 and np.log2(S) == round(np.log2(S)) and 2.0 ** 13 <= float(dx.abs().max()) * S < 2.0 ** 14, (S, float(dx.abs().max()))
    assert torch.equal(_bits(dxs * inv), _bits(dx)), "the scaled output is not the power of two times the unscaled one"
    assert torch.equal(_bits(T.colsum_rows(dxs, scale)), _bits(T.colsum_rows(dx))), "column sums of the scaled operand"


@pytest.mark.parametrize("C", [65, 256, 512])
@pytest.mark.parametrize("rows", [2, 3, 1023, 4097])
def test_batchnorm_train(gpu_lib, rows, C):
    _bn_case(rows, C)
    _bn_case(rows, C, relu=True)


def test_batchnorm_train_large_mean(gpu_lib):
    _bn_case(1023, 65, mean=1e3, dev=1e-2)


def test_batchnorm_strided_rows(gpu_lib):
    """the detector's (rows, 65) matrices live in 68-wide buffers"""
    from xpoint_amd import training as T
    rows, C = 37, 65
    xw = _rand((rows, 68), 41).cuda()
    gamma, beta = _rand((C,), 42, 0.5, 1.5).cuda(), _rand((C,), 43).cuda()
    dy = _rand((rows, C), 44).cuda()
    a = T.bn_train_fwd(xw[:, :C], gamma, beta)
    b = T.bn_train_fwd(xw[:, :C].contiguous(), gamma, beta)
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))
    dxw = torch.full((rows, 68), float("nan"), device="cuda")
    dx, dg, db, _ = T.bn_train_bwd(dy, xw[:, :C], gamma, a[1], a[2], dx=dxw[:, :C])
    assert bool(torch.isnan(dxw[:, C:]).all()) and bool(torch.isfinite(dx).all())
    assert torch.equal(_bits(dx.contiguous()), _bits(T.bn_train_bwd(dy, xw[:, :C].contiguous(), gamma, a[1], a[2])[0]))


# ---------------------------------------------------------------------------------------------------------------- L2-normalise backward
@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("rows", [1, 5, 1025])
def test_l2norm_rows_bwd(gpu_lib, rows, C):
    from xpoint_amd import training as T
    x, dy = _rand((rows, C), 51 + rows, -3.0, 3.0), _rand((rows, C), 52 + rows)
    a = x.double().requires_grad_(True)
    (g,) = torch.autograd.grad(torch.nn.functional.normalize(a, p=2, dim=1), a, dy.double())
    _close(T.l2norm_rows_bwd(x.cuda(), dy.cuda()), g, f"l2norm_bwd rows={rows} C={C}")


def test_l2norm_rows_bwd_zero_row(gpu_lib):
    """a row below eps follows torch: y = x / eps there, the clamp passes nothing to the norm"""
    from xpoint_amd import training as T
    x, dy = _rand((5, 64), 61), _rand((5, 64), 62)
    x[2] = 0.0
    a = x.double().requires_grad_(True)
    (g,) = torch.autograd.grad(torch.nn.functional.normalize(a, p=2, dim=1), a, dy.double())
    got = T.l2norm_rows_bwd(x.cuda(), dy.cuda())
    keep = [0, 1, 3, 4]
    _close(got[keep], g[keep], "l2norm_bwd rows beside the zero row")
    _close(got[2], g[2], "l2norm_bwd zero row")
    assert float(g[2].abs().max()) > 1e10


# ---------------------------------------------------------------------------------------------------------------- heads end to end
def _heads(kind, train=True):
    from xpoint_amd import training as T
    sd = Hd.head_state(kind)
    heads = T.XPointHeads(in_channels=sd[Hd.DET + "1.weight"].shape[1], descriptor_size=sd[Hd.DSC + "4.weight"].shape[0])
    heads.load_state_dict(sd)
    return heads.cuda().train(train)


@pytest.mark.parametrize("case", Hd.CASES)
def test_heads_training_step(gpu_lib, golden, case):
    seed, (enc, r1, r2), ref = Hd.case_reference(case)
    margin = Hd.relu_margin(ref["pre"])
    print(f"{case}: seed {seed}, ReLU margin {margin:.3e}")
    assert margin >= Hd.RELU_FLOOR                              # on the CPU, before any kernel runs
    g = golden("g30_head_training.npz")
    assert seed == int(g[f"{case}/seed"])
    heads = _heads(case.split("/")[0])
    out = heads(enc.permute(0, 2, 3, 1).contiguous().cuda())
    assert out["logits"].shape == r1.shape and out["desc"].shape == r2.shape
    ((out["logits"] * r1.cuda()).sum() + (out["desc"] * r2.cuda()).sum()).backward()
    got = {"logits": out["logits"], "desc": out["desc"]}
    for k, v in heads.state_dict().items():
        got[k] = v
    for k, p in heads.named_parameters():
        got["grad/" + k] = p.grad
    assert set(got) >= {k for k in ref if k != "pre"}
    for k in ref:
        if k == "pre":
            continue
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(ref[k]) == int(g[f"{case}/{k}"]) == 1
            continue
        sc = Hd.tensor_scale(ref, k)
        _close(got[k], ref[k], f"{case}/{k} vs f64", scale=sc)
        _close(Hd.golden_view(k, got[k]), g[f"{case}/{k}"], f"{case}/{k} vs reference", scale=sc)


def test_heads_training_step_is_repeatable(gpu_lib):
    case = "vmamba/3x9x7"
    seed, (enc, r1, r2), _ = Hd.case_reference(case)
    runs = []
    for _ in range(2):
        heads = _heads("vmamba")
        out = heads(enc.permute(0, 2, 3, 1).contiguous().cuda())
        ((out["logits"] * r1.cuda()).sum() + (out["desc"] * r2.cuda()).sum()).backward()
        runs.append([_bits(p.grad) for p in heads.parameters()] + [_bits(v.float()) for v in heads.state_dict().values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("kind", Hd.CONFIGS)
def test_eval_heads_equal_the_inference_path(gpu_lib, kind):
    from xpoint_amd import training as T
    net = _net(kind)
    images = _rand((2, 1, 64, 96), 71, 0.0, 1.0).cuda()
    flags = [True, False] if net.config["multispectral"] else None
    raw = net.forward_raw(images, want_logits=True, is_optical=flags)
    heads = T.XPointHeads.from_model(net).cuda().eval()
    assert heads.in_channels == (48 if kind == "vmamba" else 128)
    out = heads(raw["enc_nhwc"])
    _close(out["logits"].permute(0, 2, 3, 1), raw["logits_nhwc"], f"{kind} eval logits vs inference")
    _close(out["desc"].permute(0, 2, 3, 1), raw["desc_nhwc"], f"{kind} eval desc vs inference")
    assert not out["logits"].requires_grad
    r = net.load_state_dict(heads.state_dict(), strict=False)
    assert not r.unexpected_keys


def test_heads_refusals(gpu_lib):
    from xpoint_amd import _lib
    heads = _heads("vmamba")
    with pytest.raises(NotImplementedError, match="encoder is frozen"):
        heads(torch.zeros(1, 2, 2, 48, device="cuda", requires_grad=True))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        heads(torch.zeros(1, 1, 1, 48, device="cuda"))
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        heads(torch.zeros(1, 2, 2, 48))


# ---------------------------------------------------------------------------------------------------------------- one fine-tuning run
STEPS, LR = 8, 1e-3


def _batch_loss(net, heads, data, loss_fn):
    """the loss of the fixed batch with the current heads in training mode, without a step (and without touching the running statistics)"""
    from xpoint_amd import training as T
    keep = {k: v.clone() for k, v in heads.state_dict().items()}
    with torch.no_grad():
        enc = net.forward_raw(torch.cat([data['optical']['image'], data['thermal']['image']], 0), want_prob=False, want_desc=False,
                              is_optical=[True, True, False, False] if net.config["multispectral"] else None)["enc_nhwc"]
    torch.manual_seed(3)
    loss, _ = loss_fn({'data': data, 'pred': heads(enc[:2]), 'pred2': heads(enc[2:])})
    heads.load_state_dict(keep)
    return float(loss.detach())


def test_finetune_run(gpu_lib):
    from xpoint_amd import augmentation as aug, losses, synth, training as T
    net = _net("vmamba")
    B, h, w = 2, 64, 96
    rng = np.random.default_rng(0)
    batch = synth.to_torch(synth.make_pair_batch(0, B, h, w), "cuda")
    for k, flag in (('optical', True), ('thermal', False)):
        batch[k] = {'image': batch[k]['image'].float().contiguous(), 'valid_mask': torch.ones((B, 1, h, w), dtype=torch.bool, device="cuda"),
                    'is_optical': torch.full((B, 1), flag, device="cuda"), 'keypoints': torch.from_numpy(rng.random((B, h, w)) < 0.02).cuda()}
    data = aug.augment_pair_batch({'optical': batch['optical'], 'thermal': batch['thermal']}, AUG_CFG, np.random.default_rng(1), seed=7)
    heads = T.XPointHeads.from_model(net).cuda().train()
    loss_fn = losses.XPointLoss(LOSS_CFG)
    optimizer = torch.optim.Adam(heads.parameters(), lr=LR)
    net.forward_raw(torch.cat([data['optical']['image'], data['thermal']['image']], 0), want_prob=False, want_desc=False,
                    is_optical=[True] * B + [False] * B if net.config["multispectral"] else None)
    blobs = {k: w_.blob.clone() for k, w_ in net._weights.items()}            # packed on the first forward: every weight set the steps will use
    assert blobs
    first = _batch_loss(net, heads, data, loss_fn)
    for step in range(STEPS):
        torch.manual_seed(3)                                    # the detector loss draws its label noise from torch's generator
        loss, comp = T.finetune_step(net, heads, data, loss_fn, optimizer)
        print(f"step {step}: loss {float(loss):.6f}")
        assert bool(torch.isfinite(loss)) and 'descriptor_loss' in comp
    last = _batch_loss(net, heads, data, loss_fn)
    print(f"loss on the fixed batch: {first:.6f} -> {last:.6f} after {STEPS} Adam steps at lr {LR}")
    assert last < first
    assert int(heads.t(Hd.DET + "3.num_batches_tracked")) == 2 * STEPS          # once per spectrum and step
    for k, b in blobs.items():                                  # the frozen encoder's packed weights, bit for bit
        assert torch.equal(_bits(net._weights[k].blob), _bits(b)), k
    assert not net.training
    r = net.load_state_dict(heads.state_dict(), strict=False)
    assert not r.unexpected_keys
    net.to("cuda")
    images = torch.cat([data['optical']['image'], data['thermal']['image']], 0)
    raw = net.forward_raw(images, want_logits=True, is_optical=[True, True, False, False] if net.config["multispectral"] else None)
    out = heads.eval()(raw["enc_nhwc"])
    _close(out["logits"].permute(0, 2, 3, 1), raw["logits_nhwc"], "tuned heads: eval logits vs inference")
    _close(out["desc"].permute(0, 2, 3, 1), raw["desc_nhwc"], "tuned heads: eval desc vs inference")
