"""GPU: training of the whole VMamba encoder on the HIP library (xpoint_amd.training.VSSEncoder) — the stride-2 weight and input
gradients and the stem's kernels one by one against float64 torch autograd, the encoder end to end against the float64 restatement of
tests/encoder_f64.py and the real reference's results (tests/golden/g33_encoder_training.npz), the eval forward against the inference model,
determinism, batch neighbours, stochastic depth, a short optimisation run and the way back into the inference model.  Bar: max |got - ref| <= 1e-4 x the
scale of each tensor (tests.training_cases.TOL); every comparison prints err / scale."""
import pytest
import torch
import torch.nn.functional as F

from tests import encoder_f64 as En
from tests.training_cases import _bits, _close
from xpoint_amd import synth

pytestmark = pytest.mark.gpu

# (B, H, W, Ci, Co)
CONV_SHAPES = [(2, 5, 7, 8, 32),          # odd sizes: the last input row and column are hit by one tap row only
               (1, 4, 6, 48, 96),         # even sizes, patch embed's real channels
               (2, 1, 1, 16, 32), (1, 1, 9, 16, 32),          # degenerate axes
               (2, 24, 23, 32, 64),       # 2 x 12 x 12 = 288 output rows cross XP_WGRAD_CHUNK
               (1, 4, 4, 96, 192), (1, 2, 2, 384, 768),          # real downsampler channels
               (1, 3, 3, 128, 16),        # Ci = 128: the row-stationary input gradient's widest tile
               (2, 5, 7, 8, 24), (1, 6, 5, 72, 20)]          # Co % 16 != 0: the input gradient's tile-engine form, both tile widths


def _u(name, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform("enc_gpu/" + name, shape, lo, hi))


def _im2col_s2(x_nhwc):
    """(B, H, W, Ci) -> (B Ho Wo, 9 Ci): the A operand of the 3x3 stride-2 convolution with zero padding 1, taps row-major"""
    B, H, W, Ci = x_nhwc.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x_nhwc.permute(0, 3, 1, 2), (1, 1, 1, 1))
    return torch.cat([xp[:, :, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2].permute(0, 2, 3, 1).reshape(B * Ho * Wo, Ci)
                      for ky in range(3) for kx in range(3)], 1).contiguous()


def _conv_case(shape):
    B, H, W, Ci, Co = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, w = _u(f"x{shape}", (B, H, W, Ci), -2.0, 2.0), _u(f"w{shape}", (Co, 3, 3, Ci), -0.5, 0.5)
    dy = _u(f"dy{shape}", (B, Ho, Wo, Co)) * 1e-2
    a, k = x.double().permute(0, 3, 1, 2).requires_grad_(True), w.double().permute(0, 3, 1, 2).requires_grad_(True)
    gx, gw = torch.autograd.grad(F.conv2d(a, k, stride=2, padding=1), [a, k], dy.double().permute(0, 3, 1, 2))
    return x, w, dy, gx.permute(0, 2, 3, 1), gw.permute(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------------------------- the new kernels, one by one
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3x3_s2_wgrad(gpu_lib, shape):
    from xpoint_amd import training as T
    B, H, W, Ci, Co = shape
    x, _, dy, _, gw = _conv_case(shape)
    xg, dyg = x.cuda(), dy.cuda()
    dw = T.conv3x3_s2_wgrad(xg, dyg)
    assert dw.shape == (Co, 3, 3, Ci)
    _close(dw, gw, f"conv3x3_s2_wgrad {shape}")
    via = T.gemm_tn(dyg.view(-1, Co), _im2col_s2(xg))
    assert torch.equal(_bits(dw.view(Co, 9 * Ci)), _bits(via)), "differs from gemm_tn on the materialised stride-2 im2col"
    assert torch.equal(_bits(dw), _bits(T.conv3x3_s2_wgrad(xg, dyg))), "two calls differ"
    gs, sc = T.scale_grad(dyg)
    assert torch.equal(_bits(T.conv3x3_s2_wgrad(xg, gs, dy_scale=sc)), _bits(dw)), "the scaled call differs from the unscaled call"
    with pytest.raises(Exception):
        T.conv3x3_wgrad(xg, xg[..., :1].expand(B, H, W, Co).contiguous(), stride=2)          # the stride-1 entry keeps refusing


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3x3_s2_dgrad(gpu_lib, shape):
    from xpoint_amd import training as T
    B, H, W, Ci, Co = shape
    _, w, dy, gx, _ = _conv_case(shape)
    wg, dyg = w.cuda(), dy.cuda()
    dx = T.conv3x3_s2_dgrad(dyg, wg, (H, W))
    assert dx.shape == (B, H, W, Ci)
    _close(dx, gx, f"conv3x3_s2_dgrad {shape}")
    assert torch.equal(_bits(dx), _bits(T.conv3x3_s2_dgrad(dyg, wg, (H, W)))), "two calls differ"
    gs, sc = T.scale_grad(dyg)
    shared = T.conv3x3_s2_dgrad(gs, wg, (H, W), dy_scale=sc)
    _close(shared, gx, f"conv3x3_s2_dgrad {shape}, dy_scale given")
    for b in range(B):          # one S shared: nothing else crosses a sample boundary
        one = T.conv3x3_s2_dgrad(gs[b:b + 1].contiguous(), wg, (H, W), dy_scale=sc)
        assert torch.equal(_bits(one[0]), _bits(shared[b])), f"sample {b}: dx depends on the batch neighbours"
    for f in (2.0 ** 40, 2.0 ** -40):
        _close(T.conv3x3_s2_dgrad(dyg * f, wg, (H, W)), gx * f, f"conv3x3_s2_dgrad {shape}, dy x {f:g}")
    assert not bool(T.conv3x3_s2_dgrad(torch.zeros_like(dyg), wg, (H, W)).any()), "an all-zero dy must give exact zeros"


@pytest.mark.parametrize("Co", [16, 48])
def test_stem_conv_is_the_fused_kernels_convolution(gpu_lib, Co):
    """xp_stem_conv -> xp_layernorm -> xp_gelu_fwd against the inference path's one launch; (3, 33, 70): odd sizes, more than one block of 64 pixels"""
    from xpoint_amd import _lib as L, training as T
    from xpoint_amd.training import ops
    B, H, W = 3, 33, 70
    img = _u(f"stem/img{Co}", (B, 1, H, W), 0.0, 1.0).cuda()
    w9, b = _u(f"stem/w{Co}", (9, Co), -0.5, 0.5).cuda(), _u(f"stem/b{Co}", (Co,), -0.2, 0.2).cuda()
    lw, lb = _u(f"stem/lw{Co}", (Co,), 0.5, 1.5).cuda(), _u(f"stem/lb{Co}", (Co,), -0.2, 0.2).cuda()
    c = T.stem_conv(img, w9, b)
    Ho, Wo = 17, 35
    assert c.shape == (B, Ho, Wo, Co)
    ref = F.conv2d(img.double().cpu(), w9.double().cpu().t().reshape(Co, 1, 3, 3), b.double().cpu(), stride=2, padding=1).permute(0, 2, 3, 1)
    _close(c, ref, f"stem_conv Co={Co} vs float64")
    st = L.current_stream(img)
    got = T.gelu_fwd(ops._layernorm(c.view(-1, Co), lw, lb, st)).view(c.shape)
    fused = torch.empty_like(c)
    L.call("xp_stem_conv_ln_gelu", L.ptr(img), L.ptr(w9), L.ptr(b), L.ptr(lw), L.ptr(lb), L.ptr(fused), B, H, W, Co, 1e-5, st)
    print(f"stem Co={Co}: three launches bit-equal to the fused launch: {torch.equal(_bits(got), _bits(fused))}")
    _close(got, fused, f"stem Co={Co}: conv -> LN -> GELU vs xp_stem_conv_ln_gelu")


@pytest.mark.parametrize("Co", [16, 48])
@pytest.mark.parametrize("shape", [(2, 6, 10), (1, 5, 7), (3, 32, 32)])
def test_stem_conv_wgrad(gpu_lib, shape, Co):
    """(1, 5, 7): odd sizes; (3, 32, 32): 768 output pixels, more than one round of the 512-row column-sum pass"""
    from xpoint_amd import training as T
    B, H, W = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img, dy = _u(f"sw/img{shape}", (B, 1, H, W), 0.0, 1.0), _u(f"sw/dy{shape}{Co}", (B, Ho, Wo, Co)) * 1e-2
    k = torch.zeros(Co, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad(F.conv2d(img.double(), k, stride=2, padding=1), [k], dy.double().permute(0, 3, 1, 2))
    dw = T.stem_conv_wgrad(img.cuda(), dy.cuda())
    assert dw.shape == (9, Co)
    _close(dw, gw.reshape(Co, 9).t(), f"stem_conv_wgrad {shape} Co={Co}")
    assert torch.equal(_bits(dw), _bits(T.stem_conv_wgrad(img.cuda(), dy.cuda()))), "two calls differ"
    gs, sc = T.scale_grad(dy.cuda())
    _close(T.stem_conv_wgrad(img.cuda(), gs, dy_scale=sc), gw.reshape(Co, 9).t(), f"stem_conv_wgrad {shape} Co={Co}, dy_scale given")


# ---------------------------------------------------------------------------------------------------------------- the encoder
def _encoder(case, train=True, drop_path_rate=0.0):
    from xpoint_amd import training as T
    E, depths, _ = En.CASES[case]
    enc = T.VSSEncoder(E, depths, drop_path_rate=drop_path_rate)
    enc.load_state_dict(En.encoder_state(case, torch.float32))
    return enc.cuda().train(train)


def _step(enc, images, Rw, **kw):
    """{'out', 'grad/<name>'} of sum(out * Rw) on the GPU"""
    enc.zero_grad(set_to_none=True)
    out = enc(images.cuda(), **kw)
    (out * Rw.cuda()).sum().backward()
    res = {"out": out.detach()}
    for k, p in enc.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        res["grad/" + k] = p.grad
    return res


@pytest.mark.parametrize("case", list(En.CASES))
def test_encoder_step(gpu_lib, case):
    images, Rw = En.case_inputs(case)
    got = _step(_encoder(case), images, Rw)
    ref = En.case_reference(case)
    assert sorted(got) == sorted(ref)
    for k in ref:
        _close(got[k], ref[k], f"{case}/{k} vs the restatement")
    if case in En.GOLDEN_CASES:
        golden = En.golden()
        for k in golden.files:
            _close(got[k][:golden[k].shape[0]], golden[k], f"{case}/{k} vs the reference")          # the largest gradient is stored as its leading output channels
    if case == "D":
        fac = [tuple(torch.tensor(f) for f in pair) for pair in En.D_FACTORS]
        got = _step(_encoder(case, drop_path_rate=0.2), images, Rw, drop_path_scale=fac)
        ref = En.case_reference(case, True)
        for k in ref:
            _close(got[k], ref[k], f"{case}/{k}, given factors, vs the restatement")


@pytest.mark.parametrize("case", ["S", "R"])
def test_eval_forward_is_the_inference_encoder(gpu_lib, case):
    from xpoint_amd import models
    cfg = En.model_config(case)
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    net = net.to("cuda").eval()
    images = En.case_inputs(case)[0].cuda()
    enc = _encoder(case, train=False)
    got = enc(images)
    assert not got.requires_grad
    want = net.forward_raw(images, want_prob=False, want_desc=False)["enc_nhwc"]
    _close(got, want, f"{case}: eval forward vs the inference model's enc_nhwc")
    enc.train()
    assert torch.equal(_bits(enc(images).detach()), _bits(got)), "train() with every rate 0 must give eval()'s bits"


def test_two_steps_are_bit_identical(gpu_lib):
    images, Rw = En.case_inputs("D")
    enc = _encoder("D", drop_path_rate=0.3)
    a = {k: v.clone() for k, v in _step(enc, images, Rw, seed=5).items()}
    b = _step(enc, images, Rw, seed=5)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_batch_neighbours(gpu_lib):
    images, Rw = En.case_inputs("S")
    enc = _encoder("S")
    with torch.no_grad():
        both = enc(images.cuda())
        for b in range(images.shape[0]):
            assert torch.equal(_bits(enc(images[b:b + 1].cuda())[0]), _bits(both[b])), f"sample {b}: the output depends on the batch neighbours"


def test_stochastic_depth_draws(gpu_lib):
    """repeatable, keyed by the sample id and not by the position in the batch, and different from block to block"""
    from xpoint_amd.training import encoder as E
    B = 4
    images = _u("sd/img", (B, 1, 32, 32), 0.0, 1.0).cuda()
    enc = _encoder("D", drop_path_rate=0.5)
    with torch.no_grad():
        a, b = enc(images, seed=11), enc(images, seed=11)
        perm = torch.tensor([2, 0, 3, 1])
        c = enc(images[perm.cuda()], seed=11, sample_ids=perm)
        other = enc(images, seed=12)
    assert torch.equal(_bits(a), _bits(b)), "seeded draws are not repeatable"
    assert torch.equal(_bits(c), _bits(a[perm.cuda()])), "a sample's draw depends on its position in the batch"
    assert not torch.equal(a, other), "the draws do not depend on the seed"
    draws = [[E.drop_path_draws(0.5, 11, range(64), br, blk) for br in (0, 1)] for blk in range(5)]
    flat = [tuple(d) for pair in draws for d in pair]
    assert len(set(flat)) == len(flat), "two (block, branch) pairs share their draws"
    assert set(flat[0]) == {0.0, 2.0}
    with torch.no_grad():
        given = enc(images, drop_path_scale=[tuple(torch.tensor(E.drop_path_draws(r, 11, range(B), br, i)) if r > 0 else torch.ones(B) for br in (0, 1))
                                             for i, r in enumerate(enc.rates)])
    assert torch.equal(_bits(given), _bits(a)), "the seeded forward is not the forward under its own factors"


def test_learning_and_the_way_back(gpu_lib):
    """eight Adam steps on case S lower |enc - target|^2 and leave every parameter finite and changed; the tuned encoder changes the inference model"""
    from xpoint_amd import models, training as T
    cfg = En.model_config("S")
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    net = net.to("cuda").eval()
    enc = T.VSSEncoder.from_model(net).cuda().train()
    assert enc.rates[-1] == pytest.approx(0.2)
    images = En.case_inputs("S")[0].cuda()
    before = net.forward_raw(images, want_prob=False, want_desc=False)["enc_nhwc"].clone()
    target = before * 0.5
    start = {k: v.detach().clone() for k, v in enc.named_parameters()}
    opt = torch.optim.Adam(enc.parameters(), lr=1e-3)
    ones = [(torch.ones(2), torch.ones(2))] * 4
    losses = []
    for _ in range(9):
        opt.zero_grad(set_to_none=True)
        loss = ((enc(images, drop_path_scale=ones) - target) ** 2).sum()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print("losses:", " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < losses[0], losses
    for k, p in enc.named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), start[k]), k
    r = net.load_state_dict(enc.state_dict(), strict=False)
    assert list(r.unexpected_keys) == []
    after = net.forward_raw(images, want_prob=False, want_desc=False)["enc_nhwc"]
    with torch.no_grad():
        _close(enc.eval()(images), after, "the tuned encoder's eval forward vs the inference model that loaded it")
    assert float(((after - target) ** 2).sum()) < float(((before - target) ** 2).sum())


def test_refusals(gpu_lib):
    from xpoint_amd import training as T
    enc = _encoder("D")
    with pytest.raises(RuntimeError, match=r"image must be \(B,1,H,W\)"):
        enc(torch.zeros(1, 3, 32, 32, device="cuda"))
    with pytest.raises(ValueError, match="multiples of 32"):
        enc(torch.zeros(1, 1, 48, 32, device="cuda"))
    with pytest.raises(TypeError, match="float32"):
        enc(torch.zeros(1, 1, 32, 32, device="cuda", dtype=torch.float16))
    with pytest.raises(ValueError):
        enc(torch.zeros(1, 1, 32, 32, device="cuda"), drop_path_scale=[(torch.ones(1), torch.ones(1))])
    z = lambda *s: torch.zeros(*s, device="cuda")          # noqa: E731
    with pytest.raises(ValueError):
        T.conv3x3_s2_wgrad(z(1, 4, 4, 8), z(1, 4, 4, 8))
    with pytest.raises(ValueError):
        T.conv3x3_s2_dgrad(z(1, 2, 2, 8), z(8, 3, 3, 4), (5, 4))
    with pytest.raises(Exception, match="multiple of 4"):
        T.conv3x3_s2_dgrad(z(1, 2, 2, 6), z(6, 3, 3, 4), (4, 4))
    with pytest.raises(Exception, match="48 or 16"):
        T.stem_conv(z(1, 1, 4, 4), z(9, 8), z(8))
