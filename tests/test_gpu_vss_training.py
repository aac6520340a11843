"""GPU: training of a VSS encoder block on the HIP library (xpoint_amd.training.VSSBlock, csrc/train_vss.hip) — the new kernels one
by one against float64 torch autograd, the block end to end against the float64 restatement of tests/vss_f64.py and the real reference's results
(tests/golden/g32_vss_training.npz), the eval forward against the inference path's launch sequence, determinism, batch neighbours, the gradient range,
stochastic depth, stacking and a short optimisation run.  Bar: max |got - ref| <= 1e-4 x the scale of each tensor (the bar of every training test
here); every comparison prints err / scale."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vss_f64 as V
from tests.training_cases import TOL, _bits, _close
from xpoint_amd import synth

pytestmark = pytest.mark.gpu
KEYS = ["out", "grad/x"] + ["grad/" + k for k in V.LEAVES]


def _u(name, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform("vss_gpu/" + name, shape, lo, hi))


def _scale_ok(scale, scaled, what):
    """scale = {S, 1 / S}, S a power of two, max|scaled| in [2^13, 2^14) (or all zero with S = 1)"""
    S, inv = (float(v) for v in scale.cpu())
    assert S > 0 and S * inv == 1.0 and np.frexp(S)[0] == 0.5, (what, S, inv)
    m = float(scaled.abs().max())
    assert (m == 0.0 and S == 1.0) or 2.0 ** 13 <= m < 2.0 ** 14, (what, m, S)
    return S, inv


# ---------------------------------------------------------------------------------------------------------------- the new kernels, one by one
@pytest.mark.parametrize("shape", [(1, 32), (35, 32), (257, 96), (70, 768)])
def test_layernorm_bwd(gpu_lib, shape):
    """(1, 32): one row; (35, 32): 8 rows per wave, a partial last wave; (257, 96): 24 of 32 lanes hold data, more rows than one part of the column
    sums (64 x 8 = 512 would be the second round; 257 leaves parts empty); (70, 768): three float4s per lane"""
    from xpoint_amd import training as T
    rows, C = shape
    x, dy = _u(f"ln/x{shape}", shape, -2.0, 3.0), _u(f"ln/dy{shape}", shape) * 1e-3
    gamma, beta = _u(f"ln/g{C}", (C,), 0.5, 1.5), _u(f"ln/b{C}", (C,))
    a, g, b = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    gx, gg, gb = torch.autograd.grad(F.layer_norm(a, (C,), g, b, 1e-5), [a, g, b], dy.double())
    dx, dg, db, sc = T.layernorm_bwd(dy.cuda(), x.cuda(), gamma.cuda())
    assert sc is None
    _close(dx, gx, f"layernorm_bwd {shape} dx")
    _close(dg, gg, f"layernorm_bwd {shape} dgamma")
    _close(db, gb, f"layernorm_bwd {shape} dbeta")
    dx2, dg2, db2, _ = T.layernorm_bwd(dy.cuda(), x.cuda(), gamma.cuda())
    assert torch.equal(_bits(dx), _bits(dx2)) and torch.equal(_bits(dg), _bits(dg2)) and torch.equal(_bits(db), _bits(db2)), "two calls differ"
    dx3, dg3, db3, _ = T.layernorm_bwd(dy.cuda(), x.cuda(), gamma.cuda(), want_params=False)
    assert dg3 is None and db3 is None and torch.equal(_bits(dx3), _bits(dx)), "dx depends on dgamma / dbeta being asked for"
    dxs, _, _, sc = T.layernorm_bwd(dy.cuda(), x.cuda(), gamma.cuda(), scaled=True)
    _, inv = _scale_ok(sc, dxs, f"layernorm_bwd {shape}")
    assert torch.equal(_bits(dxs * inv), _bits(dx)), "dx (1 / S) differs from the unscaled call"


@pytest.mark.parametrize("shape", [(1, 1, 1, 32), (2, 1, 5, 32), (2, 5, 7, 32), (1, 9, 4, 96), (3, 2, 2, 192)])
def test_dwconv3x3_silu_bwd(gpu_lib, shape):
    """(1, 1, 1, 32): every tap but the centre is outside; (2, 1, 5, 32): no vertical neighbour, two samples; (3, 2, 2, 192): every pixel on a corner"""
    from xpoint_amd import training as T
    B, H, W, C = shape
    x, dy = _u(f"dw/x{shape}", shape, -2.0, 2.0), _u(f"dw/dy{shape}", shape) * 1e-2
    w = _u(f"dw/w{C}", (C, 1, 3, 3), -0.6, 0.6)
    a, k = x.double().permute(0, 3, 1, 2).requires_grad_(True), w.double().requires_grad_(True)
    gx, gw = torch.autograd.grad(F.silu(F.conv2d(a, k, padding=1, groups=C)), [a, k], dy.double().permute(0, 3, 1, 2))
    w9c = w.reshape(C, 9).t().contiguous().cuda()
    dx, dw, sc = T.dwconv3x3_silu_bwd(x.cuda(), w9c, dy.cuda())
    assert sc is None and dw.shape == (9, C)
    _close(dx, gx.permute(0, 2, 3, 1), f"dwconv_bwd {shape} dx")
    _close(dw, gw.reshape(C, 9).t(), f"dwconv_bwd {shape} dw")
    dx2, dw2, _ = T.dwconv3x3_silu_bwd(x.cuda(), w9c, dy.cuda())
    assert torch.equal(_bits(dx), _bits(dx2)) and torch.equal(_bits(dw), _bits(dw2)), "two calls differ"
    for b in range(B):          # nothing crosses a sample boundary
        one, _, _ = T.dwconv3x3_silu_bwd(x[b:b + 1].cuda(), w9c, dy[b:b + 1].cuda(), want_dw=False)
        assert torch.equal(_bits(one[0]), _bits(dx[b])), f"sample {b}: dx depends on the batch neighbours"
    dxs, _, sc = T.dwconv3x3_silu_bwd(x.cuda(), w9c, dy.cuda(), scaled=True)
    _, inv = _scale_ok(sc, dxs, f"dwconv_bwd {shape}")
    assert torch.equal(_bits(dxs * inv), _bits(dx)), "dx (1 / S) differs from the unscaled call"


def test_gelu_fwd_is_the_dense_epilogue(gpu_lib):
    """fc1 (act 0) -> xp_gelu_fwd equals fc1 (act 1) of the inference path bit for bit; 35 rows: partial tiles"""
    from xpoint_amd import _lib, training as T
    from xpoint_amd.training import ops
    a, w, b = _u("gelu/a", (35, 32), -2.0, 2.0).cuda(), _u("gelu/w", (128, 32), -0.5, 0.5).cuda(), _u("gelu/b", (128,)).cuda()
    st = _lib.current_stream(a)
    pre, fused = ops._linear(a, w, st, bias=b), ops._linear(a, w, st, bias=b, act=1)
    got = T.gelu_fwd(pre)
    assert float(pre.min()) < -2.0 and float(pre.max()) > 2.0
    assert torch.equal(_bits(got), _bits(fused))
    _close(got, F.gelu(pre.double().cpu()), "gelu_fwd vs erf GELU in float64")
    odd = pre.reshape(-1)[1:4480 - 2]          # unaligned base, n % 4 != 0: the scalar form
    assert odd.data_ptr() % 16 == 4 and torch.equal(_bits(T.gelu_fwd(odd)), _bits(got.reshape(-1)[1:4480 - 2]))


def test_gelu_bwd(gpu_lib):
    from xpoint_amd import training as T
    n = 35 * 128
    x = torch.cat([torch.linspace(-8.0, 8.0, n - 3, dtype=torch.float64), torch.tensor([0.0, 30.0, -30.0], dtype=torch.float64)]).float()
    dy = _u("gelu/dy", (n,)) * 1e-3
    a = x.double().requires_grad_(True)
    (gx,) = torch.autograd.grad(F.gelu(a), [a], dy.double())
    dx, sc = T.gelu_bwd(dy.cuda(), x.cuda())
    assert sc is None
    _close(dx, gx, "gelu_bwd")
    assert float(dx[-2]) == float(dy[-2]) and float(dx[-1]) == 0.0 and float(dx[-3]) == 0.5 * float(dy[-3])          # +30, -30, 0
    dxs, sc = T.gelu_bwd(dy.cuda(), x.cuda(), scaled=True)
    _, inv = _scale_ok(sc, dxs, "gelu_bwd")
    assert torch.equal(_bits(dxs * inv), _bits(dx))
    assert torch.equal(_bits(T.gelu_bwd(dy.cuda()[1:n - 2], x.cuda()[1:n - 2])[0]), _bits(dx[1:n - 2])), "the scalar form differs"


@pytest.mark.parametrize("shape", [(2, 35, 32), (3, 7, 5), (1, 1, 4)])
def test_add_scaled_rows(gpu_lib, shape):
    """(3, 7, 5): 35 values per sample, no vector form"""
    from xpoint_amd import training as T
    B = shape[0]
    x, r = _u(f"asr/x{shape}", shape), _u(f"asr/r{shape}", shape)
    s = torch.tensor([1.25, 0.0, 0.75][:B])
    y = T.add_scaled_rows(x.cuda(), r.cuda(), s.cuda())
    ref = x + (s.view(B, 1, 1) * r)
    assert torch.equal(_bits(y.cpu()), _bits(ref)), "y = x + s r, each operation rounded once"
    g = T.add_scaled_rows(None, r.cuda(), s.cuda())
    assert torch.equal(_bits(g.cpu()), _bits(s.view(B, 1, 1) * r))
    if B > 1:
        assert torch.equal(_bits(y[1]), _bits(x[1].cuda())) and not bool(g[1].any()), "s = 0: the sample passes through / gets no gradient"


@pytest.mark.parametrize("n", [1, 255, 256, 4480, 1024 * 256 * 4 + 77])
def test_scale_grad(gpu_lib, n):
    """n = 1, 255: the tail row alone; 256: no tail; the last: more rows than the grid covers in one pass, plus a tail"""
    from xpoint_amd import training as T
    g = _u(f"sg/{n}", (n,))
    g[n // 2] = 0.9999
    for f in (2.0 ** -30, 1.0, 2.0 ** 10, 2.0 ** -80, 2.0 ** 80):
        gs, sc = T.scale_grad((g * f).cuda())
        S, inv = _scale_ok(sc, gs, f"scale_grad n={n} f={f:g}")
        assert S == 2.0 ** 14 / f and torch.equal(_bits(gs * inv), _bits((g * f).cuda()))
    z, sc = T.scale_grad(torch.zeros(n, device="cuda"))
    assert sc.tolist() == [1.0, 1.0] and not bool(z.any())
    h = (g * 3.0).cuda()
    want, _ = T.scale_grad(h)
    out, _ = T.scale_grad(h, out=h)
    assert out.data_ptr() == h.data_ptr() and torch.equal(_bits(h), _bits(want)), "in place"
    bad = g.clone().cuda()
    bad[0] = float("nan")
    if n > 1:
        bad[1] = float("inf")
    gs, sc = T.scale_grad(bad)
    assert bool(torch.isnan(gs[0])) and (n == 1 or bool(torch.isinf(gs[1]))), "non-finite values pass through"


# ---------------------------------------------------------------------------------------------------------------- the block
def _block(case, train=True, drop_path=0.0):
    from xpoint_amd import training as T
    (_, _, _, C), R, _, stage = V.CASES[case]
    blk = T.VSSBlock(C, dt_rank=R, drop_path=drop_path, stage=stage, block=0)
    blk.load_state_dict({V.prefix(case) + k: v for k, v in V.block_state(case, torch.float32).items()})
    return blk.cuda().train(train)


def _step(blk, x, Rw, **kw):
    """{'out', 'grad/x', 'grad/<leaf>'} of sum(out * Rw) on the GPU"""
    blk.zero_grad(set_to_none=True)
    x = x.detach().cuda().clone().requires_grad_(True)
    out = blk(x, **kw)
    (out * Rw.cuda()).sum().backward()
    res = {"out": out.detach(), "grad/x": x.grad}
    for k in V.LEAVES:
        g = blk.t(k).grad
        assert g is not None and g.shape == blk.t(k).shape, k
        res["grad/" + k] = g
    return res


@pytest.mark.parametrize("case", list(V.CASES))
def test_block_step(gpu_lib, case):
    x, Rw = V.case_inputs(case)
    got = _step(_block(case), x, Rw)
    ref = V.case_reference(case)
    for k in KEYS:
        _close(got[k], ref[k], f"{case}/{k} vs the restatement")
    if case in V.GOLDEN_CASES:          # the real reference's block: the CPU test's bars (1e-5 everywhere) widened to TOL
        golden = V.golden()
        for k in KEYS:
            _close(got[k], golden[f"{case}/{k}"], f"{case}/{k} vs the reference")


_DIR_ORDER = [0, 2, 1, 3]          # the fused core's route order (xpoint_amd/models.py)


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_eval_forward_equals_the_inference_path(gpu_lib, case):
    """VSSBlock.eval() under no_grad against the unfused launch sequence of xp_xpoint_forward (csrc/model.cpp: xp_layernorm, xp_gemm_nt_h2,
    xp_dwconv3x3_silu, xp_gemm_nt_h2, xp_ss2d_core_fwd, xp_gemm_nt_h2 + residual, xp_layernorm, fc1 with GELU, fc2 + residual) on the same weights"""
    from xpoint_amd import _lib as L
    from xpoint_amd.training import ops as T
    (B, H, W, C), R, _, _ = V.CASES[case]
    p = {k: v.cuda() for k, v in V.block_state(case, torch.float32).items()}
    x = V.case_inputs(case)[0].cuda()
    blk = _block(case, train=False)
    with torch.no_grad():
        got = blk(x)
    assert not got.requires_grad
    M, st = B * H * W, L.current_stream(x)
    X = x.reshape(M, C).clone()
    t1 = T._layernorm(X, p["norm.weight"], p["norm.bias"], st)
    t2 = T._linear(t1, p["op.in_proj.weight"], st)
    t3 = torch.empty_like(t2)
    L.call("xp_dwconv3x3_silu", L.ptr(t2), L.ptr(p["op.conv2d.weight"].reshape(C, 9).t().contiguous()), L.ptr(t3), B, H, W, C, st)
    xd = T._linear(t3, p["op.x_proj_weight"][_DIR_ORDER].reshape(4 * (R + 2), C).contiguous(), st)
    par = [p["op.dt_projs_weight"][_DIR_ORDER].permute(0, 2, 1).contiguous(), p["op.dt_projs_bias"][_DIR_ORDER].contiguous(),
           (-torch.exp(p["op.A_logs"])).view(4, C)[_DIR_ORDER].contiguous(), p["op.Ds"].view(4, C)[_DIR_ORDER].contiguous(),
           p["op.out_norm.weight"], p["op.out_norm.bias"]]
    nbytes = L.load().xp_ss2d_core_workspace_bytes(B, H, W, C)
    ws = torch.empty(nbytes // 4 + 16, device="cuda")
    yn = torch.empty_like(t3)
    L.call("xp_ss2d_core_fwd", L.ptr(t3), L.ptr(xd), *[L.ptr(t) for t in par], L.ptr(yn), L.ptr(ws), ctypes.c_size_t(nbytes), B, H, W, C, R, 1, 1e-5, st)
    X = T._linear(yn, p["op.out_proj.weight"], st, res=X)
    t1 = T._layernorm(X, p["norm2.weight"], p["norm2.bias"], st)
    hb = T._linear(t1, p["mlp.fc1.weight"], st, bias=p["mlp.fc1.bias"], act=1)
    X = T._linear(hb, p["mlp.fc2.weight"], st, bias=p["mlp.fc2.bias"], res=X)
    _close(got.reshape(M, C), X, f"{case}: eval forward vs the inference launch sequence")
    _close(got, V.case_reference(case)["out"], f"{case}: eval forward vs the restatement")


def test_two_steps_are_bit_identical(gpu_lib):
    x, Rw = V.case_inputs("A")
    blk = _block("A", drop_path=0.3)
    a = {k: v.clone() for k, v in _step(blk, x, Rw, seed=5).items()}
    b = _step(blk, x, Rw, seed=5)
    for k in KEYS:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_batch_neighbours(gpu_lib):
    """a sample's forward output is bit-equal to its single-sample run; its input gradient agrees within TOL (the power of two of each scaled
    gradient is taken per call, over the whole batch: bit equality of the gradient is measured and printed, not promised)"""
    x, Rw = V.case_inputs("A")
    blk = _block("A")
    both = {k: v.clone() for k, v in _step(blk, x, Rw).items()}
    for b in range(x.shape[0]):
        one = _step(blk, x[b:b + 1], Rw[b:b + 1])
        assert torch.equal(_bits(one["out"][0]), _bits(both["out"][b])), f"sample {b}: the output depends on the batch neighbours"
        _close(one["grad/x"][0], both["grad/x"][b], f"sample {b}: input gradient alone vs in the batch")
        print(f"sample {b}: input gradient bit-equal to the single-sample run: {torch.equal(_bits(one['grad/x'][0]), _bits(both['grad/x'][b]))}")


def test_gradient_range(gpu_lib):
    x, Rw = V.case_inputs("A")
    blk = _block("A")
    base = {k: v.clone() for k, v in _step(blk, x, Rw).items()}
    for f in (2.0 ** -30, 2.0 ** 10):
        got = _step(blk, x, Rw * f)
        for k in KEYS[1:]:
            _close(got[k], base[k].double() * f, f"dy x {f:g}: {k}")
    zero = _step(blk, x, torch.zeros_like(Rw))
    for k in KEYS[1:]:
        assert not bool(zero[k].any()), f"all-zero dy: {k} is not exactly zero"


def test_stochastic_depth(gpu_lib):
    from xpoint_amd.training import vss
    x, Rw = V.case_inputs("A")
    s1, s2 = torch.tensor([0.0, 1.25]), torch.tensor([1.25, 0.0])
    blk = _block("A", drop_path=0.2)
    got = _step(blk, x, Rw, drop_path_scale=(s1, s2))
    ref = V.vss_step64(V.block_state("A"), x, Rw, s1, s2)
    for k in KEYS:
        _close(got[k], ref[k], f"given factors: {k}")
    both0 = _step(blk, x, Rw, drop_path_scale=(torch.tensor([0.0, 1.25]), torch.tensor([0.0, 1.25])))
    assert torch.equal(_bits(both0["out"][0]), _bits(x[0].cuda())), "both factors 0: the sample must pass through"
    assert torch.equal(_bits(both0["grad/x"][0]), _bits(Rw[0].cuda()))
    # seeded draws: repeatable, and keyed by the sample id, not by the position in the batch
    B = 6
    xb = _u("sd/x", (B, 3, 4, 32))
    hi = _block("A", drop_path=0.5)
    with torch.no_grad():
        a, b = hi(xb.cuda(), seed=11), hi(xb.cuda(), seed=11)
        perm = torch.tensor([4, 2, 5, 0, 3, 1])
        c = hi(xb[perm].cuda(), seed=11, sample_ids=perm)
        other = hi(xb.cuda(), seed=12)
        hi.eval()
        plain = hi(xb.cuda(), seed=11)
    assert torch.equal(_bits(a), _bits(b)), "seeded draws are not repeatable"
    assert torch.equal(_bits(c), _bits(a[perm.cuda()])), "a sample's draw depends on its position in the batch"
    assert not torch.equal(a, other) and not torch.equal(a, plain), "the draws do not depend on the seed / eval mode scales"
    want = [vss._drop_path_draws(0.5, 11, range(B), br) for br in (0, 1)]
    assert {0.0, 2.0} == set(want[0] + want[1])
    with torch.no_grad():
        given = hi.train()(xb.cuda(), drop_path_scale=(torch.tensor(want[0]), torch.tensor(want[1])))
    assert torch.equal(_bits(given), _bits(a)), "the seeded forward is not the forward under its own factors"


def test_stacking_and_learning(gpu_lib):
    """two blocks in sequence — the second's input gradient flows into the first — lower an MSE loss in five Adam steps, and the tuned blocks change
    the inference model's encoder output"""
    from xpoint_amd import models, training as T
    cfg = synth.xpoint_exp1_config(64, 96, vssm={"EMBED_DIM": 32, "DEPTHS": [2, 1, 1, 1]})
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    net = net.to("cuda").eval()
    blocks = [T.VSSBlock.from_model(net, 0, j).cuda().train() for j in (0, 1)]
    assert blocks[1].drop_path > 0.0
    x, target = _u("learn/x", (2, 6, 9, 32)).cuda(), _u("learn/t", (2, 6, 9, 32)).cuda()
    # the first block's gradients through the second: against the float64 restatement of the pair
    ps = [{k: blk.t(k).detach().cpu().double().requires_grad_(True) for k in V.LEAVES} for blk in blocks]
    x64 = x.cpu().double().requires_grad_(True)
    y64 = V.vss_block64(ps[1], V.vss_block64(ps[0], x64))
    ref = torch.autograd.grad(((y64 - target.cpu().double()) ** 2).mean(), [x64] + [ps[0][k] for k in V.LEAVES])
    xg = x.clone().requires_grad_(True)
    ones = (torch.ones(2), torch.ones(2))
    ((blocks[1](blocks[0](xg, drop_path_scale=ones), drop_path_scale=ones) - target) ** 2).mean().backward()
    _close(xg.grad, ref[0], "stacked: input gradient")
    for k, r in zip(V.LEAVES, ref[1:]):
        _close(blocks[0].t(k).grad, r, f"stacked: first block grad/{k}")
    opt = torch.optim.Adam([p for blk in blocks for p in blk.parameters()], lr=1e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss = ((blocks[1](blocks[0](x, drop_path_scale=ones), drop_path_scale=ones) - target) ** 2).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print("losses:", " ".join(f"{v:.6f}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses          # five steps, each strictly lower
    images = _u("learn/img", (1, 1, 64, 96), 0.0, 1.0).cuda()
    before = net.forward_raw(images, want_prob=False, want_desc=False)["enc_nhwc"].clone()
    for blk in blocks:
        r = net.load_state_dict(blk.state_dict(), strict=False)
        assert not r.unexpected_keys
    after = net.forward_raw(images, want_prob=False, want_desc=False)["enc_nhwc"]
    assert bool(torch.isfinite(after).all()) and float((after - before).abs().max()) > 1e-4 * float(before.abs().max())


def test_refusals(gpu_lib):
    from xpoint_amd import _lib, training as T
    blk = _block("A")
    with pytest.raises(ValueError, match=r"\(B, H, W, 32\)"):
        blk(torch.zeros(1, 2, 3, 64, device="cuda"))
    with pytest.raises(ValueError):
        blk(torch.zeros(2, 3, 32, device="cuda"))
    with pytest.raises(TypeError, match="float32"):
        blk(torch.zeros(1, 2, 3, 32, device="cuda", dtype=torch.float16))
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        blk(torch.zeros(1, 2, 3, 32))
    with pytest.raises(ValueError):
        blk(torch.zeros(2, 2, 3, 32, device="cuda"), drop_path_scale=(torch.ones(3), torch.ones(2)))
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)          # noqa: E731
    with pytest.raises(ValueError, match="multiple of 4"):
        T.layernorm_bwd(z(3, 6), z(3, 6), z(6))
    with pytest.raises(ValueError, match="multiple of 4"):
        T.layernorm_bwd(z(3, 1028), z(3, 1028), z(1028))
    with pytest.raises(ValueError, match="multiple of 4"):
        T.dwconv3x3_silu_bwd(z(1, 2, 2, 6), z(9, 6), z(1, 2, 2, 6))
    with pytest.raises(ValueError):
        T.dwconv3x3_silu_bwd(z(1, 2, 2, 8), z(8, 9), z(1, 2, 2, 8))
    with pytest.raises(TypeError, match="float32"):
        T.layernorm_bwd(z(3, 8, dtype=torch.float16), z(3, 8), z(8))
    with pytest.raises(TypeError, match="float32"):
        T.gelu_bwd(z(8), z(8, dtype=torch.float64))
    with pytest.raises(ValueError):
        T.add_scaled_rows(z(2, 3, 4), z(2, 3, 4), z(3))
    # the C ABI itself: bad shapes and a short workspace are refused with a message
    a = z(3, 8)
    ws = torch.empty(8192, dtype=torch.uint8, device="cuda")
    for args in ((_lib.ptr(a), _lib.ptr(a), _lib.ptr(z(8)), _lib.ptr(z(3, 8)), None, None, 3, 6, 1e-5, None, _lib.ptr(ws), ctypes.c_size_t(8192), None),
                 (_lib.ptr(a), _lib.ptr(a), _lib.ptr(z(8)), _lib.ptr(z(3, 8)), None, None, 3, 8, 1e-5, None, _lib.ptr(ws), ctypes.c_size_t(64), None)):
        with pytest.raises(_lib.XPointHipError, match="xp_layernorm_bwd"):
            _lib.call("xp_layernorm_bwd", *args)
    with pytest.raises(_lib.XPointHipError, match="xp_dwconv3x3_silu_bwd"):
        _lib.call("xp_dwconv3x3_silu_bwd", _lib.ptr(a), _lib.ptr(a), _lib.ptr(a), _lib.ptr(z(3, 8)), None, 1, 1, 3, 6, None, _lib.ptr(ws),
                  ctypes.c_size_t(8192), None)
