"""tests/amp_recipe64.py — the float64 restatement of the mixed-precision recipe that tests/test_gpu_amp16f_kernels.py holds the fp16-storage kernels to —
pinned without a GPU: against the REAL reference's half tensors (g20: its first VSS block and patch_embed under float16 autocast, each op fed the
reference's input tap), against the oracle's AMP16 switch at deep-stage shapes, and its recurrence against scan_fwd64 (pinned by gradcheck and g26)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import xpoint_oracle as xo
from tests import amp_recipe64 as rc
from tests.test_cpu_scan_grad import scan_fwd64
from xpoint_amd import synth


def _check(name, mine, ref, frac=0.999, ulps=1.01):
    """The bars of test_cpu_parity_tools.py::test_oracle_amp16_recipe_vs_reference_taps: the bit-equal fraction, and the worst error in fp16 ulps of the
    reference floored at its rms."""
    mine, ref = mine.double(), ref.double()
    eq = float((mine == ref).double().mean())
    ulp = torch.clamp(ref.abs(), min=float(ref.pow(2).mean().sqrt())) * 2.0 ** -10
    worst = float(((mine - ref).abs() / ulp).max())
    print(f"{name:40s} bit-equal {eq:.5f}, worst {worst:.2f} fp16 ulp")
    assert eq >= frac and worst <= ulps, (name, eq, worst)


def _core64(sd, pre, u16):
    """ss2d_core_amp64 on u16 (B, H, W, C) with the layer's weights, x_proj evaluated as the recipe's half conv1d."""
    _, H, W, C = u16.shape
    R = sd[pre + "dt_projs_weight"].shape[2]
    o = rc.ORDER
    xdbl = rc.xdbl_amp64(u16.reshape(-1, C), rc.r16(sd[pre + "x_proj_weight"][o].reshape(4 * (R + 2), C)))
    A = -torch.exp(sd[pre + "A_logs"].float())                   # f32, as the recipe computes it (VMamba.py:619)
    return rc.ss2d_core_amp64(u16, xdbl, rc.r16(sd[pre + "dt_projs_weight"])[o].permute(0, 2, 1), sd[pre + "dt_projs_bias"].reshape(4, C)[o],
                              A.reshape(4, C)[o], sd[pre + "Ds"].reshape(4, C)[o], sd[pre + "out_norm.weight"], sd[pre + "out_norm.bias"], H, W)


def test_recipe64_reproduces_the_reference_taps(golden):
    g = golden("g20_mixed_precision_fp16.npz")
    tp = lambda k: torch.from_numpy(g[f"64x96/tap/{k}"].astype(np.float64))
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(synth.xpoint_exp1_config(64, 96)).items()}
    p = "encoder.layers.0.blocks.0."
    x = tp("b0.norm/in")
    C = x.shape[-1]
    _check("norm (LayerNorm)", rc.r16(rc.layernorm_f16_64(x, sd[p + "norm.weight"], sd[p + "norm.bias"])[-1][0]), tp("b0.norm/out"))
    w9c = rc.r16(sd[p + "op.conv2d.weight"]).reshape(C, 9).t()
    dw = rc.dwconv_silu_f16_64(tp("b0.conv2d/in").permute(0, 2, 3, 1), w9c)          # the reference runs the depthwise conv in NCHW
    _check("conv2d + SiLU", rc.r16(dw[-1][0]), tp("b0.act/out").permute(0, 2, 3, 1), ulps=2.01)        # two rounding points
    on64, _ = _core64(sd, p + "op.", tp("b0.act/out").permute(0, 2, 3, 1).contiguous())
    _check("SS2D core output .to(half)", rc.r16(on64), rc.r16(tp("b0.out_norm/out")))
    q = "encoder.patch_embed."
    st = rc.stem_f16_64(tp("patch_embed/in")[:, :1], sd[q + "0.weight"], sd[q + "0.bias"], sd[q + "2.weight"], sd[q + "2.bias"])
    s1 = rc.r16(st[-1][0]).permute(0, 3, 1, 2)
    c2 = rc.r16(F.conv2d(s1, rc.r16(sd[q + "5.weight"]), rc.r16(sd[q + "5.bias"]), stride=2, padding=1)).permute(0, 2, 3, 1)
    pe = rc.layernorm_f16_64(c2, sd[q + "7.weight"], sd[q + "7.bias"])
    # five rounding points and a 432-term f32 convolution in the reference: measured 0.9918 bit-equal, 1.23 ulps (the GPU taps bar is 0.97 / 3)
    _check("patch_embed (stem, conv, LN)", rc.r16(pe[-1][0]), tp("patch_embed/out"), frac=0.99, ulps=2.01)


@pytest.mark.parametrize("C,R,H,W", [(384, 24, 5, 7), (768, 48, 3, 4)])
def test_recipe64_core_matches_the_oracle_amp16_switch(C, R, H, W):
    """The deep-stage ranks (dt_rank 24 / 48) against xo.ss2d_core under AMP16 (f32 arithmetic between the same rounding points)."""
    pre = "op."
    u = lambda name, shape, lo, hi: torch.from_numpy(synth.uniform(f"amp64/{name}{C}", shape, lo, hi))
    sd = {pre + "x_proj_weight": u("xp", (4, R + 2, C), -C ** -0.5, C ** -0.5), pre + "dt_projs_weight": u("dtw", (4, C, R), -R ** -0.5, R ** -0.5),
          pre + "dt_projs_bias": u("dtb", (4, C), -6.9, -2.25), pre + "A_logs": u("al", (4 * C, 1), -0.5, 0.5), pre + "Ds": u("ds", (4 * C,), 0.5, 1.5),
          pre + "out_norm.weight": u("onw", (C,), 0.8, 1.2), pre + "out_norm.bias": u("onb", (C,), -0.1, 0.1)}
    x16 = u("x", (2, C, H, W), -0.3, 1.0).half().float()
    xo.AMP16 = True
    try:
        with torch.no_grad():
            ref = xo.ss2d_core(x16, sd, pre)
    finally:
        xo.AMP16 = False
    on64, _ = _core64(sd, pre, x16.permute(0, 2, 3, 1).double())
    _check(f"SS2D core C {C} R {R} vs oracle AMP16", rc.r16(on64), ref)


def test_recipe64_scan_matches_scan_fwd64():
    b, d, L = 2, 6, 41
    u = lambda name, shape, lo, hi: torch.from_numpy(synth.uniform("amp64/scan/" + name, shape, lo, hi)).double()
    x, dl, bias = u("u", (b, d, L), -1.0, 1.0), u("dl", (b, d, L), -3.0, 3.0), u("bias", (d,), -4.0, 22.0)     # delta on both sides of the threshold 20
    A, D = -torch.exp(u("A", (d, 1), -1.0, 1.0)), u("D", (d,), 0.5, 1.5)
    Bm, Cm = u("B", (b, 1, 1, L), -1.0, 1.0), u("C", (b, 1, 1, L), -1.0, 1.0)
    ref = scan_fwd64(x, dl, A, Bm, Cm, D, bias)
    delta = rc.softplus64(dl + bias[:, None]).transpose(1, 2)
    mine = rc.scan64(x.transpose(1, 2), delta, A[:, 0], Bm[:, 0, 0, :, None], Cm[:, 0, 0, :, None], D).transpose(1, 2)
    assert torch.allclose(mine, ref, rtol=1e-12, atol=1e-13), float((mine - ref).abs().max())


def test_recipe64_routes_and_ties():
    """The route order is the oracle's cross-scan (directions stored (0, 2, 1, 3)); the tie arithmetic on known values."""
    for H, W in ((1, 1), (3, 5), (7, 4), (16, 24)):
        for s in range(4):
            assert np.array_equal(rc.route_pixels(s, H, W).numpy(), xo._route_pixels(rc.ORDER[s], 0, H, W)), (H, W, s)
    v = torch.tensor([1 + 2 ** -11, 1.0, 2.0 ** -25, 3 * 2.0 ** -25, 65504.0, -(1 + 3 * 2 ** -11)], dtype=torch.float64)
    assert rc.tie_distance(v).tolist() == [0.0, 2 ** -11, 0.0, 0.0, 16.0, 0.0]
    assert rc.r16(v).tolist() == [1.0, 1.0, 0.0, 2.0 ** -23, 65504.0, -(1 + 2 ** -9)]
