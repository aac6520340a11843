"""A float64 restatement of the mixed-precision recipe (the fast class "amp16f" and its f32-container twin "amp16") for the kernels that are not GEMMs:
the fused SS2D core and the glue kernels of csrc/elementwise_f16.hip.  Test helper only: plain torch, no kernels.

Every rounding point of the recipe (oracle/xpoint_oracle.py, the AMP16 comment) is applied explicitly, and the helpers return the float64 value
BEFORE each rounding point together with a scale: the magnitude an f32 evaluation of that value errs against, so that a test can tell an element
whose rounding an f32 kernel may legitimately decide the other way (near an fp16 midpoint) from one it must reproduce bit for bit.

The recurrence runs on whatever device its inputs live on: the GPU tests run it on the device, the CPU tests on the host."""
import math

import torch
import torch.nn.functional as F

from oracle.xpoint_oracle import depth_to_space  # noqa: F401  (the glue restatement of depth_to_space is the oracle's own)

ORDER = [0, 2, 1, 3]          # the kernels' storage order of the four scan directions: a route pair's operands are adjacent


def r16(x):
    """fp16 rounding (round to nearest even) of a float64 value, kept in float64."""
    return x.double().float().half().double()


def spacing16(x):
    """fp16 spacing at |x| (the binade's ulp; 2^-24 in the subnormal range), built from its exponent bits: exact on every device."""
    _, e = torch.frexp(x.double().abs())
    return (((e.long() - 11).clamp_min(-24) + 1023) << 52).view(torch.float64)


def tie_distance(x):
    """Distance of x from the nearest fp16 rounding midpoint (midpoints of x's own binade)."""
    sp = spacing16(x)
    f = torch.frac(x.double().abs() / sp)
    return (f - 0.5).abs() * sp


def softplus64(dt):
    """torch's softplus with threshold 20 (csms6s.py:49-50)."""
    return torch.where(dt <= 20.0, torch.log1p(torch.exp(dt.clamp(max=20.0))), dt)


def scan64(u, delta, A, Bv, Cv, D):
    """The d_state 1 selective scan along dim 1 of (batch, L, K) tensors (A, D broadcast over L): h_t = exp(delta_t A) h_{t-1} + delta_t B_t u_t,
    y_t = C_t h_t + D u_t."""
    a = torch.exp(delta * A)
    bu = delta * Bv * u
    h = torch.zeros_like(a[:, 0])
    hs = torch.empty_like(a)
    for t in range(a.shape[1]):
        h = a[:, t] * h + bu[:, t]
        hs[:, t] = h
    return hs * Cv + D * u


def route_pixels(s, H, W, device="cpu"):
    """Pixel (h W + w) at sequence position i of the direction stored at index s: pairs 0 / 1 walk row- / column-major (l = w H + h), the second
    direction of a pair the flipped sequence (csm_triton.py:22-53)."""
    L = H * W
    i = torch.arange(L, device=device)
    l = L - 1 - i if s & 1 else i
    return (l % H) * W + torch.div(l, H, rounding_mode="floor") if s >> 1 else l


def ss2d_core_amp64(u16, xdbl16, wdt16, dtb, A, D, lnw, lnb, H, W, eps=1e-5):
    """The fused SS2D core of the recipe in float64, in the kernels' layout: u16 (B, H, W, C) and xdbl16 (B H W, 4 (R + 2)) hold fp16 values,
    wdt16 (4, R, C) fp16 values, dtb / A (= -exp(A_logs)) / D (4, C) f32; directions stored in the order (0, 2, 1, 3).
    Returns (on64, dt_margin):
      on64       (B, H, W, C) out_norm's value before the final .to(half) (VMamba.py:646);
      dt_margin  (B, H W, 4, C) for every dt: the distance of the float64 projection sum from the nearest fp16 midpoint, in units of the sum of
                 |w x| over the dt_rank terms (the scale an f32 evaluation of the sum errs against).  A dt with a margin of a few 2^-24 x dt_rank
                 may round the other way in f32.
    Steps: dt = r16(sum_r w x) rounded BEFORE the f32 bias is added (csms6s.py:47-50); softplus, threshold 20; exp(delta A); the recurrence;
    merge (y0 + y2) + (y1 + y3) (csm_triton.py:60-62); LayerNorm over C (VMamba.py:644)."""
    B, _, _, C = u16.shape
    L = H * W
    R = wdt16.shape[1]
    dev = u16.device
    u = u16.double().reshape(B, L, 1, C)
    xd = xdbl16.double().reshape(B, L, 4, R + 2)
    w = wdt16.double()
    dt_pre = torch.einsum("blsr,src->blsc", xd[..., :R], w)
    dt_abs = torch.einsum("blsr,src->blsc", xd[..., :R].abs(), w.abs())
    dt_margin = tie_distance(dt_pre) / dt_abs.clamp_min(2.0 ** -60)
    delta = softplus64(r16(dt_pre) + dtb.double())
    Bv, Cv = xd[..., R:R + 1], xd[..., R + 1:R + 2]
    ys = torch.empty((B, L, 4, C), dtype=torch.float64, device=dev)
    for s in range(4):
        pix = route_pixels(s, H, W, dev)
        ys[:, pix, s] = scan64(u[:, pix, 0], delta[:, pix, s], A[s].double(), Bv[:, pix, s], Cv[:, pix, s], D[s].double())
    y = (ys[:, :, 0] + ys[:, :, 1]) + (ys[:, :, 2] + ys[:, :, 3])          # stored (0, 2, 1, 3): (y0 + y2) + (y1 + y3)
    on = F.layer_norm(y, (C,), lnw.double(), lnb.double(), eps)
    return on.reshape(B, H, W, C), dt_margin


def xdbl_amp64(u16, xw16):
    """x_proj of the recipe (a half conv1d): r16(u16 . xw16^T) from the float64 product; u16 (M, C), xw16 (4 (R + 2), C)."""
    return r16(u16.double() @ xw16.double().t())


# ------------------------------------------------------------------------------------------------------------------------------ glue kernels
def _ln_point(x, w, b, eps):
    """LayerNorm over the last dim of fp16-valued x: (value, scale).  The scale is what the f32 two-pass statistics err against: the normalised
    term, the bias, and a quarter of the row's mean magnitude in units of its standard deviation (the rounding of the mean, seen through rstd)."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    xh = d * rstd
    v = xh * w.double() + b.double()
    scale = (xh.abs() + 0.25 * x.abs().mean(-1, keepdim=True) * rstd) * w.double().abs() + b.double().abs()
    return v, scale


def layernorm_f16_64(x16, w, b, eps=1e-5):
    """xp_layernorm_f16: half in, statistics and affine in f32, half out (VMamba.py:1222-1234).  [(value, scale)] of its one rounding point."""
    return [_ln_point(x16, w, b, eps)]


def dwconv_silu_f16_64(x16, w9c):
    """xp_dwconv3x3_silu_f16: x16 (B, H, W, C) fp16 values, w9c (9, C) (tap kh 3 + kw, fp16 values); depthwise 3x3, zero padding 1, no bias
    (VMamba.py:657) -> r16 -> SiLU (:658) -> r16.  [(conv, sum |x w|), (SiLU(r16(conv)), |SiLU|)], NHWC."""
    C = x16.shape[-1]
    xin = x16.double().permute(0, 3, 1, 2)
    wt = w9c.double().t().reshape(C, 1, 3, 3)
    conv = F.conv2d(xin, wt, None, padding=1, groups=C).permute(0, 2, 3, 1)
    cabs = F.conv2d(xin.abs(), wt.abs(), None, padding=1, groups=C).permute(0, 2, 3, 1)
    s = F.silu(r16(conv))
    return [(conv, cabs), (s, s.abs())]


def stem_f16_64(img, w, b, lnw, lnb, eps=1e-5, kappa=4e-7):
    """The first three layers of patch_embed under the recipe (VMamba.py:1405-1416, the gray image repeated to three identical channels,
    :1509-1510): conv3x3 stride 2 padding 1 with r16 input, weights and bias -> r16 -> LayerNorm over the CO channels -> r16 -> exact-erf GELU -> r16.
    img (B, 1, H, W), w (CO, 3, 3, 3).  [(conv, sum |x w| + |b|), LayerNorm point, (GELU, max(1, |x|))], NHWC (B, ceil(H/2), ceil(W/2), CO).
    The GELU point's scale is the form of xp_gelu_fast's stated error, <= 4e-7 max(1, |x|).
    A conv value within kappa x scale of an fp16 midpoint may round either way in f32, and the way it goes moves the LayerNorm statistics of its whole
    pixel, i.e. every channel's output: such values take the direction of the f32 evaluation the kernel does (three input channels' weights folded to
    f32, taps in order by fma, then the bias), so that the other channels of the pixel stay decidable."""
    x = r16(img).repeat(1, 3, 1, 1)
    w16, b16 = r16(w), r16(b)
    conv = F.conv2d(x, w16, b16, stride=2, padding=1).permute(0, 2, 3, 1)
    cabs = (F.conv2d(x.abs(), w16.abs(), None, stride=2, padding=1) + b16.abs()[None, :, None, None]).permute(0, 2, 3, 1)
    B, Ho, Wo, CO = conv.shape
    taps = F.unfold(r16(img), 3, padding=1, stride=2)                     # (B, 9, Ho Wo), tap kh 3 + kw
    wf = w16.sum(dim=1).float().double().reshape(CO, 9)
    acc = torch.zeros((B, CO, Ho * Wo), dtype=torch.float64, device=conv.device)
    for t in range(9):                                                   # fma: the product is exact in float64, one rounding to f32
        acc = (taps[:, t:t + 1] * wf[:, t, None] + acc).float().double()
    acc = (acc + b16[:, None]).float().double().permute(0, 2, 1).reshape(conv.shape)
    c16 = torch.where(tie_distance(conv) <= kappa * cabs, r16(acc), r16(conv))
    ln, lscale = _ln_point(c16, lnw, lnb, eps)
    x3 = r16(ln)
    g = 0.5 * x3 * (1.0 + torch.erf(x3 / math.sqrt(2.0)))
    return [(conv, cabs), (ln, lscale), (g, x3.abs().clamp_min(1.0))]


def assert_r16_exact_off_ties(name, got16, points, kappa, max_tie_frac=0.01):
    """got16: the kernel's fp16 output; points: [(value64, scale64)] of every rounding point, the last one the output's.  An element is NEAR A TIE
    if the value at any of its rounding points lies within kappa x scale of an fp16 midpoint (kappa states the kernel's f32 error bound).  Elements
    that are not must be bit-equal to r16(last value); near-tie elements within one fp16 ulp (two where there are several rounding points: a value
    rounded the other way at an earlier point moves the output by one ulp times the slope of the later steps) beyond the last point's own error
    window kappa x scale; and the near-tie fraction must stay <= max_tie_frac (or a handful of elements, 8 / n, on tiny outputs), so that a loose
    kappa cannot hollow the test out.  Prints one line in the style of test_gpu_model.py's check() and returns its numbers."""
    got = got16.double().reshape(-1)
    want = r16(points[-1][0]).reshape(-1).to(got.device)
    near = torch.zeros_like(got, dtype=torch.bool)
    for v, s in points:
        near |= (tie_distance(v) <= kappa * s).reshape(-1).to(got.device)
    same = got == want
    window = kappa * points[-1][1].reshape(-1).to(got.device)
    ulps = ((got - want).abs() - window).clamp_min(0) / spacing16(torch.maximum(got.abs(), want.abs()))
    eq, tie, worst = float(same.double().mean()), float(near.double().mean()), float(ulps.max())
    off_bad = int((~same & ~near).sum())
    print(f"{name:44s} bit-equal {eq:.5f}, near-tie {tie:.5f}, worst {worst:.2f} fp16 ulp, off-tie mismatches {off_bad}")
    assert off_bad == 0, f"{name}: {off_bad} elements away from any fp16 tie differ from the recipe"
    assert worst <= (1.0 if len(points) == 1 else 2.0), f"{name}: worst {worst:.2f} fp16 ulp"
    assert tie <= max(max_tie_frac, 8 / got.numel()), f"{name}: {tie:.4f} of the elements are near a tie: kappa = {kappa} is too loose for this data"
    return eq, tie, worst
