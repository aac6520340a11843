"""Float64 restatements of the f32 class's glue operations (csrc/elementwise.hip, csrc/glue_core.h), torch on the CPU.  One plain function per operation, in
the kernels' own layouts (activations NHWC, depthwise weights [9][C], stem weights [9][Co]) and written from each operation's formula.
tests/test_cpu_glue_f64.py ties every one of them to torch's own float64 operator; tests/test_gpu_glue_f32.py holds the kernels to them."""
import math

import torch
import torch.nn.functional as F


def _gelu(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def layernorm(x, w, b, eps=1e-5, gelu=False):
    """(rows, C): (x - mean) / sqrt(biased variance + eps) * w + b, optionally followed by the exact (erf) GELU"""
    x = x.double()
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    y = (x - mu) / torch.sqrt(var + eps) * w.double() + b.double()
    return _gelu(y) if gelu else y


def dwconv3x3_silu(x, w9c):
    """x (B, H, W, C), w9c (9, C) tap-major: y[b, h, w, c] = silu(sum_{kh, kw} x[b, h + kh - 1, w + kw - 1, c] w9c[3 kh + kw, c]), zeros outside the image"""
    B, H, W, C = x.shape
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    acc = torch.zeros((B, H, W, C), dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            acc += xp[:, kh:kh + H, kw:kw + W, :] * w9c[3 * kh + kw].double()
    return acc / (1.0 + torch.exp(-acc))


def stem_conv_ln_gelu(img, w9co, bias, lnw, lnb, eps=1e-5):
    """img (B, H, W) gray, w9co (9, Co): 3x3 convolution with stride 2 and zero pad 1 (ceil(H / 2) x ceil(W / 2) outputs) + bias, LayerNorm over Co, erf-GELU;
    (B, Ho, Wo, Co)"""
    B, H, W = img.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = F.pad(img.double(), (1, 1, 1, 1))
    acc = bias.double().expand(B, Ho, Wo, -1).clone()
    for kh in range(3):
        for kw in range(3):
            acc += xp[:, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2, None] * w9co[3 * kh + kw].double()
    return layernorm(acc, lnw, lnb, eps, gelu=True)


def depth_to_space(x, bs):
    """out[n, bs h + i, bs w + j, c] = x[n, h, w, (bs i + j) Cq + c]: block-major channel order (not PixelShuffle's)"""
    B, H, W, C = x.shape
    Cq = C // (bs * bs)
    return x.reshape(B, H, W, bs, bs, Cq).permute(0, 1, 3, 2, 4, 5).reshape(B, H * bs, W * bs, Cq)


def softmax_shuffle(logits, r, mode=0):
    """logits (B, Hc, Wc, ld), the first r r + 1 columns used.  mode 0: softmax over the r r + 1 channels, the last one dropped; mode 1: exp(x) / (sum + 1e-5)
    over the same channels.  Then prob[b, r h + i, r w + j] = p[b, h, w, r i + j]; (B, r Hc, r Wc)."""
    B, Hc, Wc, _ = logits.shape
    z = logits[..., :r * r + 1].double()
    if mode == 0:
        e = torch.exp(z - z.max(dim=-1, keepdim=True).values)
        p = e / e.sum(dim=-1, keepdim=True)
    else:
        e = torch.exp(z)
        p = e / (e.sum(dim=-1, keepdim=True) + 1e-5)
    return p[..., :r * r].reshape(B, Hc, Wc, r, r).permute(0, 1, 3, 2, 4).reshape(B, Hc * r, Wc * r)


def l2norm_rows(x, eps):
    """(rows, C): x / max(|x|, eps); eps < 0: x / |x|"""
    x = x.double()
    n = torch.sqrt((x * x).sum(dim=-1, keepdim=True))
    return x / (n.clamp_min(eps) if eps >= 0 else n)


def nhwc_to_nchw(x):
    """(B, HW, C) -> (B, C, HW)"""
    return x.transpose(1, 2).contiguous()


def maxpool2(x):
    """(B, H, W, C) -> (B, H // 2, W // 2, C): the maximum of each whole 2 x 2 window; an odd last row / column is dropped"""
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    v = x[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C)
    return v.amax(dim=(2, 4))


def costvolume_mean(a, b):
    """a, b (B, hw, C): the mean over q of a[n][p] . b[n][q]; (B, hw)"""
    return torch.bmm(a.double(), b.double().transpose(1, 2)).mean(dim=2)


def u8_to_unit(src):
    """uint8 -> k / 255 rounded to float32"""
    return (src.double() / 255.0).float()
