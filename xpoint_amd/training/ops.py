"""The operator level of xpoint_amd.training: one wrapper per training kernel of the HIP library (csrc/train_dense.hip, csrc/train_dgrad.hip, csrc/train_regnet.hip,
csrc/train_vss.hip, csrc/train_ss2d.hip), the forward launches the autograd functions share, and the base of the three trainable modules.  There is no CPU fallback.

The public wrappers (`gemm_tn` ... `scale_grad`, re-exported by the package) check every operand — float32, on the GPU, one device — allocate outputs and
workspace and make ONE library call; the tests pin them one by one.  The underscore helpers are the forward engine's launches as the autograd functions
use them: no checks, the stream passed down.  Only the f32-grade class is built (split-fp16 operands, three products): activations must stay below 65504
in magnitude; a gradient operand is S x the gradient with the device float[2] {S, 1 / S} next to it (one power of two per operand): any finite range.

A linear layer's input gradient has TWO routes, and a layer never changes its route silently (the last bits differ): `_linear_dgrad`, the forward engine
on the transposed weight with 1 / S in the epilogue's scale vector, and `_linear_dgrad_tn`, the weight-gradient GEMM read the other way."""
import ctypes

import torch

from .. import _lib
from .._lib import ptr

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
L2_EPS = 1e-12           # F.normalize's default, as xp_xpoint_forward uses
LN_EPS = 1e-5
_NO_WS = object()


def _need_device(t, who):
    if not t.is_cuda:
        raise _lib.XPointHipError(f"{who}: tensors must live on the GPU (xpoint_amd has no CPU fallback)")


def _check_operands(who, *tensors):
    """Every tensor operand of an operator-level call: float32, on the GPU, all on the first one's device (None = an absent optional operand)."""
    tensors = [t for t in tensors if t is not None]
    for t in tensors:
        _need_device(t, who)
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: operands must be float32, got {t.dtype}")
        if t.device != tensors[0].device:
            raise _lib.XPointHipError(f"{who}: operands live on different devices ({tensors[0].device} and {t.device})")


def _vp(t, offset=0):
    """Pointer of element `offset` of a float32 device tensor whose rows are contiguous (column slices carry their ld separately); None stays None."""
    if t is None:
        return None
    assert t.is_cuda and t.dtype == torch.float32
    return ctypes.c_void_p(t.data_ptr() + 4 * offset)


def _launch(name, ref, stream, *args, ws=_NO_WS):
    """_lib.call(name, *args[, workspace pointer, workspace bytes], stream).  stream None: the current stream of `ref`'s device.  ws: the uint8
    workspace tensor the call ends with, or None for the (NULL, 0) of a call that needs none this time."""
    if ws is not _NO_WS:
        args += (ptr(ws), ctypes.c_size_t(0 if ws is None else ws.numel()))
    _lib.call(name, *args, _lib.current_stream(ref) if stream is None else stream)


def _f32(shape, dev):
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _scale_out(scaled, dev):
    """The device float[2] {S, 1 / S} a `scaled` call fills, else None."""
    return _f32(2, dev) if scaled else None


def _ws(dev, query, *dims):
    """The uint8 workspace that xp_<query>_workspace_bytes(*dims) asks for (256 bytes at least)."""
    return torch.empty(max(int(getattr(_lib.load(), f"xp_{query}_workspace_bytes")(*dims)), 256), dtype=torch.uint8, device=dev)


# ---- the public wrappers (what tests/test_gpu_head_training.py, test_gpu_regnet_training.py and test_gpu_vss_training.py pin one by one)
def gemm_tn(P, Q, out=None, p_scale=None, stream=None):
    """out[i][j] = sum_m P[m][i] Q[m][j].  P (M, I) the gradient operand, Q (M, J); both may be column slices of wider matrices (row stride
    = ld).  out: an (I, J) view with contiguous rows or None (allocated).  p_scale: None, or the device float[2] {S, 1 / S} of an operand that
    already holds S x the gradient."""
    _check_operands("gemm_tn", P, Q, out, p_scale)
    M, I = P.shape
    J = Q.shape[1]
    assert Q.shape[0] == M and P.stride(1) == 1 and Q.stride(1) == 1
    if out is None:
        out = _f32((I, J), P.device)
    assert out.shape == (I, J) and out.stride(1) == 1
    ws = _ws(P.device, "gemm_tn_h2", M, I, J)
    _launch("xp_gemm_tn_h2", P, stream, _vp(P), _vp(Q), _vp(out), M, I, J, int(P.stride(0)) if M > 1 else max(I, int(P.stride(0))),
            int(Q.stride(0)) if M > 1 else max(J, int(Q.stride(0))), int(out.stride(0)) if I > 1 else max(J, int(out.stride(0))), _vp(p_scale), ws=ws)
    return out


def _conv3x3_wgrad(who, kernel, pad_args, x, dy, dy_scale, stream, stride=1):
    """The three 3x3 weight gradients differ in the entry point, in the padding arguments it takes and in dy's grid: the input's, or its stride-2
    output grid."""
    _check_operands(who, x, dy, dy_scale)
    if stride == 1:
        if x.dim() != 4 or dy.dim() != 4 or tuple(dy.shape[:3]) != tuple(x.shape[:3]):
            raise ValueError(f"{who}: x {tuple(x.shape)} and dy {tuple(dy.shape)} do not share (B, H, W)")
    elif x.dim() != 4 or dy.dim() != 4 or min(x.shape) < 1 or tuple(dy.shape[:3]) != (x.shape[0], _s2_out(x.shape[1]), _s2_out(x.shape[2])):
        raise ValueError(f"{who}: dy {tuple(dy.shape)} is not the stride-2 output grid of x {tuple(x.shape)}")
    B, H, W, Ci = x.shape
    Co = dy.shape[-1]
    dw = _f32((Co, 3, 3, Ci), x.device)
    ws = _ws(x.device, "gemm_tn_h2", dy.shape[0] * dy.shape[1] * dy.shape[2], Co, 9 * Ci)
    _launch(kernel, x, stream, ptr(x), ptr(dy), ptr(dw), B, H, W, Ci, Co, *pad_args, _vp(dy_scale), ws=ws)
    return dw


def conv3x3_wgrad(x_nhwc, dy_nhwc, dy_scale=None, stride=1, reflect_pad=1, stream=None):
    """Weight gradient (Co, 3, 3, Ci) of the reflection-padded stride-1 3x3 convolution: x (B, H, W, Ci), dy (B, H, W, Co), contiguous."""
    return _conv3x3_wgrad("conv3x3_wgrad", "xp_conv3x3_wgrad_h2", (int(stride), int(reflect_pad)), x_nhwc, dy_nhwc, dy_scale, stream)


def conv3x3_wgrad_zero_pad(x_nhwc, dy_nhwc, dy_scale=None, stream=None):
    """Weight gradient (Co, 3, 3, Ci) of the stride-1 3x3 convolution with ZERO padding 1 (the RegNet head's): x (B, H, W, Ci), dy (B, H, W, Co)."""
    return _conv3x3_wgrad("conv3x3_wgrad_zero_pad", "xp_conv3x3_zp_wgrad_h2", (), x_nhwc, dy_nhwc, dy_scale, stream)


def _conv3x3_dgrad(who, kernel, query, dy, w, in_hw, dy_scale, stream):
    """The three 3x3 input gradients differ in the entry point, its workspace query and in whether dy's grid is the input's (in_hw None) or its
    stride-2 output grid."""
    _check_operands(who, dy, w, dy_scale)
    ok = dy.dim() == 4 and w.dim() == 4 and tuple(w.shape[:3]) == (dy.shape[-1], 3, 3)
    if in_hw is None:
        if not ok:
            raise ValueError(f"{who}: dy {tuple(dy.shape)} must be (B, H, W, Co) and w {tuple(w.shape)} (Co, 3, 3, Ci)")
        H, W = dy.shape[1:3]
    else:
        H, W = (int(v) for v in in_hw)
        if not ok or H < 1 or W < 1 or tuple(dy.shape[1:3]) != (_s2_out(H), _s2_out(W)):
            raise ValueError(f"{who}: dy {tuple(dy.shape)} must be (B, Ho, Wo, Co) of in_hw {(H, W)} and w {tuple(w.shape)} (Co, 3, 3, Ci)")
    B, Co, Ci = dy.shape[0], dy.shape[-1], w.shape[-1]
    dx = _f32((B, H, W, Ci), dy.device)
    _launch(kernel, dy, stream, ptr(dy), ptr(w), ptr(dx), B, H, W, Ci, Co, _vp(dy_scale), ws=_ws(dy.device, query, B, H, W, Ci, Co))
    return dx


def conv3x3_dgrad(dy_nhwc, w_ohwi, dy_scale=None, stream=None):
    """Input gradient (B, H, W, Ci) of the stride-1 zero-padded 3x3 convolution from dy (B, H, W, Co) and w (Co, 3, 3, Ci).  dy_scale: None, or
    the device float[2] {S, 1 / S} of a dy that already holds S x the gradient; the result is the unscaled gradient either way.  Co % 4 == 0."""
    return _conv3x3_dgrad("conv3x3_dgrad", "xp_conv3x3_dgrad_h2", "conv3x3_dgrad_h2", dy_nhwc, w_ohwi, None, dy_scale, stream)


def conv3x3_dgrad_reflect(dy_nhwc, w_ohwi, dy_scale=None, stream=None):
    """Input gradient (B, H, W, Ci) of the stride-1 REFLECTION-padded 3x3 convolution (the head trunk's) from dy (B, H, W, Co) and w (Co, 3, 3, Ci):
    conv3x3_dgrad's launch plus the frame terms that reflection folds back onto rows and columns 1 and n - 2.  dy_scale as conv3x3_dgrad's; the
    result is the unscaled gradient either way.  Co % 4 == 0; H, W >= 2."""
    return _conv3x3_dgrad("conv3x3_dgrad_reflect", "xp_conv3x3_rp_dgrad_h2", "conv3x3_rp_dgrad_h2", dy_nhwc, w_ohwi, None, dy_scale, stream)


def _s2_out(n):
    """Output length of the 3x3 stride-2 padding-1 convolution along an axis of n pixels."""
    return (n - 1) // 2 + 1


def conv3x3_s2_wgrad(x_nhwc, dy_nhwc, dy_scale=None, stream=None):
    """Weight gradient (Co, 3, 3, Ci) of the zero-padded STRIDE-2 3x3 convolution (patch embed, the downsamplers): x (B, H, W, Ci),
    dy (B, Ho, Wo, Co) with Ho = (H - 1) // 2 + 1, Wo = (W - 1) // 2 + 1, contiguous.  dy_scale as gemm_tn's p_scale."""
    return _conv3x3_wgrad("conv3x3_s2_wgrad", "xp_conv3x3_s2_wgrad_h2", (), x_nhwc, dy_nhwc, dy_scale, stream, stride=2)


def conv3x3_s2_dgrad(dy_nhwc, w_ohwi, in_hw, dy_scale=None, stream=None):
    """Input gradient (B, H, W, Ci) of the zero-padded STRIDE-2 3x3 convolution from dy (B, Ho, Wo, Co) and w (Co, 3, 3, Ci); in_hw = (H, W) of the
    input (Ho does not determine H).  dy_scale: None, or the device float[2] {S, 1 / S} of a dy that already holds S x the gradient; the result is the
    unscaled gradient either way.  Co % 4 == 0."""
    return _conv3x3_dgrad("conv3x3_s2_dgrad", "xp_conv3x3_s2_dgrad_h2", "conv3x3_s2_dgrad_h2", dy_nhwc, w_ohwi, in_hw, dy_scale, stream)


def conv3x3_s2_fwd(x_nhwc, w_ohwi, bias=None, stream=None):
    """conv3x3(zero_pad(x), stride 2) + bias on the split-fp16 engine, the inference path's launch of patch embed's second convolution and of the
    downsamplers: x (B, H, W, Ci), w (Co, 3, 3, Ci) -> (B, Ho, Wo, Co).  Ci % 4 == 0."""
    _check_operands("conv3x3_s2_fwd", x_nhwc, w_ohwi, bias)
    if x_nhwc.dim() != 4 or w_ohwi.dim() != 4 or tuple(w_ohwi.shape[1:]) != (3, 3, x_nhwc.shape[-1]) or x_nhwc.shape[-1] % 4:
        raise ValueError(f"conv3x3_s2_fwd: x {tuple(x_nhwc.shape)} must be (B, H, W, Ci) with Ci % 4 == 0 and w {tuple(w_ohwi.shape)} (Co, 3, 3, Ci)")
    B, H, W, Ci = x_nhwc.shape
    Co = w_ohwi.shape[0]
    y = _f32((B, _s2_out(H), _s2_out(W), Co), x_nhwc.device)
    wsplit = _split_h2(w_ohwi.reshape(Co, 9 * Ci), stream=stream)
    _launch("xp_conv3x3_nhwc_h2", x_nhwc, stream, ptr(x_nhwc), ctypes.c_void_p(wsplit.data_ptr()), ptr(y), ptr(bias), None, None, B, H, W, Ci, Co, 2, 0, 0)
    return y


def stem_conv(img, w9co, bias, stream=None):
    """The stem's convolution alone: img (B, 1, H, W) or (B, H, W), w9co (9, Co) the weight folded over the three identical input channels, bias
    (Co,) -> (B, Ho, Wo, Co).  The device definition the inference path fuses with LayerNorm and GELU.  Co 48 or 16."""
    _check_operands("stem_conv", img, w9co, bias)
    if img.dim() == 4 and img.shape[1] == 1:
        img = img[:, 0]
    if img.dim() != 3 or w9co.dim() != 2 or w9co.shape[0] != 9 or tuple(bias.shape) != (w9co.shape[1],) or min(img.shape) < 1:
        raise ValueError(f"stem_conv: img (B, 1, H, W), w9co (9, Co), bias (Co,); got {tuple(img.shape)}, {tuple(w9co.shape)}, {tuple(bias.shape)}")
    B, H, W = img.shape
    Co = w9co.shape[1]
    y = _f32((B, _s2_out(H), _s2_out(W), Co), img.device)
    _launch("xp_stem_conv", img, stream, ptr(img.contiguous()), ptr(w9co.contiguous()), ptr(bias.contiguous()), ptr(y), B, H, W, Co)
    return y


def stem_conv_wgrad(img, dy_nhwc, dy_scale=None, stream=None):
    """dw9co (9, Co) of the stem's convolution: img (B, 1, H, W) or (B, H, W), dy (B, Ho, Wo, Co); dy_scale {S, 1 / S}: dy holds S x the gradient.
    f64 accumulators in the fixed order of colsum_rows (which gives the bias gradient)."""
    _check_operands("stem_conv_wgrad", img, dy_nhwc, dy_scale)
    if img.dim() == 4 and img.shape[1] == 1:
        img = img[:, 0]
    if img.dim() != 3 or dy_nhwc.dim() != 4 or min(img.shape) < 1 or tuple(dy_nhwc.shape[:3]) != (img.shape[0], _s2_out(img.shape[1]), _s2_out(img.shape[2])):
        raise ValueError(f"stem_conv_wgrad: dy {tuple(dy_nhwc.shape)} is not the stride-2 output grid of img {tuple(img.shape)}")
    B, H, W = img.shape
    Co = dy_nhwc.shape[-1]
    dw = _f32((9, Co), img.device)
    _launch("xp_stem_conv_wgrad", img, stream, ptr(img.contiguous()), ptr(dy_nhwc.contiguous()), ptr(dw), B, H, W, Co, _vp(dy_scale),
            ws=_ws(img.device, "stem_conv_wgrad", Co))
    return dw


def bn_train_fwd(x, gamma, beta, eps=BN_EPS, y=None, stream=None):
    """x (rows, C) rows with any ld -> (y, save_mean (2, C), save_invstd, biased batch variance)."""
    _check_operands("bn_train_fwd", x, gamma, beta, y)
    rows, C = x.shape
    if gamma.shape != (C,) or beta.shape != (C,) or x.stride(1) != 1:
        raise ValueError(f"bn_train_fwd: gamma / beta must be ({C},) and the rows of x contiguous")
    dev = x.device
    if y is None:
        y = _f32((rows, C), dev)
    mean, invstd, var = _f32((2, C), dev), _f32(C, dev), _f32(C, dev)          # mean: the f32 mean and the f32 remainder of the f64 mean
    _launch("xp_bn_train_fwd", x, stream, _vp(x), int(x.stride(0)), ptr(gamma), ptr(beta), _vp(y), int(y.stride(0)), ptr(mean), ptr(invstd), ptr(var),
            rows, C, float(eps), ws=_ws(dev, "bn", C))
    return y, mean, invstd, var


def bn_train_bwd(dy, x, gamma, mean, invstd, relu_mask=False, scaled=False, dx=None, stream=None):
    """-> (dx, dgamma, dbeta, scale).  scaled: dx holds S x the gradient and scale = the device float[2] {S, 1 / S}; else scale is None."""
    _check_operands("bn_train_bwd", x, dy, gamma, mean, invstd, dx)
    rows, C = x.shape
    if dy.shape != x.shape or gamma.shape != (C,) or mean.shape != (2, C) or invstd.shape != (C,) or x.stride(1) != 1 or dy.stride(1) != 1:
        raise ValueError("bn_train_bwd: dy as x, gamma / invstd (C,), mean (2, C), contiguous rows")
    dev = x.device
    if dx is None:
        dx = _f32((rows, C), dev)
    dgamma, dbeta = _f32(C, dev), _f32(C, dev)
    scale = _scale_out(scaled, dev)
    _launch("xp_bn_train_bwd", x, stream, _vp(dy), int(dy.stride(0)), _vp(x), int(x.stride(0)), ptr(gamma), ptr(mean), ptr(invstd), _vp(dx),
            int(dx.stride(0)), ptr(dgamma), ptr(dbeta), ptr(scale), int(bool(relu_mask)), rows, C, ws=_ws(dev, "bn", C))
    return dx, dgamma, dbeta, scale


def colsum_rows(x, x_scale=None, stream=None):
    """out[c] = sum_r x[r][c] in the fixed order of the BatchNorm sums; x_scale {S, 1 / S}: x holds S x the values."""
    _check_operands("colsum_rows", x, x_scale)
    rows, C = x.shape
    out = _f32(C, x.device)
    _launch("xp_colsum_rows", x, stream, _vp(x), int(x.stride(0)), rows, C, _vp(x_scale), ptr(out), ws=_ws(x.device, "bn", C))
    return out


def _l2norm_rows(x, stream=None):
    """y = x / max(|x|, eps) over the rows of a contiguous x (rows, C): F.normalize, the inference path's launch."""
    y = torch.empty_like(x)
    _launch("xp_l2norm_rows", x, stream, ptr(x), ptr(y), x.shape[0], x.shape[1], float(L2_EPS))
    return y


def l2norm_rows_bwd(x, dy, eps=L2_EPS, stream=None):
    """Backward of y = x / max(|x|, eps) over the rows of x (rows, C)."""
    _check_operands("l2norm_rows_bwd", x, dy)
    rows, C = x.shape
    if dy.shape != x.shape:
        raise ValueError("l2norm_rows_bwd: dy must have the shape of x")
    dy = dy.contiguous()
    dx = _f32((rows, C), x.device)
    _launch("xp_l2norm_rows_bwd", x, stream, _vp(x), int(x.stride(0)), ptr(dy), ptr(dx), rows, C, float(eps))
    return dx


class _L2NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _l2norm_rows(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return l2norm_rows_bwd(x, dy)


def relu_bwd(dr, y, stream=None):
    """dy = dr where y > 0, else 0 (y: the ReLU's input, or its output)."""
    _check_operands("relu_bwd", dr, y)
    if dr.shape != y.shape:
        raise ValueError("relu_bwd: dr must have the shape of y")
    dr, y = dr.contiguous(), y.contiguous()
    dy = torch.empty_like(y)
    _launch("xp_relu_bwd", y, stream, ptr(dr), ptr(y), ptr(dy), y.numel())
    return dy


def maxpool2_relu_bwd(dpool, y_nhwc, stream=None):
    """Backward of max_pool2d(relu(y), 2): y (B, H, W, C), dpool (B, H // 2, W // 2, C) -> dy (B, H, W, C), torch's choice element for element."""
    _check_operands("maxpool2_relu_bwd", dpool, y_nhwc)
    B, H, W, C = y_nhwc.shape
    if tuple(dpool.shape) != (B, H // 2, W // 2, C):
        raise ValueError(f"maxpool2_relu_bwd: dpool {tuple(dpool.shape)} must be {(B, H // 2, W // 2, C)}")
    dy = torch.empty_like(y_nhwc, memory_format=torch.contiguous_format)
    _launch("xp_maxpool2_relu_bwd", y_nhwc, stream, ptr(dpool.contiguous()) if dpool.numel() else None, ptr(y_nhwc), ptr(dy), B, H, W, C)
    return dy


def costvolume_mean_bwd(a, b, dv, stream=None):
    """Backward of v[n][p] = a[n][p] . mean_q b[n][q]: a, b (B, hw, C), dv (B, hw) -> (da, db)."""
    _check_operands("costvolume_mean_bwd", a, b, dv)
    B, hw, C = a.shape
    if b.shape != a.shape or tuple(dv.shape) != (B, hw):
        raise ValueError("costvolume_mean_bwd: b as a (B, hw, C), dv (B, hw)")
    da, db = torch.empty_like(a, memory_format=torch.contiguous_format), torch.empty_like(a, memory_format=torch.contiguous_format)
    _launch("xp_costvolume_mean_bwd", a, stream, ptr(a), ptr(b), ptr(dv.contiguous()), ptr(da), ptr(db), B, hw, C)
    return da, db


def dropout_rows(x, p=0.5, seed=0, sample_ids=None, tag=0, mask=None, stream=None):
    """nn.Dropout(p) over the rows of x (rows, C) -> (y, mask (rows, C) uint8).  mask None: row r keeps column c iff the uniform draw of
    (seed, sample_ids[r], tag, c) is >= p (sample_ids: int32 device tensor, default 0 .. rows - 1), so a sample's mask does not depend on its batch
    neighbours; mask given: it is applied as it is (the backward pass; replaying recorded masks)."""
    _check_operands("dropout_rows", x)
    rows, C = x.shape
    x = x.contiguous()
    y = torch.empty_like(x)
    for t, what in ((mask, "mask"), (sample_ids, "sample_ids")):
        if t is not None:
            _need_device(t, "dropout_rows")
            if t.device != x.device:
                raise _lib.XPointHipError(f"dropout_rows: x and {what} live on different devices")
    if mask is not None:
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (rows, C):
            raise ValueError(f"dropout_rows: mask must be uint8 ({rows}, {C})")
        mask, use, ids = mask.contiguous(), 1, None
    else:
        mask, use = torch.empty((rows, C), dtype=torch.uint8, device=x.device), 0
        ids = torch.arange(rows, dtype=torch.int32, device=x.device) if sample_ids is None else sample_ids.to(torch.int32).contiguous()
        if tuple(ids.shape) != (rows,):
            raise ValueError(f"dropout_rows: sample_ids must be ({rows},)")
    _launch("xp_dropout_rows", x, stream, ptr(x), ptr(y), ctypes.c_void_p(mask.data_ptr()), use, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
            None if ids is None else ctypes.c_void_p(ids.data_ptr()), int(tag), float(p), rows, C)
    return y, mask


def scale_grad(g, out=None, stream=None):
    """-> (S g, scale): scale the device float[2] {S, 1 / S} with max|g| S in [2^13, 2^14) (S = 1 for an all-zero g): the operand format of a gradient
    that feeds gemm_tn (p_scale) or the forward engine (1 / S in the epilogue).  out: None (allocated), or a tensor of g's shape (g itself is allowed)."""
    _check_operands("scale_grad", g, out)
    g = g.contiguous()
    if out is None:
        out = torch.empty_like(g)
    if out.shape != g.shape or not out.is_contiguous():
        raise ValueError("scale_grad: out must be contiguous and have the shape of g")
    scale = _scale_out(True, g.device)
    _launch("xp_scale_grad", g, stream, ptr(g), ptr(out), g.numel(), ptr(scale), ws=_ws(g.device, "scale_grad"))
    return out, scale


def layernorm_bwd(dy, x, gamma, eps=LN_EPS, want_params=True, scaled=False, stream=None):
    """Backward of the LayerNorm over the rows of x (rows, C), x the forward's input -> (dx, dgamma, dbeta, scale).  want_params False: dgamma and
    dbeta are None.  scaled: dx holds S x the gradient and scale = the device float[2] {S, 1 / S}; else scale is None.  C % 4 == 0, C <= 1024."""
    _check_operands("layernorm_bwd", dy, x, gamma)
    if x.dim() != 2 or dy.shape != x.shape or tuple(gamma.shape) != (x.shape[1],):
        raise ValueError(f"layernorm_bwd: x (rows, C), dy as x, gamma (C,); got {tuple(x.shape)}, {tuple(dy.shape)}, {tuple(gamma.shape)}")
    rows, C = x.shape
    if C % 4 or C > 1024 or rows < 1:
        raise ValueError(f"layernorm_bwd: C must be a multiple of 4 up to 1024 and rows >= 1 (got rows = {rows}, C = {C})")
    dy, x, gamma = dy.contiguous(), x.contiguous(), gamma.contiguous()
    dev = x.device
    dx = torch.empty_like(x)
    dg, db = (_f32(C, dev), _f32(C, dev)) if want_params else (None, None)
    scale = _scale_out(scaled, dev)
    ws = _ws(dev, "layernorm_bwd", rows, C)
    _launch("xp_layernorm_bwd", x, stream, ptr(dy), ptr(x), ptr(gamma), ptr(dx), ptr(dg), ptr(db), rows, C, float(eps), ptr(scale), ws=ws)
    return dx, dg, db, scale


def dwconv3x3_silu_bwd(x_nhwc, w9c, dy_nhwc, want_dw=True, scaled=False, stream=None):
    """Backward of silu(depthwise conv3x3(x)) (zero padding 1, no bias): x, dy (B, H, W, C), w9c (9, C) -> (dx, dw9c, scale).  want_dw False: dw9c is
    None.  scaled: dx holds S x the gradient and scale = the device float[2] {S, 1 / S}; else scale is None.  C % 4 == 0."""
    _check_operands("dwconv3x3_silu_bwd", x_nhwc, w9c, dy_nhwc)
    if x_nhwc.dim() != 4 or dy_nhwc.shape != x_nhwc.shape or tuple(w9c.shape) != (9, x_nhwc.shape[-1]):
        raise ValueError(f"dwconv3x3_silu_bwd: x (B, H, W, C), dy as x, w9c (9, C); got {tuple(x_nhwc.shape)}, {tuple(dy_nhwc.shape)}, {tuple(w9c.shape)}")
    B, H, W, C = x_nhwc.shape
    if C % 4 or min(B, H, W) < 1:
        raise ValueError(f"dwconv3x3_silu_bwd: C must be a multiple of 4 and B, H, W >= 1 (got {tuple(x_nhwc.shape)})")
    x, w9c, dy = x_nhwc.contiguous(), w9c.contiguous(), dy_nhwc.contiguous()
    dev = x.device
    dx = torch.empty_like(x)
    dw = _f32((9, C), dev) if want_dw else None
    scale = _scale_out(scaled, dev)
    ws = _ws(dev, "dwconv3x3_silu_bwd", B, H, W, C)
    _launch("xp_dwconv3x3_silu_bwd", x, stream, ptr(x), ptr(w9c), ptr(dy), ptr(dx), ptr(dw), B, H, W, C, ptr(scale), ws=ws)
    return dx, dw, scale


def gelu_fwd(x, stream=None):
    """GELU (erf form) with the function of the dense engine's act = 1 epilogue: gemm (act 0) -> gelu_fwd equals gemm (act 1) bit for bit."""
    _check_operands("gelu_fwd", x)
    x = x.contiguous()
    y = torch.empty_like(x)
    if x.numel():
        _launch("xp_gelu_fwd", x, stream, ptr(x), ptr(y), x.numel())
    return y


def gelu_bwd(dy, x, scaled=False, stream=None):
    """dx = dy (Phi(x) + x phi(x)) -> (dx, scale).  scaled: dx holds S x the gradient and scale = {S, 1 / S}; else scale is None."""
    _check_operands("gelu_bwd", dy, x)
    if dy.shape != x.shape or not x.numel():
        raise ValueError("gelu_bwd: dy must have the shape of x, and x at least one element")
    dy, x = dy.contiguous(), x.contiguous()
    dx = torch.empty_like(x)
    scale = _scale_out(scaled, x.device)
    _launch("xp_gelu_bwd", x, stream, ptr(dy), ptr(x), ptr(dx), x.numel(), ptr(scale), ws=_ws(x.device, "scale_grad") if scaled else None)
    return dx, scale


def add_scaled_rows(x, r, s, stream=None):
    """y = x + s[b] r: r (B, ..., C) with one factor per sample, s (B,) float32; x None: y = s[b] r (the backward of the residual add under
    stochastic depth)."""
    _check_operands("add_scaled_rows", r, x, s)
    if r.dim() < 2 or tuple(s.shape) != (r.shape[0],) or (x is not None and x.shape != r.shape):
        raise ValueError(f"add_scaled_rows: r (B, ..., C), x None or as r, s (B,); got r {tuple(r.shape)}, s {tuple(s.shape)}")
    r = r.contiguous()
    x = None if x is None else x.contiguous()
    y = torch.empty_like(r)
    B, C = r.shape[0], r.shape[-1]
    _launch("xp_add_scaled_rows", r, stream, ptr(x), ptr(r), ptr(s.contiguous()), ptr(y), B, r.numel() // (B * C), C)
    return y


SS2D_CORES = ("routes", "pixel")


def check_ss2d_core(kind, who):
    """The name of a form of the training SS2D core: 'routes' (the cross-scan / selective-scan / cross-merge composition) or 'pixel' (ss2d_core)."""
    if kind not in SS2D_CORES:
        raise ValueError(f"{who}: ss2d_core must be 'routes' or 'pixel' (got {kind!r})")
    return kind


def ss2d_takes_pixel(B, H, W, C):
    """THE shapes the pixel form runs at under ss2d_core = 'pixel': every shape its entry points accept (DESIGN.md section 24 has the per-stage
    measurement); the others keep the composition, in the forward and the backward alike."""
    return 1 <= C <= 1024 and B <= 65535 and B * H * W * 4 * C < 2 ** 31


def _bc_view(xd, R):
    """The B / C entries of the x_proj rows xd (M, 4 (R + 2)) as the (M, 4, 2) view the kernels read in place."""
    M = xd.shape[0]
    assert xd.is_contiguous() and xd.shape[1] % 4 == 0 and xd.shape[1] // 4 == R + 2
    return xd.view(M, 4, R + 2)[:, :, R:]


def _ss2d_core_fwd(u, dtp, xd, R, A, Ds, dt_bias, dims, chunk, stream):
    """-> (ym (M, C), ws): the forward launch; ws holds what the backward needs of it and goes to _ss2d_core_bwd untouched."""
    B, H, W = dims
    M, C = u.shape
    bc = _bc_view(xd, R)
    ws = _ws(u.device, "ss2d_train", B, H, W, C, int(chunk))
    ym = _f32((M, C), u.device)
    _launch("xp_ss2d_train_fwd", u, stream, ptr(u), ptr(dtp), _vp(xd, R), int(bc.stride(0)), int(bc.stride(1)), ptr(A), ptr(Ds), ptr(dt_bias), ptr(ym),
            ptr(ws), ctypes.c_size_t(ws.numel()), B, H, W, C, 1, int(chunk))
    return ym, ws


def _ss2d_core_bwd(dym, u, dtp, xd, R, A, Ds, dt_bias, ws, dims, chunk, stream):
    """-> (du (M, C), ddtp (M, 4 C), dbc (M, 4, 2), dA, dD, ddt_bias (4, C) each): the backward launch on the forward's inputs and workspace."""
    B, H, W = dims
    M, C = u.shape
    bc = _bc_view(xd, R)
    dev = u.device
    du, ddtp, dbc = _f32((M, C), dev), _f32((M, 4 * C), dev), _f32((M, 4, 2), dev)
    dA, dD, ddb = _f32((4, C), dev), _f32((4, C), dev), _f32((4, C), dev)
    _launch("xp_ss2d_train_bwd", u, stream, ptr(u), ptr(dtp), _vp(xd, R), int(bc.stride(0)), int(bc.stride(1)), ptr(A), ptr(Ds), ptr(dt_bias), ptr(dym),
            ptr(du), ptr(ddtp), ptr(dbc), ptr(dA), ptr(dD), ptr(ddb), ptr(ws), ctypes.c_size_t(ws.numel()), B, H, W, C, 1, int(chunk))
    return du, ddtp, dbc, dA, dD, ddb


class _Ss2dCoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, dtp, xd, A, Ds, dt_bias, R, dims, chunk, stream):
        ym, ws = _ss2d_core_fwd(u, dtp, xd, R, A, Ds, dt_bias, dims, chunk, stream)
        ctx.args = (R, dims, chunk, stream)
        ctx.save_for_backward(u, dtp, xd, A, Ds, dt_bias, ws)
        return ym

    @staticmethod
    def backward(ctx, dym):
        u, dtp, xd, A, Ds, dt_bias, ws = ctx.saved_tensors
        R, dims, chunk, stream = ctx.args
        du, ddtp, dbc, dA, dD, ddb = _ss2d_core_bwd(dym.contiguous(), u, dtp, xd, R, A, Ds, dt_bias, ws, dims, chunk, stream)
        dxd = torch.zeros_like(xd)
        _bc_view(dxd, R).copy_(dbc)
        return du, ddtp.view(dtp.shape), dxd, dA.view(A.shape), dD.view(Ds.shape), ddb.view(dt_bias.shape), None, None, None, None


def ss2d_core(u, dtp, xd, R, A, Ds, dt_bias, dims, chunk=0, stream=None):
    """The SS2D core of a VSS block in pixel layout, one operator (csrc/train_ss2d.hip): cross-scan, the four-route selective scan (d_state 1) and
    cross-merge without a (B, 4, C, L) tensor.  dims = (B, H, W), M = B H W: u (M, C); dtp (M, 4 C) or (M, 4, C), the dt projection before bias and
    softplus; xd (M, 4 (R + 2)) the x_proj rows, whose B / C entries (columns R and R + 1 of each route's block) are read in place; A = -exp(A_logs),
    Ds, dt_bias: 4 C elements each, route-major -> ym (M, C).  Differentiable in u, dtp, the B / C entries of xd (the gradient of its dt entries is
    zero: they reach the core through dtp), A, Ds and dt_bias; the backward is the library's kernel only.  chunk: 0 (the library's choice) or a
    power of two in [2, 64] with chunk C <= 6144."""
    _check_operands("ss2d_core", u, dtp, xd, A, Ds, dt_bias)
    B, H, W = (int(v) for v in dims)
    R = int(R)
    if u.dim() != 2 or min(B, H, W) < 1 or u.shape[0] != B * H * W:
        raise ValueError(f"ss2d_core: u must be (B H W, C) of dims {tuple(dims)}, got {tuple(u.shape)}")
    M, C = u.shape
    if R < 0 or tuple(xd.shape) != (M, 4 * (R + 2)) or dtp.numel() != M * 4 * C or dtp.shape[0] != M:
        raise ValueError(f"ss2d_core: dtp must be ({M}, {4 * C}) and xd ({M}, {4 * (R + 2)}); got {tuple(dtp.shape)}, {tuple(xd.shape)}")
    if A.numel() != 4 * C or Ds.numel() != 4 * C or dt_bias.numel() != 4 * C:
        raise ValueError(f"ss2d_core: A, Ds and dt_bias must hold 4 C = {4 * C} elements")
    if not int(getattr(_lib.load(), "xp_ss2d_train_workspace_bytes")(B, H, W, C, int(chunk))):
        raise ValueError(f"ss2d_core: dims {(B, H, W)}, C = {C}, chunk = {chunk}: batch <= 65535, C <= 1024, B H W 4 C < 2^31, and chunk 0 or a power "
                         "of two in [2, 64] with chunk C <= 6144")
    with torch.cuda.device(u.device):
        return _Ss2dCoreFn.apply(u.contiguous(), dtp.contiguous(), xd.contiguous(), A.contiguous(), Ds.contiguous(), dt_bias.contiguous(), R, (B, H, W),
                                 int(chunk), stream)


# ---- the forward engine as the autograd functions launch it (no checks; the caller passes its stream down)
def _split_h2(w_nk, stream=None):
    N, K = w_nk.shape
    out = torch.empty(_lib.load().xp_split_weights_h2_bytes(N, K), dtype=torch.uint8, device=w_nk.device)
    _launch("xp_split_weights_h2", w_nk, stream, ptr(w_nk.contiguous()), ctypes.c_void_p(out.data_ptr()), N, K)
    return out


def _gemm_nt_h2(a, wsplit, N, K, out, bias=None, scale=None, shift=None, act=0, stream=None, res=None):
    """out (M, N; ld) = epilogue(a (M, K; ld) @ W^T) [+ res (M, N; ld)] on the forward's split-fp16 engine."""
    _launch("xp_gemm_nt_h2", a, stream, _vp(a), ctypes.c_void_p(wsplit.data_ptr()), _vp(out), ptr(bias), ptr(scale), ptr(shift), _vp(res),
            a.shape[0], N, K, int(a.stride(0)), int(out.stride(0)), 0 if res is None else int(res.stride(0)), act)
    return out


def _conv3x3_h2(x, w_ohwi, bias, scale=None, shift=None, stream=None):
    """relu(conv3x3(reflection_pad(x)) + bias) [* scale + shift]: the head trunk's launch of the inference path."""
    B, H, W, Ci = x.shape
    Co = w_ohwi.shape[0]
    y = _f32((B, H, W, Co), x.device)
    wsplit = _split_h2(w_ohwi.reshape(Co, 9 * Ci), stream=stream)
    _launch("xp_conv3x3_nhwc_h2", x, stream, ptr(x), ctypes.c_void_p(wsplit.data_ptr()), ptr(y), ptr(bias), ptr(scale), ptr(shift),
            B, H, W, Ci, Co, 1, 1, 2)
    return y


def _conv3x3_zp_h2(x, wsplit, Co, stream=None):
    """conv3x3(zero_pad(x)), no bias, no activation, on the split-fp16 engine: x (B, H, W, Ci), wsplit = _split_h2 of w (Co, 9 Ci)."""
    B, H, W, Ci = x.shape
    y = _f32((B, H, W, Co), x.device)
    _launch("xp_conv3x3_nhwc_h2", x, stream, ptr(x), ctypes.c_void_p(wsplit.data_ptr()), ptr(y), None, None, None, B, H, W, Ci, Co, 1, 0, 0)
    return y


def _relu(x, stream=None):
    y = torch.empty_like(x)
    _launch("xp_relu_fwd", x, stream, ptr(x), ptr(y), x.numel())
    return y


def _layernorm(x, w, b, stream):
    y = torch.empty_like(x)
    _lib.call("xp_layernorm", ptr(x), ptr(y), ptr(w.contiguous()), ptr(b.contiguous()), x.shape[0], x.shape[1], LN_EPS, 0, stream)
    return y


def _pad4(n):
    return (n + 3) // 4 * 4


def _transposed(x, cols=None):
    """x^T with contiguous rows of stride 1 (what `.t().contiguous()` does not promise when a dimension is 1); cols: rows zero-padded to that length."""
    n = x.shape[0]
    out = (torch.empty if cols in (None, n) else torch.zeros)((x.shape[1], cols or n), dtype=x.dtype, device=x.device)
    out[:, :n].copy_(x.t())
    return out


def _linear(a, w, stream, bias=None, res=None, act=0, scale=None, shift=None):
    """epilogue(a (M, K) w (N, K)^T) [+ res] on the forward engine: K % 4 == 0."""
    N, K = w.shape
    out = _f32((a.shape[0], N), a.device)
    return _gemm_nt_h2(a, _split_h2(w, stream=stream), N, K, out, bias=None if bias is None else bias.contiguous(), scale=scale, shift=shift, act=act,
                       stream=stream, res=res)


def _linear_dgrad(gs, scale, w, stream, res=None, out=None):
    """The input gradient g w [+ res] of a linear layer from gs = S g and scale = {S, 1 / S}: the forward engine on the transposed weight, 1 / S in
    the epilogue's scale vector.  w (N, K); gs (M, N) with N % 4 == 0 (the engine's reduction length here), or (M, pad4(N)) with pad columns the
    caller zeroed: they meet zero weight columns.  out: None (allocated) or an (M, K) column slice."""
    N, K = w.shape
    if out is None:
        out = _f32((gs.shape[0], K), gs.device)
    wsplit = _split_h2(_transposed(w, cols=gs.shape[1]), stream=stream)
    return _gemm_nt_h2(gs, wsplit, K, gs.shape[1], out, scale=scale[1:2].expand(K).contiguous(), shift=torch.zeros(K, dtype=torch.float32, device=gs.device),
                       stream=stream, res=res)


def _linear_dgrad_tn(dy, w, stream):
    """The input gradient dy w of a linear layer as the weight-gradient GEMM read the other way (reduction over the output features): its gradient
    operand takes one power of two per call, so any finite gradient range is accepted without a scaled copy.  The RegNet fc layers' route."""
    return gemm_tn(_transposed(dy), w.contiguous(), stream=stream)


# ---- the module base
class TrainModule(torch.nn.Module):
    """What the three trainable modules share: parameters and buffers under the reference's names, a copy of the module's slice of a loaded model,
    nn.BatchNorm2d's update of the running statistics."""

    prefix = ""          # what `t` puts in front of a key (VSSBlock: the block's place in the encoder)

    def t(self, key):
        """The parameter or buffer with the reference's name `prefix + key`."""
        mod, _, leaf = (self.prefix + key).rpartition(".")
        return getattr(self.get_submodule(mod), leaf)

    def _load_slice(self, sd, exempt="", strict=True):
        """Load this module's names from the state dict `sd` of a whole model; names ending in `exempt` may be absent (then strict must be False)."""
        own = self.state_dict()
        missing = [k for k in own if k not in sd and not (exempt and k.endswith(exempt))]
        if missing:
            raise RuntimeError(f"{type(self).__name__}.from_model: the model holds no {missing[:3]}")
        self.load_state_dict({k: sd[k] for k in own if k in sd}, strict=strict)
        return self

    def _update_running(self, stats, rows):
        """nn.BatchNorm2d's update of the buffers of every BatchNorm in stats = [(prefix, f32 batch mean (C,), biased batch variance (C,))], four
        launches in all."""
        with torch.no_grad():
            rm = [self.t(p + "running_mean") for p, _, _ in stats]
            rv = [self.t(p + "running_var") for p, _, _ in stats]
            torch._foreach_mul_(rm + rv, 1.0 - BN_MOMENTUM)
            torch._foreach_add_(rm, [m for _, m, _ in stats], alpha=BN_MOMENTUM)
            torch._foreach_add_(rv, [v for _, _, v in stats], alpha=BN_MOMENTUM * rows / (rows - 1.0))       # the running value is the unbiased variance
            torch._foreach_add_([self.t(p + "num_batches_tracked") for p, _, _ in stats], 1)
