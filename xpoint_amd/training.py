"""Head fine-tuning over a frozen encoder: the detector and descriptor heads of the reference's XPoint (XPoint.py:112-138, 348-371) in
training mode, forward and backward on the HIP library (csrc/train_dense.hip).

    heads = training.XPointHeads.from_model(net).cuda().train()
    optimizer = torch.optim.Adam(heads.parameters(), lr=1e-3)
    loss, components = training.finetune_step(net, heads, data, losses.XPointLoss(cfg), optimizer)
    net.load_state_dict(heads.state_dict(), strict=False)        # the inference model with the tuned heads

`XPointHeads` carries the reference's parameter and buffer names, so its `state_dict()` is a slice of the reference's checkpoint.  Each
head is [ReflectionPad, Conv3x3, ReLU, BatchNorm, Conv1x1, BatchNorm] (+ F.normalize on the descriptor); both trunk convolutions run as the
one Ci -> 512 launch of the inference path.  In `.train()` BatchNorm uses the statistics of the batch and updates the running ones as
nn.BatchNorm2d does (momentum 0.1, eps 1e-5, unbiased variance for the running value); in `.eval()` it uses the running statistics and the
forward is the inference path's launches.  The backward is three `torch.autograd.Function`s whose dense arithmetic is HIP only: weight
gradients by xp_conv3x3_wgrad_h2 / xp_gemm_tn_h2, BatchNorm by xp_bn_train_bwd, bias gradients by xp_colsum_rows, the 1x1 layers' input
gradient by xp_gemm_nt_h2 on the transposed weight, F.normalize by xp_l2norm_rows_bwd.  Torch only concatenates / permutes parameters and
gradients.  There is no CPU fallback and no gradient for the encoder: an `enc_nhwc` that requires grad raises NotImplementedError.

Only the f32-grade class is built (split-fp16 operands, three products): activations must stay below 65504 in magnitude (the encoder output
and the trunk's BatchNorm output: O(1) in this network); gradients of any finite range are accepted (one power of two per operand).
`RegNetHead` is the homography regression head (reference RegNet.py) behind the same frozen encoder: two zero-padded 3x3 convolutions in the order
conv -> BatchNorm -> ReLU, max pool, F.normalize, the cost volume's global mean, and two linear layers with dropout.  Its backward adds the zero-padded
convolution's weight gradient (xp_conv3x3_zp_wgrad_h2) and INPUT gradient (xp_conv3x3_dgrad_h2: the forward engine on the rotated, transposed weight),
the ReLU / max-pool gates on the BatchNorm output, the cost volume's backward and a counter-based dropout.
`VSSBlock` is one block of the VMamba encoder (reference VMamba.py:1153-1234) as a trainable module: LayerNorm, in_proj, depthwise conv + SiLU, x_proj,
the dt projection, the SS2D core composed from the differentiable cross-scan / selective-scan / cross-merge operators, out_norm, out_proj and the MLP,
with stochastic depth.  Its backward is HIP only and passes the gradient through to its input, so blocks stack.
Not built: the gradient of patch embed / downsample / the head trunk's input, autocast / GradScaler training, a training command line."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import ptr

__all__ = ["XPointHeads", "RegNetHead", "finetune_step", "gemm_tn", "conv3x3_wgrad", "bn_train_fwd", "bn_train_bwd", "colsum_rows", "l2norm_rows_bwd",
           "conv3x3_wgrad_zero_pad", "conv3x3_dgrad", "relu_bwd", "maxpool2_relu_bwd", "costvolume_mean_bwd", "dropout_rows",
           "VSSBlock", "layernorm_bwd", "dwconv3x3_silu_bwd", "gelu_fwd", "gelu_bwd", "add_scaled_rows", "scale_grad"]

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
L2_EPS = 1e-12           # F.normalize's default, as xp_xpoint_forward uses
_DET, _DSC = "detector_head_convolutions.", "descriptor_head_convolutions."


def _need_device(t, who):
    if not t.is_cuda:
        raise _lib.XPointHipError(f"{who}: tensors must live on the GPU (xpoint_amd has no CPU fallback)")


def _check_operands(who, *tensors):
    """Every tensor operand of an operator-level call: float32, on the GPU, all on the first one's device (None = an absent optional operand)."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        _need_device(t, who)
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: operands must be float32, got {t.dtype}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise _lib.XPointHipError(f"{who}: operands live on different devices ({dev} and {t.device})")


def _vp(t, offset=0):
    """Pointer of element `offset` of a float32 device tensor whose rows are contiguous (column slices carry their ld separately)."""
    assert t.is_cuda and t.dtype == torch.float32
    return ctypes.c_void_p(t.data_ptr() + 4 * offset)


def _bytes(n, dev):
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device=dev)


def _bn_ws(C, dev):
    return _bytes(_lib.load().xp_bn_workspace_bytes(C), dev)


# ------------------------------------------------------------------------------------------------------------------------------------
# operator level (what tests/test_gpu_head_training.py pins one by one)
# ------------------------------------------------------------------------------------------------------------------------------------
def gemm_tn(P, Q, out=None, p_scale=None, stream=None):
    """out[i][j] = sum_m P[m][i] Q[m][j].  P (M, I) the gradient operand, Q (M, J); both may be column slices of wider matrices (row stride
    = ld).  out: an (I, J) view with contiguous rows or None (allocated).  p_scale: None, or the device float[2] {S, 1 / S} of an operand that
    already holds S x the gradient."""
    _check_operands("gemm_tn", P, Q, out, p_scale)
    M, I = P.shape
    J = Q.shape[1]
    assert Q.shape[0] == M and P.stride(1) == 1 and Q.stride(1) == 1
    if out is None:
        out = torch.empty((I, J), dtype=torch.float32, device=P.device)
    assert out.shape == (I, J) and out.stride(1) == 1
    n = _lib.load().xp_gemm_tn_h2_workspace_bytes(M, I, J)
    ws = _bytes(n, P.device)
    _lib.call("xp_gemm_tn_h2", _vp(P), _vp(Q), _vp(out), M, I, J, int(P.stride(0)) if M > 1 else max(I, int(P.stride(0))),
              int(Q.stride(0)) if M > 1 else max(J, int(Q.stride(0))), int(out.stride(0)) if I > 1 else max(J, int(out.stride(0))),
              None if p_scale is None else _vp(p_scale), ptr(ws), ctypes.c_size_t(ws.numel()), _lib.current_stream(P) if stream is None else stream)
    return out


def conv3x3_wgrad(x_nhwc, dy_nhwc, dy_scale=None, stride=1, reflect_pad=1, stream=None):
    """Weight gradient (Co, 3, 3, Ci) of the reflection-padded stride-1 3x3 convolution: x (B, H, W, Ci), dy (B, H, W, Co), contiguous."""
    _check_operands("conv3x3_wgrad", x_nhwc, dy_nhwc, dy_scale)
    if tuple(dy_nhwc.shape[:3]) != tuple(x_nhwc.shape[:3]):
        raise ValueError(f"conv3x3_wgrad: x {tuple(x_nhwc.shape)} and dy {tuple(dy_nhwc.shape)} do not share (B, H, W)")
    B, H, W, Ci = x_nhwc.shape
    Co = dy_nhwc.shape[-1]
    dw = torch.empty((Co, 3, 3, Ci), dtype=torch.float32, device=x_nhwc.device)
    ws = _bytes(_lib.load().xp_gemm_tn_h2_workspace_bytes(B * H * W, Co, 9 * Ci), x_nhwc.device)
    _lib.call("xp_conv3x3_wgrad_h2", ptr(x_nhwc), ptr(dy_nhwc), ptr(dw), B, H, W, Ci, Co, int(stride), int(reflect_pad),
              None if dy_scale is None else _vp(dy_scale), ptr(ws), ctypes.c_size_t(ws.numel()), _lib.current_stream(x_nhwc) if stream is None else stream)
    return dw


def bn_train_fwd(x, gamma, beta, eps=BN_EPS, y=None, stream=None):
    """x (rows, C) rows with any ld -> (y, save_mean (2, C), save_invstd, biased batch variance)."""
    _check_operands("bn_train_fwd", x, gamma, beta, y)
    rows, C = x.shape
    if gamma.shape != (C,) or beta.shape != (C,) or x.stride(1) != 1:
        raise ValueError(f"bn_train_fwd: gamma / beta must be ({C},) and the rows of x contiguous")
    dev = x.device
    if y is None:
        y = torch.empty((rows, C), dtype=torch.float32, device=dev)
    mean = torch.empty((2, C), dtype=torch.float32, device=dev)          # the f32 mean and the f32 remainder of the f64 mean
    invstd, var = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
    ws = _bn_ws(C, dev)
    _lib.call("xp_bn_train_fwd", _vp(x), int(x.stride(0)), ptr(gamma), ptr(beta), _vp(y), int(y.stride(0)), ptr(mean), ptr(invstd), ptr(var),
              rows, C, float(eps), ptr(ws), ctypes.c_size_t(ws.numel()), _lib.current_stream(x) if stream is None else stream)
    return y, mean, invstd, var


def bn_train_bwd(dy, x, gamma, mean, invstd, relu_mask=False, scaled=False, dx=None, stream=None):
    """-> (dx, dgamma, dbeta, scale).  scaled: dx holds S x the gradient and scale = the device float[2] {S, 1 / S}; else scale is None."""
    _check_operands("bn_train_bwd", x, dy, gamma, mean, invstd, dx)
    rows, C = x.shape
    if dy.shape != x.shape or gamma.shape != (C,) or mean.shape != (2, C) or invstd.shape != (C,) or x.stride(1) != 1 or dy.stride(1) != 1:
        raise ValueError("bn_train_bwd: dy as x, gamma / invstd (C,), mean (2, C), contiguous rows")
    dev = x.device
    if dx is None:
        dx = torch.empty((rows, C), dtype=torch.float32, device=dev)
    dgamma, dbeta = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
    scale = torch.empty(2, dtype=torch.float32, device=dev) if scaled else None
    ws = _bn_ws(C, dev)
    _lib.call("xp_bn_train_bwd", _vp(dy), int(dy.stride(0)), _vp(x), int(x.stride(0)), ptr(gamma), ptr(mean), ptr(invstd), _vp(dx), int(dx.stride(0)),
              ptr(dgamma), ptr(dbeta), ptr(scale), int(bool(relu_mask)), rows, C, ptr(ws), ctypes.c_size_t(ws.numel()), _lib.current_stream(x) if stream is None else stream)
    return dx, dgamma, dbeta, scale


def colsum_rows(x, x_scale=None, stream=None):
    """out[c] = sum_r x[r][c] in the fixed order of the BatchNorm sums; x_scale {S, 1 / S}: x holds S x the values."""
    _check_operands("colsum_rows", x, x_scale)
    rows, C = x.shape
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = _bn_ws(C, x.device)
    _lib.call("xp_colsum_rows", _vp(x), int(x.stride(0)), rows, C, None if x_scale is None else _vp(x_scale), ptr(out), ptr(ws),
              ctypes.c_size_t(ws.numel()), _lib.current_stream(x) if stream is None else stream)
    return out


def l2norm_rows_bwd(x, dy, eps=L2_EPS, stream=None):
    """Backward of y = x / max(|x|, eps) over the rows of x (rows, C)."""
    _check_operands("l2norm_rows_bwd", x, dy)
    rows, C = x.shape
    if dy.shape != x.shape:
        raise ValueError("l2norm_rows_bwd: dy must have the shape of x")
    dy = dy.contiguous()
    dx = torch.empty((rows, C), dtype=torch.float32, device=x.device)
    _lib.call("xp_l2norm_rows_bwd", _vp(x), int(x.stride(0)), ptr(dy), ptr(dx), rows, C, float(eps), _lib.current_stream(x) if stream is None else stream)
    return dx


def conv3x3_wgrad_zero_pad(x_nhwc, dy_nhwc, dy_scale=None, stream=None):
    """Weight gradient (Co, 3, 3, Ci) of the stride-1 3x3 convolution with ZERO padding 1 (the RegNet head's): x (B, H, W, Ci), dy (B, H, W, Co)."""
    _check_operands("conv3x3_wgrad_zero_pad", x_nhwc, dy_nhwc, dy_scale)
    if x_nhwc.dim() != 4 or dy_nhwc.dim() != 4 or tuple(dy_nhwc.shape[:3]) != tuple(x_nhwc.shape[:3]):
        raise ValueError(f"conv3x3_wgrad_zero_pad: x {tuple(x_nhwc.shape)} and dy {tuple(dy_nhwc.shape)} do not share (B, H, W)")
    B, H, W, Ci = x_nhwc.shape
    Co = dy_nhwc.shape[-1]
    dw = torch.empty((Co, 3, 3, Ci), dtype=torch.float32, device=x_nhwc.device)
    ws = _bytes(_lib.load().xp_gemm_tn_h2_workspace_bytes(B * H * W, Co, 9 * Ci), x_nhwc.device)
    _lib.call("xp_conv3x3_zp_wgrad_h2", ptr(x_nhwc), ptr(dy_nhwc), ptr(dw), B, H, W, Ci, Co, None if dy_scale is None else _vp(dy_scale), ptr(ws),
              ctypes.c_size_t(ws.numel()), _lib.current_stream(x_nhwc) if stream is None else stream)
    return dw


def conv3x3_dgrad(dy_nhwc, w_ohwi, dy_scale=None, stream=None):
    """Input gradient (B, H, W, Ci) of the stride-1 zero-padded 3x3 convolution from dy (B, H, W, Co) and w (Co, 3, 3, Ci).  dy_scale: None, or
    the device float[2] {S, 1 / S} of a dy that already holds S x the gradient; the result is the unscaled gradient either way.  Co % 4 == 0."""
    _check_operands("conv3x3_dgrad", dy_nhwc, w_ohwi, dy_scale)
    if dy_nhwc.dim() != 4 or w_ohwi.dim() != 4 or tuple(w_ohwi.shape[:3]) != (dy_nhwc.shape[-1], 3, 3):
        raise ValueError(f"conv3x3_dgrad: dy {tuple(dy_nhwc.shape)} must be (B, H, W, Co) and w {tuple(w_ohwi.shape)} (Co, 3, 3, Ci)")
    B, H, W, Co = dy_nhwc.shape
    Ci = w_ohwi.shape[-1]
    dx = torch.empty((B, H, W, Ci), dtype=torch.float32, device=dy_nhwc.device)
    ws = _bytes(_lib.load().xp_conv3x3_dgrad_h2_workspace_bytes(B, H, W, Ci, Co), dy_nhwc.device)
    _lib.call("xp_conv3x3_dgrad_h2", ptr(dy_nhwc), ptr(w_ohwi), ptr(dx), B, H, W, Ci, Co, None if dy_scale is None else _vp(dy_scale), ptr(ws),
              ctypes.c_size_t(ws.numel()), _lib.current_stream(dy_nhwc) if stream is None else stream)
    return dx


def _relu(x, stream=None):
    y = torch.empty_like(x)
    _lib.call("xp_relu_fwd", ptr(x), ptr(y), x.numel(), _lib.current_stream(x) if stream is None else stream)
    return y


def relu_bwd(dr, y, stream=None):
    """dy = dr where y > 0, else 0 (y: the ReLU's input, or its output)."""
    _check_operands("relu_bwd", dr, y)
    if dr.shape != y.shape:
        raise ValueError("relu_bwd: dr must have the shape of y")
    dr, y = dr.contiguous(), y.contiguous()
    dy = torch.empty_like(y)
    _lib.call("xp_relu_bwd", ptr(dr), ptr(y), ptr(dy), y.numel(), _lib.current_stream(y) if stream is None else stream)
    return dy


def maxpool2_relu_bwd(dpool, y_nhwc, stream=None):
    """Backward of max_pool2d(relu(y), 2): y (B, H, W, C), dpool (B, H // 2, W // 2, C) -> dy (B, H, W, C), torch's choice element for element."""
    _check_operands("maxpool2_relu_bwd", dpool, y_nhwc)
    B, H, W, C = y_nhwc.shape
    if tuple(dpool.shape) != (B, H // 2, W // 2, C):
        raise ValueError(f"maxpool2_relu_bwd: dpool {tuple(dpool.shape)} must be {(B, H // 2, W // 2, C)}")
    dy = torch.empty_like(y_nhwc, memory_format=torch.contiguous_format)
    _lib.call("xp_maxpool2_relu_bwd", ptr(dpool.contiguous()) if dpool.numel() else None, ptr(y_nhwc), ptr(dy), B, H, W, C,
              _lib.current_stream(y_nhwc) if stream is None else stream)
    return dy


def costvolume_mean_bwd(a, b, dv, stream=None):
    """Backward of v[n][p] = a[n][p] . mean_q b[n][q]: a, b (B, hw, C), dv (B, hw) -> (da, db)."""
    _check_operands("costvolume_mean_bwd", a, b, dv)
    B, hw, C = a.shape
    if b.shape != a.shape or tuple(dv.shape) != (B, hw):
        raise ValueError("costvolume_mean_bwd: b as a (B, hw, C), dv (B, hw)")
    da, db = torch.empty_like(a, memory_format=torch.contiguous_format), torch.empty_like(a, memory_format=torch.contiguous_format)
    _lib.call("xp_costvolume_mean_bwd", ptr(a), ptr(b), ptr(dv.contiguous()), ptr(da), ptr(db), B, hw, C, _lib.current_stream(a) if stream is None else stream)
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
        mask, use = mask.contiguous(), 1
        ids = None
    else:
        mask, use = torch.empty((rows, C), dtype=torch.uint8, device=x.device), 0
        ids = torch.arange(rows, dtype=torch.int32, device=x.device) if sample_ids is None else sample_ids.to(torch.int32).contiguous()
        if tuple(ids.shape) != (rows,):
            raise ValueError(f"dropout_rows: sample_ids must be ({rows},)")
    _lib.call("xp_dropout_rows", ptr(x), ptr(y), ctypes.c_void_p(mask.data_ptr()), use, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
              None if ids is None else ctypes.c_void_p(ids.data_ptr()), int(tag), float(p), rows, C, _lib.current_stream(x) if stream is None else stream)
    return y, mask


def _split_h2(w_nk, stream=None):
    N, K = w_nk.shape
    out = torch.empty(_lib.load().xp_split_weights_h2_bytes(N, K), dtype=torch.uint8, device=w_nk.device)
    _lib.call("xp_split_weights_h2", ptr(w_nk.contiguous()), ctypes.c_void_p(out.data_ptr()), N, K, _lib.current_stream(w_nk) if stream is None else stream)
    return out


def _gemm_nt_h2(a, wsplit, N, K, out, bias=None, scale=None, shift=None, act=0, stream=None, res=None):
    """out (M, N; ld) = epilogue(a (M, K; ld) @ W^T) [+ res (M, N; ld)] on the forward's split-fp16 engine."""
    _lib.call("xp_gemm_nt_h2", _vp(a), ctypes.c_void_p(wsplit.data_ptr()), _vp(out), ptr(bias), ptr(scale), ptr(shift), None if res is None else _vp(res),
              a.shape[0], N, K, int(a.stride(0)), int(out.stride(0)), 0 if res is None else int(res.stride(0)), act,
              _lib.current_stream(a) if stream is None else stream)
    return out


def _conv3x3_h2(x, w_ohwi, bias, scale=None, shift=None, stream=None):
    """relu(conv3x3(reflection_pad(x)) + bias) [* scale + shift]: the head trunk's launch of the inference path."""
    B, H, W, Ci = x.shape
    Co = w_ohwi.shape[0]
    y = torch.empty((B, H, W, Co), dtype=torch.float32, device=x.device)
    wsplit = _split_h2(w_ohwi.reshape(Co, 9 * Ci), stream=stream)
    _lib.call("xp_conv3x3_nhwc_h2", ptr(x), ctypes.c_void_p(wsplit.data_ptr()), ptr(y), ptr(bias), ptr(scale), ptr(shift), B, H, W, Ci, Co, 1, 1, 2,
              _lib.current_stream(x) if stream is None else stream)
    return y


def _pad4(n):
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------------------------------------------
# autograd
# ------------------------------------------------------------------------------------------------------------------------------------
class _TrunkFn(torch.autograd.Function):
    """enc (B, Hc, Wc, Ci), w (Co, 3, 3, Ci), b, gamma, beta (Co) -> h = BN(relu(conv(enc))) (B, Hc, Wc, Co), batch mean, biased batch var."""

    @staticmethod
    def forward(ctx, enc, w, b, gamma, beta):
        B, H, W, _ = enc.shape
        Co = w.shape[0]
        st = _lib.current_stream(enc)            # looked up once per call: every launch below goes to it
        a = _conv3x3_h2(enc, w.contiguous(), b.contiguous(), stream=st)
        h, mean, invstd, var = bn_train_fwd(a.view(B * H * W, Co), gamma.contiguous(), beta.contiguous(), stream=st)
        ctx.save_for_backward(enc, a, gamma, mean, invstd)
        ctx.mark_non_differentiable(mean, var)
        return h.view(B, H, W, Co), mean, var

    @staticmethod
    def backward(ctx, dh, _dm, _dv):
        enc, a, gamma, mean, invstd = ctx.saved_tensors
        B, H, W, Co = a.shape
        dh = dh.contiguous().view(B * H * W, Co)
        # the trunk's order is conv -> ReLU -> BatchNorm: the masked, scaled dx is the gradient of the convolution's output
        st = _lib.current_stream(enc)
        da, dgamma, dbeta, scale = bn_train_bwd(dh, a.view(B * H * W, Co), gamma.contiguous(), mean, invstd, relu_mask=True, scaled=True, stream=st)
        db = colsum_rows(da, scale, stream=st)
        dw = conv3x3_wgrad(enc, da.view(B, H, W, Co), scale, stream=st)
        return None, dw, db, dgamma, dbeta


class _TailFn(torch.autograd.Function):
    """h (rows, 2 Ch) -> BN(h[:, :Ch] W_det^T + b_det) (rows, 65), BN(h[:, Ch:] W_desc^T + b_desc) (rows, D), and the four batch statistics."""

    @staticmethod
    def forward(ctx, h, w_det, b_det, g_det, be_det, w_dsc, b_dsc, g_dsc, be_dsc):
        rows, Ch2 = h.shape
        Ch = Ch2 // 2
        outs, saved, stats = [], [], []
        st = _lib.current_stream(h)
        for k, (w, b, g, be) in enumerate(((w_det, b_det, g_det, be_det), (w_dsc, b_dsc, g_dsc, be_dsc))):
            C = w.shape[0]
            z = torch.empty((rows, _pad4(C)), dtype=torch.float32, device=h.device)[:, :C]      # ld a multiple of 4: the backward's A operand
            _gemm_nt_h2(h[:, k * Ch:(k + 1) * Ch], _split_h2(w, stream=st), C, Ch, z, bias=b.contiguous(), stream=st)
            o, mean, invstd, var = bn_train_fwd(z, g.contiguous(), be.contiguous(), stream=st)
            outs.append(o); saved += [z, mean, invstd]; stats += [mean, var]
        ctx.save_for_backward(h, w_det, g_det, w_dsc, g_dsc, *saved)
        ctx.mark_non_differentiable(*stats)
        return (outs[0], outs[1]) + tuple(stats)

    @staticmethod
    def backward(ctx, do_det, do_dsc, *_stats):
        h, w_det, g_det, w_dsc, g_dsc, z0, m0, i0, z1, m1, i1 = ctx.saved_tensors
        rows, Ch2 = h.shape
        Ch = Ch2 // 2
        dh = torch.empty_like(h)
        grads = []
        st = _lib.current_stream(h)
        zero_shift = torch.zeros(Ch, dtype=torch.float32, device=h.device)
        for k, (do, w, g, z, mean, invstd) in enumerate(((do_det, w_det, g_det, z0, m0, i0), (do_dsc, w_dsc, g_dsc, z1, m1, i1))):
            C = w.shape[0]
            Cp = _pad4(C)
            do = torch.zeros((rows, C), dtype=torch.float32, device=h.device) if do is None else do.contiguous()
            dzp = torch.empty((rows, Cp), dtype=torch.float32, device=h.device)
            if Cp != C:
                dzp[:, C:] = 0.0                                                                # the pad columns of the A operand
            dz, dg, dbe, scale = bn_train_bwd(do, z, g.contiguous(), mean, invstd, scaled=True, dx=dzp[:, :C], stream=st)
            db = colsum_rows(dz, scale, stream=st)
            hk = h[:, k * Ch:(k + 1) * Ch]
            dw = gemm_tn(dz, hk, p_scale=scale, stream=st)
            # input gradient: (S dz) W / S — the forward engine on the transposed weight, 1 / S in the epilogue's scale vector
            wt = torch.zeros((Ch, Cp), dtype=torch.float32, device=h.device)
            wt[:, :C] = w.t()
            _gemm_nt_h2(dzp, _split_h2(wt, stream=st), Ch, Cp, dh[:, k * Ch:(k + 1) * Ch], scale=scale[1:2].expand(Ch).contiguous(), shift=zero_shift,
                        stream=st)
            grads += [dw, db, dg, dbe]
        return (dh,) + tuple(grads)


class _L2NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = torch.empty_like(x)
        _lib.call("xp_l2norm_rows", ptr(x), ptr(y), x.shape[0], x.shape[1], float(L2_EPS), _lib.current_stream(x))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return l2norm_rows_bwd(x, dy)


# ------------------------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------------------------
class XPointHeads(torch.nn.Module):
    """The detector and descriptor heads of XPoint with the reference's state_dict names (XPoint.py:112-138)."""

    def __init__(self, in_channels=48, head_channels=256, descriptor_size=256, detector_channels=65):
        super().__init__()
        self.in_channels, self.head_channels = int(in_channels), int(head_channels)
        self.descriptor_size, self.detector_channels = int(descriptor_size), int(detector_channels)
        if self.in_channels % 4 or self.head_channels % 4:
            raise ValueError("XPointHeads: in_channels and head_channels must be multiples of 4")
        nn = torch.nn

        def head(co):       # parameter containers with the reference's layout and initialisation; forward() never calls them
            return nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(self.in_channels, self.head_channels, 3), nn.ReLU(inplace=True),
                                 nn.BatchNorm2d(self.head_channels), nn.Conv2d(self.head_channels, co, 1), nn.BatchNorm2d(co))
        self.detector_head_convolutions = head(self.detector_channels)
        self.descriptor_head_convolutions = head(self.descriptor_size)

    def t(self, key):
        """The parameter or buffer with the reference's name `key`."""
        mod, _, leaf = key.rpartition(".")
        return getattr(self.get_submodule(mod), leaf)

    @classmethod
    def from_model(cls, net):
        """The heads of a loaded models.XPoint (VMamba: Ci = EMBED_DIM / 2 = 48; conv encoder: Ci = 128), as a copy."""
        sd = net.state_dict()
        w1 = sd[_DET + "1.weight"]
        heads = cls(in_channels=w1.shape[1], head_channels=w1.shape[0], descriptor_size=sd[_DSC + "4.weight"].shape[0],
                    detector_channels=sd[_DET + "4.weight"].shape[0])
        own = heads.state_dict()
        missing = [k for k in own if k not in sd and not k.endswith("num_batches_tracked")]
        if missing:
            raise RuntimeError(f"XPointHeads.from_model: the model holds no {missing[:3]}")
        heads.load_state_dict({k: sd[k] for k in own if k in sd}, strict=False)
        return heads

    def _update_running(self, stats, rows):
        """nn.BatchNorm2d's update of the four BatchNorms' buffers from stats = [(prefix, batch mean, biased batch variance)], four launches in all."""
        with torch.no_grad():
            rm = [self.t(p + "running_mean") for p, _, _ in stats]
            rv = [self.t(p + "running_var") for p, _, _ in stats]
            torch._foreach_mul_(rm + rv, 1.0 - BN_MOMENTUM)
            torch._foreach_add_(rm, [m for _, m, _ in stats], alpha=BN_MOMENTUM)
            torch._foreach_add_(rv, [v for _, _, v in stats], alpha=BN_MOMENTUM * rows / (rows - 1.0))       # the running value is the unbiased variance
            torch._foreach_add_([self.t(p + "num_batches_tracked") for p, _, _ in stats], 1)

    def _affine(self, pre):
        scale = self.t(pre + "weight").double() / torch.sqrt(self.t(pre + "running_var").double() + BN_EPS)
        shift = self.t(pre + "bias").double() - self.t(pre + "running_mean").double() * scale
        return scale.float().contiguous(), shift.float().contiguous()

    def forward(self, enc_nhwc):
        """enc_nhwc (B, Hc, Wc, Ci) on the GPU -> {'logits': (B, 65, Hc, Wc), 'desc': (B, D, Hc, Wc)} (channel-last memory, NCHW shape)."""
        _need_device(enc_nhwc, "XPointHeads")
        if enc_nhwc.requires_grad:
            raise NotImplementedError("XPointHeads: the encoder is frozen in this build (no convolution input gradient); pass a detached enc_nhwc")
        if enc_nhwc.dim() != 4 or enc_nhwc.shape[-1] != self.in_channels:
            raise ValueError(f"XPointHeads: enc_nhwc must be (B, Hc, Wc, {self.in_channels}), got {tuple(enc_nhwc.shape)}")
        if self.t(_DET + "1.weight").device != enc_nhwc.device:
            raise _lib.XPointHipError("XPointHeads: parameters and enc_nhwc live on different devices")
        enc = enc_nhwc.detach().to(torch.float32).contiguous()
        B, Hc, Wc, _ = enc.shape
        rows, Ch = B * Hc * Wc, self.head_channels
        cat = lambda suffix: torch.cat([self.t(_DET + suffix), self.t(_DSC + suffix)], 0)
        w1 = cat("1.weight").permute(0, 2, 3, 1)                 # (2 Ch, 3, 3, Ci): both trunks as one launch
        w4 = [self.t(p + "4.weight").reshape(-1, Ch) for p in (_DET, _DSC)]
        with torch.cuda.device(enc.device):
            if self.training:
                if rows < 2:
                    raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size((B, Ch, Hc, Wc))}")
                h, m3, v3 = _TrunkFn.apply(enc, w1, cat("1.bias"), cat("3.weight"), cat("3.bias"))
                o_det, o_dsc, m_det, v_det, m_dsc, v_dsc = _TailFn.apply(
                    h.view(rows, 2 * Ch), w4[0], self.t(_DET + "4.bias"), self.t(_DET + "5.weight"), self.t(_DET + "5.bias"),
                    w4[1], self.t(_DSC + "4.bias"), self.t(_DSC + "5.weight"), self.t(_DSC + "5.bias"))
                self._update_running([(_DET + "3.", m3[0, :Ch], v3[:Ch]), (_DSC + "3.", m3[0, Ch:], v3[Ch:]),
                                      (_DET + "5.", m_det[0], v_det), (_DSC + "5.", m_dsc[0], v_dsc)], rows)
                desc = _L2NormFn.apply(o_dsc)
            else:
                with torch.no_grad():
                    a, b = self._affine(_DET + "3."), self._affine(_DSC + "3.")
                    h = _conv3x3_h2(enc, w1.contiguous(), cat("1.bias"), torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]])).view(rows, 2 * Ch)
                    outs = []
                    for k, p in enumerate((_DET, _DSC)):
                        sc, sh = self._affine(p + "5.")
                        o = torch.empty((rows, w4[k].shape[0]), dtype=torch.float32, device=enc.device)
                        _gemm_nt_h2(h[:, k * Ch:(k + 1) * Ch], _split_h2(w4[k]), w4[k].shape[0], Ch, o, bias=self.t(p + "4.bias").contiguous(), scale=sc, shift=sh)
                        outs.append(o)
                    o_det = outs[0]
                    desc = torch.empty_like(outs[1])
                    _lib.call("xp_l2norm_rows", ptr(outs[1]), ptr(desc), rows, desc.shape[1], float(L2_EPS), _lib.current_stream(enc))
        return {'logits': o_det.view(B, Hc, Wc, -1).permute(0, 3, 1, 2), 'desc': desc.view(B, Hc, Wc, -1).permute(0, 3, 1, 2)}


# ------------------------------------------------------------------------------------------------------------------------------------
# the homography head (reference xpoint/models/RegNet.py)
# ------------------------------------------------------------------------------------------------------------------------------------
_HM = "hm_regressor."


def _conv3x3_zp_h2(x, wsplit, Co, stream=None):
    """conv3x3(zero_pad(x)), no bias, no activation, on the split-fp16 engine: x (B, H, W, Ci), wsplit = _split_h2 of w (Co, 9 Ci)."""
    B, H, W, Ci = x.shape
    y = torch.empty((B, H, W, Co), dtype=torch.float32, device=x.device)
    _lib.call("xp_conv3x3_nhwc_h2", ptr(x), ctypes.c_void_p(wsplit.data_ptr()), ptr(y), None, None, None, B, H, W, Ci, Co, 1, 0, 0,
              _lib.current_stream(x) if stream is None else stream)
    return y


class _Layer1Fn(torch.autograd.Function):
    """RegNet.layer1 on one image's maps: enc (B, H, W, Ci), w1 (C1, 3, 3, Ci), gamma1, beta1, w2 (C2, 3, 3, C1), gamma2, beta2 ->
    maxpool2(relu(y2)) (B, H / 2, W / 2, C2), the two BatchNorm outputs y1, y2 and the batch statistics (mean (2, C), biased variance) of both.
    s1, s2: the split-fp16 planes of w1, w2 (made once per forward of the module: both images use them)."""

    @staticmethod
    def forward(ctx, enc, w1, g1, b1, w2, g2, b2, s1, s2):
        B, H, W, _ = enc.shape
        C1, C2 = w1.shape[0], w2.shape[0]
        rows = B * H * W
        st = _lib.current_stream(enc)
        z1 = _conv3x3_zp_h2(enc, s1, C1, stream=st)
        y1, m1, i1, v1 = bn_train_fwd(z1.view(rows, C1), g1.contiguous(), b1.contiguous(), stream=st)
        r1 = _relu(y1, stream=st).view(B, H, W, C1)
        z2 = _conv3x3_zp_h2(r1, s2, C2, stream=st)
        y2, m2, i2, v2 = bn_train_fwd(z2.view(rows, C2), g2.contiguous(), b2.contiguous(), stream=st)
        y2 = y2.view(B, H, W, C2)
        pooled = torch.empty((B, H // 2, W // 2, C2), dtype=torch.float32, device=enc.device)
        _lib.call("xp_maxpool2_nhwc", ptr(y2), ptr(pooled), B, H, W, C2, st)
        a = _relu(pooled, stream=st)                       # relu(maxpool(y)) == maxpool(relu(y)), value for value: the ReLU is monotone
        y1 = y1.view(B, H, W, C1)
        ctx.save_for_backward(enc, z1, y1, r1, z2, y2, w2, g1, g2, m1, i1, m2, i2)
        ctx.mark_non_differentiable(y1, y2, m1, v1, m2, v2)
        return a, y1, y2, m1, v1, m2, v2

    @staticmethod
    def backward(ctx, da, *_rest):
        enc, z1, y1, r1, z2, y2, w2, g1, g2, m1, i1, m2, i2 = ctx.saved_tensors
        B, H, W, C1 = y1.shape
        C2 = y2.shape[-1]
        rows = B * H * W
        st = _lib.current_stream(enc)
        dy2 = maxpool2_relu_bwd(da.contiguous(), y2, stream=st)
        dz2, dg2, db2, sc2 = bn_train_bwd(dy2.view(rows, C2), z2.view(rows, C2), g2.contiguous(), m2, i2, scaled=True, stream=st)
        dz2 = dz2.view(B, H, W, C2)
        dw2 = conv3x3_wgrad_zero_pad(r1, dz2, sc2, stream=st)
        dr1 = conv3x3_dgrad(dz2, w2, sc2, stream=st)        # unscaled: 1 / S is applied in the engine's epilogue
        dy1 = relu_bwd(dr1, y1, stream=st)
        dz1, dg1, db1, sc1 = bn_train_bwd(dy1.view(rows, C1), z1.view(rows, C1), g1.contiguous(), m1, i1, scaled=True, stream=st)
        dw1 = conv3x3_wgrad_zero_pad(enc, dz1.view(B, H, W, C1), sc1, stream=st)
        return None, dw1, dg1, db1, dw2, dg2, db2, None, None


class _CostVolumeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        B, hw, C = a.shape
        v = torch.empty((B, hw), dtype=torch.float32, device=a.device)
        _lib.call("xp_costvolume_mean", ptr(a), ptr(b), ptr(v), B, hw, C, _lib.current_stream(a))
        ctx.save_for_backward(a, b)
        return v

    @staticmethod
    def backward(ctx, dv):
        a, b = ctx.saved_tensors
        return costvolume_mean_bwd(a, b, dv)


def _transposed(x):
    """x^T with contiguous rows of stride 1 (what `.t().contiguous()` does not promise when a dimension is 1)."""
    out = torch.empty((x.shape[1], x.shape[0]), dtype=x.dtype, device=x.device)
    out.copy_(x.t())
    return out


class _FcFn(torch.autograd.Function):
    """RegNet.fc in training mode: v (B, K) -> Linear(relu(Linear(dropout(v))) dropped again).  masks: (m1 (B, K), m2 (B, N1)) uint8 or None (drawn from
    seed and sample_ids with tags 0 and 1)."""

    @staticmethod
    def forward(ctx, v, w1, b1, w2, b2, p, seed, sample_ids, masks):
        B, K = v.shape
        N1, N2 = w1.shape[0], w2.shape[0]
        st = _lib.current_stream(v)
        dev = v.device
        d1, m1 = dropout_rows(v, p, seed, sample_ids, 0, None if masks is None else masks[0], stream=st)
        h = torch.empty((B, N1), dtype=torch.float32, device=dev)
        _gemm_nt_h2(d1, _split_h2(w1, stream=st), N1, K, h, bias=b1.contiguous(), act=2, stream=st)
        d2, m2 = dropout_rows(h, p, seed, sample_ids, 1, None if masks is None else masks[1], stream=st)
        hm = torch.empty((B, N2), dtype=torch.float32, device=dev)
        _gemm_nt_h2(d2, _split_h2(w2, stream=st), N2, N1, hm, bias=b2.contiguous(), stream=st)
        ctx.save_for_backward(d1, h, d2, m1, m2, w1, w2)
        ctx.p = p
        return hm

    @staticmethod
    def backward(ctx, dhm):
        d1, h, d2, m1, m2, w1, w2 = ctx.saved_tensors
        st = _lib.current_stream(h)
        dhm = dhm.contiguous()
        dw2 = gemm_tn(dhm, d2, stream=st)
        db2 = colsum_rows(dhm, stream=st)
        # a linear layer's input gradient dX = dY W as the weight-gradient GEMM read the other way (reduction over the output features): its
        # gradient operand takes one power of two per call, so any finite gradient range is accepted without a scaled copy
        dd2 = gemm_tn(_transposed(dhm), w2.contiguous(), stream=st)
        dh, _ = dropout_rows(dd2, ctx.p, mask=m2, stream=st)
        dpre = relu_bwd(dh, h, stream=st)
        dw1 = gemm_tn(dpre, d1, stream=st)
        db1 = colsum_rows(dpre, stream=st)
        dd1 = gemm_tn(_transposed(dpre), w1.contiguous(), stream=st)
        dv, _ = dropout_rows(dd1, ctx.p, mask=m1, stream=st)
        return dv, dw1, db1, dw2, db2, None, None, None, None


class RegNetHead(torch.nn.Module):
    """The homography regression head of XPoint (reference xpoint/models/RegNet.py) with the reference's state_dict names under `hm_regressor.`:

        regnet = training.RegNetHead.from_model(net).cuda().train()
        pred_hm = regnet(enc[:n], enc[n:], seed=step)              # (n, 8); enc: the frozen encoder's NHWC maps of both spectra

    layer1 = [Conv3x3(zero pad, no bias), BatchNorm, ReLU] x 2 + MaxPool2 runs once per image — first image, then second — each call on its own
    batch statistics, so the running statistics are updated twice per forward and num_batches_tracked advances by 2, as the reference's two
    `self.layer1(...)` calls do.  Then F.normalize over channels, the cost volume with its global average pool, and fc = [Dropout(0.5),
    Linear(256, 64), ReLU, Dropout(0.5), Linear(64, 8)].  Dropout masks are drawn per sample from (seed, sample id), never from the batch
    neighbours, or given (`dropout_masks`).  In `.eval()` the forward is convmodels.regnet_forward on this module's weights.
    Both convolutions run on the split-fp16 engine: activations must stay below 65504 in magnitude — the encoder output, and the first BatchNorm's
    output, which batch statistics bound by |gamma| sqrt(rows) + |beta| (O(1) in this network); gradients of any finite range are accepted.
    No gradient reaches the encoder: an input that requires grad raises NotImplementedError."""

    DROPOUT_P = 0.5

    def __init__(self):
        super().__init__()
        nn = torch.nn
        hm = nn.Module()          # parameter containers with the reference's layout and initialisation; forward() never calls them
        hm.layer1 = nn.Sequential(nn.Conv2d(48, 96, 3, padding=1, bias=False), nn.BatchNorm2d(96), nn.ReLU(inplace=True),
                                  nn.Conv2d(96, 192, 3, padding=1, bias=False), nn.BatchNorm2d(192), nn.ReLU(inplace=True), nn.MaxPool2d(2))
        hm.fc = nn.Sequential(nn.Dropout(0.5), nn.Linear(256, 64), nn.ReLU(True), nn.Dropout(0.5), nn.Linear(64, 8))
        self.hm_regressor = hm
        self.last_taps = None

    def t(self, key):
        """The parameter or buffer with the reference's name `key`."""
        mod, _, leaf = key.rpartition(".")
        return getattr(self.get_submodule(mod), leaf)

    @classmethod
    def from_model(cls, net):
        """The homography head of a loaded models.XPoint (configuration with homography_regression_head), as a copy."""
        sd = net.state_dict()
        head = cls()
        own = head.state_dict()
        missing = [k for k in own if k not in sd and not k.endswith("num_batches_tracked")]
        if missing:
            raise RuntimeError(f"RegNetHead.from_model: the model holds no {missing[:3]}")
        head.load_state_dict({k: sd[k] for k in own if k in sd}, strict=False)
        return head

    def _update_running(self, stats, rows):
        """nn.BatchNorm2d's update of both BatchNorms' buffers from stats = [(prefix, batch mean (2, C), biased batch variance)], four launches in all."""
        with torch.no_grad():
            rm = [self.t(p + "running_mean") for p, _, _ in stats]
            rv = [self.t(p + "running_var") for p, _, _ in stats]
            torch._foreach_mul_(rm + rv, 1.0 - BN_MOMENTUM)
            torch._foreach_add_(rm, [m[0] for _, m, _ in stats], alpha=BN_MOMENTUM)
            torch._foreach_add_(rv, [v for _, _, v in stats], alpha=BN_MOMENTUM * rows / (rows - 1.0))       # the running value is the unbiased variance
            torch._foreach_add_([self.t(p + "num_batches_tracked") for p, _, _ in stats], 1)

    def forward(self, enc1_nhwc, enc2_nhwc, seed=0, sample_ids=None, dropout_masks=None, keep_taps=False):
        """enc1_nhwc, enc2_nhwc (B, H', W', 48) on the GPU with (H' / 2)(W' / 2) == 256 -> (B, 8).  seed / sample_ids (int32 (B,), default 0 .. B - 1):
        the keys of the training dropout; dropout_masks = (m1 (B, 256), m2 (B, 64)) uint8 replaces the draws; keep_taps: keep the BatchNorm outputs
        before the two ReLUs as self.last_taps = {'y1': [image 1, image 2], 'y2': [...]} (NHWC)."""
        for e in (enc1_nhwc, enc2_nhwc):
            _need_device(e, "RegNetHead")
            if e.requires_grad:
                raise NotImplementedError("RegNetHead: the encoder is frozen in this build (no gradient is passed to it); pass detached encoder maps")
        w1 = self.t(_HM + "layer1.0.weight")
        if enc1_nhwc.dim() != 4 or enc1_nhwc.shape[-1] != w1.shape[1] or enc2_nhwc.shape != enc1_nhwc.shape:
            raise ValueError(f"RegNetHead: both inputs must be (B, H', W', {w1.shape[1]}), got {tuple(enc1_nhwc.shape)} and {tuple(enc2_nhwc.shape)}")
        if w1.device != enc1_nhwc.device or enc2_nhwc.device != enc1_nhwc.device:
            raise _lib.XPointHipError("RegNetHead: parameters and inputs live on different devices")
        enc1, enc2 = (e.detach().to(torch.float32).contiguous() for e in (enc1_nhwc, enc2_nhwc))
        B, H, W, _ = enc1.shape
        fw1, fw2 = self.t(_HM + "fc.1.weight"), self.t(_HM + "fc.4.weight")
        with torch.cuda.device(enc1.device):
            if not self.training:
                from .convmodels import regnet_forward, regnet_weights
                with torch.no_grad():          # the BatchNorm affines from host copies, as models.XPoint folds them after load_state_dict
                    host = {k: v.detach().cpu() for k, v in self.state_dict().items()}
                    return regnet_forward(regnet_weights(host, enc1.device), enc1, enc2)
            rows, hw = B * H * W, (H // 2) * (W // 2)
            if rows < 2:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size((B, w1.shape[0], H, W))}")
            if hw != fw1.shape[1]:
                raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({B}x{hw} and {fw1.shape[1]}x{fw1.shape[0]})")
            if dropout_masks is not None:
                dropout_masks = tuple(m.to(device=enc1.device, dtype=torch.uint8).contiguous() for m in dropout_masks)
            if sample_ids is not None:
                sample_ids = torch.as_tensor(sample_ids, dtype=torch.int32, device=enc1.device)
            w2 = self.t(_HM + "layer1.3.weight")
            w1p, w2p = w1.permute(0, 2, 3, 1).contiguous(), w2.permute(0, 2, 3, 1).contiguous()      # (Co, 3, 3, Ci); autograd permutes the gradients back
            with torch.no_grad():
                s1, s2 = _split_h2(w1p.view(w1.shape[0], -1)), _split_h2(w2p.view(w2.shape[0], -1))
            args = (w1p, self.t(_HM + "layer1.1.weight"), self.t(_HM + "layer1.1.bias"), w2p, self.t(_HM + "layer1.4.weight"), self.t(_HM + "layer1.4.bias"),
                    s1, s2)
            feats, taps = [], {'y1': [], 'y2': []}
            for enc in (enc1, enc2):                      # two calls of layer1, each on its own batch statistics (RegNet.py:33-34)
                a, y1, y2, m1, v1, m2, v2 = _Layer1Fn.apply(enc, *args)
                self._update_running([(_HM + "layer1.1.", m1, v1), (_HM + "layer1.4.", m2, v2)], rows)
                feats.append(_L2NormFn.apply(a.view(B * hw, -1)).view(B, hw, -1))
                taps['y1'].append(y1); taps['y2'].append(y2)
            self.last_taps = taps if keep_taps else None
            v = _CostVolumeFn.apply(feats[0], feats[1])
            return _FcFn.apply(v, fw1, self.t(_HM + "fc.1.bias"), fw2, self.t(_HM + "fc.4.bias"), self.DROPOUT_P, int(seed), sample_ids, dropout_masks)


def finetune_step(net, heads, data, loss_fn, optimizer, regnet=None, seed=0):
    """One head fine-tuning step on a pair batch `data` = {'optical': {'image', 'keypoints', 'valid_mask', 'homography', ...}, 'thermal': {...}}
    (augmentation.augment_pair_batch's dict).  The frozen `net` (eval) produces the encoder output of both spectra in one forward; `heads` runs
    once per spectrum, so each spectrum has its own batch statistics and the running statistics update twice, as the reference's forward_impl
    does per call (XPoint.py:283-323).  regnet: a RegNetHead whose parameters the optimizer also holds: its prediction from the two spectra's encoder
    maps (optical first, XPoint.py:210) goes to the loss as 'pred_hm' (the loss needs homography_regression_loss.check and data['hfour_points']);
    `seed` keys its dropout for this step (pass the step number).  Returns (loss, loss_components)."""
    opt, th = data['optical'], data['thermal']
    n = opt['image'].shape[0]
    if net.training:
        raise RuntimeError("finetune_step: the encoder is frozen; call net.eval()")
    with torch.no_grad():
        flags = None
        if net.config['multispectral']:
            flags = [True] * n + [False] * th['image'].shape[0]
        raw = net.forward_raw(torch.cat([opt['image'], th['image']], 0), want_prob=False, want_desc=False, is_optical=flags)
        enc = raw['enc_nhwc']
    heads.train()
    optimizer.zero_grad(set_to_none=True)
    pred = heads(enc[:n])
    pred2 = heads(enc[n:])
    loss_input = {'data': data, 'pred': pred, 'pred2': pred2}
    if regnet is not None:
        regnet.train()
        loss_input['pred_hm'] = regnet(enc[:n], enc[n:], seed=seed)
    loss, components = loss_fn(loss_input)
    loss.backward()
    optimizer.step()
    return loss.detach(), components


# ------------------------------------------------------------------------------------------------------------------------------------
# a VSS encoder block (reference xpoint/models/vmamba_src/VMamba.py:1153-1234)
# ------------------------------------------------------------------------------------------------------------------------------------
LN_EPS = 1e-5


def _scale_ws(dev):
    return _bytes(_lib.load().xp_scale_grad_workspace_bytes(), dev)


def scale_grad(g, out=None, stream=None):
    """-> (S g, scale): scale the device float[2] {S, 1 / S} with max|g| S in [2^13, 2^14) (S = 1 for an all-zero g): the operand format of a gradient
    that feeds gemm_tn (p_scale) or the forward engine (1 / S in the epilogue).  out: None (allocated), or a tensor of g's shape (g itself is allowed)."""
    _check_operands("scale_grad", g, out)
    g = g.contiguous()
    if out is None:
        out = torch.empty_like(g)
    if out.shape != g.shape or not out.is_contiguous():
        raise ValueError("scale_grad: out must be contiguous and have the shape of g")
    scale = torch.empty(2, dtype=torch.float32, device=g.device)
    ws = _scale_ws(g.device)
    _lib.call("xp_scale_grad", ptr(g), ptr(out), g.numel(), ptr(scale), ptr(ws), ctypes.c_size_t(ws.numel()), _lib.current_stream(g) if stream is None else stream)
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
    dg = torch.empty(C, dtype=torch.float32, device=dev) if want_params else None
    db = torch.empty(C, dtype=torch.float32, device=dev) if want_params else None
    scale = torch.empty(2, dtype=torch.float32, device=dev) if scaled else None
    ws = _bytes(_lib.load().xp_layernorm_bwd_workspace_bytes(rows, C), dev)
    _lib.call("xp_layernorm_bwd", ptr(dy), ptr(x), ptr(gamma), ptr(dx), ptr(dg), ptr(db), rows, C, float(eps), ptr(scale), ptr(ws),
              ctypes.c_size_t(ws.numel()), _lib.current_stream(x) if stream is None else stream)
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
    dw = torch.empty((9, C), dtype=torch.float32, device=dev) if want_dw else None
    scale = torch.empty(2, dtype=torch.float32, device=dev) if scaled else None
    ws = _bytes(_lib.load().xp_dwconv3x3_silu_bwd_workspace_bytes(B, H, W, C), dev)
    _lib.call("xp_dwconv3x3_silu_bwd", ptr(x), ptr(w9c), ptr(dy), ptr(dx), ptr(dw), B, H, W, C, ptr(scale), ptr(ws), ctypes.c_size_t(ws.numel()),
              _lib.current_stream(x) if stream is None else stream)
    return dx, dw, scale


def gelu_fwd(x, stream=None):
    """GELU (erf form) with the function of the dense engine's act = 1 epilogue: gemm (act 0) -> gelu_fwd equals gemm (act 1) bit for bit."""
    _check_operands("gelu_fwd", x)
    x = x.contiguous()
    y = torch.empty_like(x)
    if x.numel():
        _lib.call("xp_gelu_fwd", ptr(x), ptr(y), x.numel(), _lib.current_stream(x) if stream is None else stream)
    return y


def gelu_bwd(dy, x, scaled=False, stream=None):
    """dx = dy (Phi(x) + x phi(x)) -> (dx, scale).  scaled: dx holds S x the gradient and scale = {S, 1 / S}; else scale is None."""
    _check_operands("gelu_bwd", dy, x)
    if dy.shape != x.shape or not x.numel():
        raise ValueError("gelu_bwd: dy must have the shape of x, and x at least one element")
    dy, x = dy.contiguous(), x.contiguous()
    dx = torch.empty_like(x)
    scale = torch.empty(2, dtype=torch.float32, device=x.device) if scaled else None
    ws = _scale_ws(x.device) if scaled else None
    _lib.call("xp_gelu_bwd", ptr(dy), ptr(x), ptr(dx), x.numel(), ptr(scale), ptr(ws), ctypes.c_size_t(ws.numel() if scaled else 0),
              _lib.current_stream(x) if stream is None else stream)
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
    _lib.call("xp_add_scaled_rows", ptr(x), ptr(r), ptr(s.contiguous()), ptr(y), B, r.numel() // (B * C), C, _lib.current_stream(r) if stream is None else stream)
    return y


def _layernorm(x, w, b, stream):
    y = torch.empty_like(x)
    _lib.call("xp_layernorm", ptr(x), ptr(y), ptr(w.contiguous()), ptr(b.contiguous()), x.shape[0], x.shape[1], LN_EPS, 0, stream)
    return y


def _linear(a, w, stream, bias=None, res=None, act=0):
    """epilogue(a (M, K) w (N, K)^T) [+ res] on the forward engine: K % 4 == 0."""
    N, K = w.shape
    out = torch.empty((a.shape[0], N), dtype=torch.float32, device=a.device)
    return _gemm_nt_h2(a, _split_h2(w, stream=stream), N, K, out, bias=None if bias is None else bias.contiguous(), act=act, stream=stream, res=res)


def _linear_dgrad(gs, scale, w, stream, res=None):
    """The input gradient g w [+ res] of a linear layer from gs = S g and scale = {S, 1 / S}: the forward engine on the transposed weight, 1 / S in
    the epilogue's scale vector.  w (N, K) with N % 4 == 0 (the engine's reduction length here)."""
    N, K = w.shape
    out = torch.empty((gs.shape[0], K), dtype=torch.float32, device=gs.device)
    return _gemm_nt_h2(gs, _split_h2(_transposed(w), stream=stream), K, N, out, scale=scale[1:2].expand(K).contiguous(),
                       shift=torch.zeros(K, dtype=torch.float32, device=gs.device), stream=stream, res=res)


def _dt_block_diagonal(dt_w, R2):
    """dt_projs_weight (4, C, R) as ONE (4 C, 4 (R + 2)) weight over the whole x_proj row: direction k's block under its own dt entries, zeros under
    the B / C entries and the other directions (K = R alone is no multiple of 4: R = 6 at C = 96, 2 at C = 32)."""
    K, C, R = dt_w.shape
    wbd = torch.zeros((K, C, K, R2), dtype=torch.float32, device=dt_w.device)
    for k in range(K):
        wbd[k, :, k, :R] = dt_w[k]
    return wbd.view(K * C, K * R2)


class _SsmBranchFn(torch.autograd.Function):
    """x (M, C) rows of (B, H, W) -> x + s[b] out_proj(out_norm(SS2D(silu(dwconv(in_proj(LN(x))))))); s None: no factor, the residual rides in the
    out_proj launch.  Parameters in the reference's order."""

    @staticmethod
    def forward(ctx, x, s, dims, norm_w, norm_b, xproj_w, A_logs, Ds, dt_w, dt_b, on_w, on_b, in_w, conv_w, out_w):
        from .kernels import _cross_merge, _cross_scan, _selective_scan_fn_nograd
        B, H, W = dims
        M, C = x.shape
        R = dt_w.shape[2]
        R2, L = R + 2, H * W
        st = _lib.current_stream(x)
        t1 = _layernorm(x, norm_w, norm_b, st)
        t2 = _linear(t1, in_w, st)
        w9c = conv_w.reshape(C, 9).t().contiguous()
        t3 = torch.empty_like(t2)
        _lib.call("xp_dwconv3x3_silu", ptr(t2), ptr(w9c), ptr(t3), B, H, W, C, st)
        xd = _linear(t3, xproj_w.reshape(4 * R2, C), st)                              # x_proj in pixel layout: (M, 4 (R + 2))
        wbd = _dt_block_diagonal(dt_w, R2)
        dtp = _linear(xd, wbd, st)                                                     # (M, 4 C): every direction's dt at its pixel
        xs = _cross_scan(t3.view(B, H, W, C), False, True, False, 0)                   # (B, 4, C, L)
        dts = _cross_scan(dtp.view(B, H, W, 4, C), False, True, True, 0)               # one_by_one, channel-last in: (B, 4, C, L)
        bc = _cross_scan(xd.view(M, 4, R2)[:, :, R:].reshape(B, H, W, 4, 2), False, True, True, 0)      # (B, 4, 2, L): B and C (d_state 1)
        Bs, Cs = bc[:, :, 0:1].contiguous(), bc[:, :, 1:2].contiguous()
        A = -torch.exp(A_logs.detach().float())
        ys, xstate = _selective_scan_fn_nograd(xs.view(B, 4 * C, L), dts.view(B, 4 * C, L), A, Bs, Cs, Ds.detach(), dt_b.detach().reshape(-1), True, want_x=True)
        ym = _cross_merge(ys.view(B, 4, C, H, W), False, True, False, 0).view(M, C)
        yn = _layernorm(ym, on_w, on_b, st)
        if s is None:
            out = _linear(yn, out_w, st, res=x)
        else:
            out = add_scaled_rows(x.view(B, L, C), _linear(yn, out_w, st).view(B, L, C), s, stream=st).view(M, C)
        ctx.dims, ctx.has_s = dims, s is not None
        ctx.save_for_backward(x, t1, t2, t3, xd, xs, dts, Bs, Cs, A, xstate, ym, yn, w9c, wbd, norm_w, xproj_w, Ds, dt_w, dt_b, on_w, in_w, out_w,
                              *(() if s is None else (s,)))
        return out

    @staticmethod
    def backward(ctx, dy):
        from .kernels import _cross_merge, _cross_scan, selective_scan_bwd
        x, t1, t2, t3, xd, xs, dts, Bs, Cs, A, xstate, ym, yn, w9c, wbd, norm_w, xproj_w, Ds, dt_w, dt_b, on_w, in_w, out_w = ctx.saved_tensors[:23]
        B, H, W = ctx.dims
        M, C = x.shape
        R = dt_w.shape[2]
        R2, L = R + 2, H * W
        st = _lib.current_stream(x)
        dy = dy.contiguous()
        g = add_scaled_rows(None, dy.view(B, L, C), ctx.saved_tensors[23], stream=st).view(M, C) if ctx.has_s else dy
        gs, sc = scale_grad(g, stream=st)
        d_out_w = gemm_tn(gs, yn, p_scale=sc, stream=st)
        dyn = _linear_dgrad(gs, sc, out_w, st)
        dym, d_on_w, d_on_b, _ = layernorm_bwd(dyn, ym, on_w, stream=st)
        dys = _cross_scan(dym.view(B, H, W, C), False, True, False, 0)                 # the merge's adjoint: (B, 4, C, L)
        du, ddelta, dA, dB, dC, dD, ddb = selective_scan_bwd(xs.view(B, 4 * C, L), dts.view(B, 4 * C, L), A, Bs, Cs, Ds, dt_b.reshape(-1),
                                                             dys.view(B, 4 * C, L), xstate, True, 1)
        dt3 = _cross_merge(du.view(B, 4, C, H, W), False, True, False, 0).view(M, C)   # the scan's adjoint
        ddtp = _cross_merge(ddelta.view(B, 4, C, H, W), False, True, True, 0).view(M, 4 * C)
        dbc = _cross_merge(torch.cat([dB, dC], 2).view(B, 4, 2, H, W), False, True, True, 0).view(M, 4, 2)
        # the dt projection: one block-diagonal GEMM over the whole x_proj row; its weight gradient is the diagonal blocks of one gemm_tn result
        g2, sc2 = scale_grad(ddtp, out=ddtp, stream=st)
        d_wbd = gemm_tn(g2, xd, p_scale=sc2, stream=st).view(4, C, 4, R2)
        d_dt_w = torch.stack([d_wbd[k, :, k, :R] for k in range(4)], 0)
        dxd = _linear_dgrad(g2, sc2, wbd, st)                                          # exact zeros under the B / C entries: wbd's columns there are 0
        dxd.view(M, 4, R2)[:, :, R:] = dbc
        g3, sc3 = scale_grad(dxd, out=dxd, stream=st)
        xw = xproj_w.reshape(4 * R2, C)
        d_xproj = gemm_tn(g3, t3, p_scale=sc3, stream=st).view(4, R2, C)
        dt3 = _linear_dgrad(g3, sc3, xw, st, res=dt3)                                  # + the scan's share, in the epilogue
        dt2, dw9c, sc4 = dwconv3x3_silu_bwd(t2.view(B, H, W, C), w9c, dt3.view(B, H, W, C), scaled=True, stream=st)
        dt2 = dt2.view(M, C)
        d_conv_w = dw9c.t().reshape(C, 1, 3, 3)
        d_in_w = gemm_tn(dt2, t1, p_scale=sc4, stream=st)
        dt1 = _linear_dgrad(dt2, sc4, in_w, st)
        dx, d_norm_w, d_norm_b, _ = layernorm_bwd(dt1, x, norm_w, stream=st)
        if ctx.needs_input_grad[0]:
            dx = add_scaled_rows(dy.view(B, L, C), dx.view(B, L, C), torch.ones(B, dtype=torch.float32, device=x.device), stream=st).view(M, C)
        else:
            dx = None
        # A = -exp(A_logs): dA_logs = dA A (parameter-sized)
        return dx, None, None, d_norm_w, d_norm_b, d_xproj, (dA * A).view(4 * C, 1), dD, d_dt_w, ddb.view(4, C), d_on_w, d_on_b, d_in_w, d_conv_w, d_out_w


class _MlpBranchFn(torch.autograd.Function):
    """x (M, C) rows of B samples -> x + s[b] fc2(GELU(fc1(LN(x)))); s None: no factor, the residual rides in the fc2 launch."""

    @staticmethod
    def forward(ctx, x, s, batch, n_w, n_b, w1, b1, w2, b2):
        M, C = x.shape
        st = _lib.current_stream(x)
        t = _layernorm(x, n_w, n_b, st)
        keep = any(ctx.needs_input_grad)
        if keep:
            pre = _linear(t, w1, st, bias=b1)
            h = gelu_fwd(pre, stream=st)
        else:                    # nothing to keep: the GELU rides in fc1's epilogue, the inference path's launch (the same bits)
            pre, h = None, _linear(t, w1, st, bias=b1, act=1)
        if s is None:
            out = _linear(h, w2, st, bias=b2, res=x)
        else:
            out = add_scaled_rows(x.view(batch, -1, C), _linear(h, w2, st, bias=b2).view(batch, -1, C), s, stream=st).view(M, C)
        ctx.batch, ctx.has_s = batch, s is not None
        if keep:
            ctx.save_for_backward(x, t, pre, h, n_w, w1, w2, *(() if s is None else (s,)))
        return out

    @staticmethod
    def backward(ctx, dy):
        x, t, pre, h, n_w, w1, w2 = ctx.saved_tensors[:7]
        M, C = x.shape
        B = ctx.batch
        st = _lib.current_stream(x)
        dy = dy.contiguous()
        g = add_scaled_rows(None, dy.view(B, -1, C), ctx.saved_tensors[7], stream=st).view(M, C) if ctx.has_s else dy
        gs, sc = scale_grad(g, stream=st)
        db2 = colsum_rows(gs, sc, stream=st)
        dw2 = gemm_tn(gs, h, p_scale=sc, stream=st)
        dh = _linear_dgrad(gs, sc, w2, st)
        dpre, sc1 = gelu_bwd(dh, pre, scaled=True, stream=st)
        db1 = colsum_rows(dpre, sc1, stream=st)
        dw1 = gemm_tn(dpre, t, p_scale=sc1, stream=st)
        dt = _linear_dgrad(dpre, sc1, w1, st)
        dx, dn_w, dn_b, _ = layernorm_bwd(dt, x, n_w, stream=st)
        if ctx.needs_input_grad[0]:
            dx = add_scaled_rows(dy.view(B, -1, C), dx.view(B, -1, C), torch.ones(B, dtype=torch.float32, device=x.device), stream=st).view(M, C)
        else:
            dx = None
        return dx, None, None, dn_w, dn_b, dw1, db1, dw2, db2


def drop_path_rates(depths, drop_path_rate):
    """The reference's per-block stochastic-depth rates: linspace(0, DROP_PATH_RATE, sum(DEPTHS)) (VMamba.py:1289), as a flat list."""
    return [float(v) for v in torch.linspace(0, float(drop_path_rate), int(sum(depths)))]


def _drop_path_draws(p, seed, sample_ids, branch):
    """keep / (1 - p) per sample from the Philox stream keyed by (seed, 2 sample id + branch): a sample's draw never depends on its batch neighbours."""
    import numpy as np
    out = []
    for sid in sample_ids:
        u = np.random.Generator(np.random.Philox(key=[int(seed) & (2 ** 64 - 1), 2 * int(sid) + branch])).random()
        out.append(0.0 if u < p else 1.0 / (1.0 - p))
    return out


class VSSBlock(torch.nn.Module):
    """One VSS block of the VMamba encoder (reference VMamba.py:1153-1234; SS2D forwardv2 / forward_corev2 with v05_noz, d_state 1, SSM_RATIO 1.0, no
    convolution bias) with the reference's state_dict names under `{encoder}layers.{stage}.blocks.{block}.`:

        blk = training.VSSBlock.from_model(net, stage=0, block=1).cuda().train()
        y = blk(x_nhwc, seed=step)                                  # (B, H, W, C) -> (B, H, W, C); x may require grad: blocks stack
        net.load_state_dict(blk.state_dict(), strict=False)         # the inference model with the tuned block

    x = x + drop_path(op(norm(x))); x = x + drop_path(mlp(norm2(x))).  Dense layers run on the split-fp16 engine (their operands must stay below 65504 in
    magnitude: LayerNorm outputs and O(1) activations in this network); gradients of any finite range are accepted.  Stochastic depth (`.train()` and
    drop_path > 0): each branch of each sample is multiplied by keep / (1 - p), the draws keyed by (seed, sample id, branch) or given as
    drop_path_scale = (s1, s2).  In `.eval()`, or with rate 0, the residual adds ride in the dense launches, as in the inference path."""

    def __init__(self, dim, dt_rank=None, mlp_ratio=4.0, drop_path=0.0, stage=0, block=0, encoder="encoder."):
        super().__init__()
        C = self.dim = int(dim)
        if C % 4 or C > 1024 or C < 4:
            raise ValueError(f"VSSBlock: dim must be a multiple of 4 in [4, 1024] (got {dim})")
        R = self.dt_rank = int(dt_rank) if dt_rank is not None else (C + 15) // 16
        H4 = self.hidden = int(C * mlp_ratio)
        if H4 % 4:
            raise ValueError(f"VSSBlock: the MLP width {H4} must be a multiple of 4")
        self.drop_path = float(drop_path)
        if not 0.0 <= self.drop_path < 1.0:
            raise ValueError(f"VSSBlock: drop_path must be in [0, 1) (got {drop_path})")
        if encoder not in ("encoder.", "encoder_thermal.", "encoder_optical."):
            raise ValueError(f"VSSBlock: encoder must be 'encoder.', 'encoder_thermal.' or 'encoder_optical.' (got {encoder!r})")
        self.prefix = f"{encoder}layers.{int(stage)}.blocks.{int(block)}."
        nn = torch.nn
        blk = nn.Module()          # parameter containers with the reference's names, order and initialisation; forward() never calls them
        blk.norm = nn.LayerNorm(C)
        op = nn.Module()
        op.x_proj_weight = nn.Parameter(torch.empty(4, R + 2, C).uniform_(-C ** -0.5, C ** -0.5))
        op.A_logs = nn.Parameter(torch.zeros(4 * C, 1))                                  # log(arange(1, d_state + 1)), d_state 1
        op.Ds = nn.Parameter(torch.ones(4 * C))
        op.dt_projs_weight = nn.Parameter(torch.empty(4, C, R).uniform_(-R ** -0.5, R ** -0.5))
        dt = torch.exp(torch.rand(4, C) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3)).clamp(min=1e-4)
        op.dt_projs_bias = nn.Parameter(dt + torch.log(-torch.expm1(-dt)))               # softplus^-1 (VMamba.py:196-211)
        op.out_norm = nn.LayerNorm(C)
        op.in_proj = nn.Linear(C, C, bias=False)
        op.conv2d = nn.Conv2d(C, C, 3, padding=1, groups=C, bias=False)
        op.out_proj = nn.Linear(C, C, bias=False)
        blk.op = op
        blk.norm2 = nn.LayerNorm(C)
        mlp = nn.Module()
        mlp.fc1, mlp.fc2 = nn.Linear(C, H4), nn.Linear(H4, C)
        blk.mlp = mlp
        node = self
        parts = self.prefix.rstrip(".").split(".")
        for name in parts[:-1]:
            child = nn.Module()
            node.add_module(name, child)
            node = child
        node.add_module(parts[-1], blk)

    def t(self, leaf):
        """The parameter with the reference's name `prefix + leaf`."""
        mod, _, name = (self.prefix + leaf).rpartition(".")
        return getattr(self.get_submodule(mod), name)

    @classmethod
    def from_model(cls, net, stage, block, encoder="encoder."):
        """Block `block` of stage `stage` of a loaded models.XPoint (VMamba encoder), as a copy, with the reference's stochastic-depth rate for
        that block.  encoder: 'encoder.', or 'encoder_thermal.' / 'encoder_optical.' of a multispectral model."""
        sd = net.state_dict()
        pre = f"{encoder}layers.{int(stage)}.blocks.{int(block)}."
        if pre + "norm.weight" not in sd:
            raise RuntimeError(f"VSSBlock.from_model: the model holds no {pre}norm.weight")
        model = net.config['use_attention']['model_parameters']['MODEL']
        depths = list(model['VSSM']['DEPTHS'])
        rates = drop_path_rates(depths, model.get('DROP_PATH_RATE', 0.0))
        C, R = sd[pre + "norm.weight"].shape[0], sd[pre + "op.dt_projs_weight"].shape[2]
        blk = cls(C, dt_rank=R, mlp_ratio=sd[pre + "mlp.fc1.weight"].shape[0] / C, drop_path=rates[sum(depths[:int(stage)]) + int(block)],
                  stage=stage, block=block, encoder=encoder)
        own = blk.state_dict()
        missing = [k for k in own if k not in sd]
        if missing:
            raise RuntimeError(f"VSSBlock.from_model: the model holds no {missing[:3]}")
        blk.load_state_dict({k: sd[k] for k in own})
        return blk

    def forward(self, x_nhwc, drop_path_scale=None, seed=0, sample_ids=None):
        """x_nhwc (B, H, W, C) float32 on the GPU -> (B, H, W, C).  drop_path_scale = (s1, s2): two (B,) tensors that replace the stochastic-depth
        draws of the two branches; else, in training with drop_path > 0, the draws are keyed by (seed, sample_ids[b], branch) (sample_ids: default
        0 .. B - 1)."""
        _need_device(x_nhwc, "VSSBlock")
        if x_nhwc.dtype != torch.float32:
            raise TypeError(f"VSSBlock: the input must be float32, got {x_nhwc.dtype}")
        C = self.dim
        if x_nhwc.dim() != 4 or x_nhwc.shape[-1] != C:
            raise ValueError(f"VSSBlock: x_nhwc must be (B, H, W, {C}), got {tuple(x_nhwc.shape)}")
        if self.t("norm.weight").device != x_nhwc.device:
            raise _lib.XPointHipError("VSSBlock: parameters and x_nhwc live on different devices")
        B, H, W, _ = x_nhwc.shape
        dev = x_nhwc.device
        s1 = s2 = None
        if drop_path_scale is not None:
            s1, s2 = (torch.as_tensor(s, dtype=torch.float32, device=dev).contiguous() for s in drop_path_scale)
            if tuple(s1.shape) != (B,) or tuple(s2.shape) != (B,):
                raise ValueError(f"VSSBlock: drop_path_scale must be two ({B},) tensors")
        elif self.training and self.drop_path > 0.0:
            ids = range(B) if sample_ids is None else [int(v) for v in torch.as_tensor(sample_ids).reshape(-1).tolist()]
            if len(ids) != B:
                raise ValueError(f"VSSBlock: sample_ids must be ({B},)")
            s1, s2 = (torch.tensor(_drop_path_draws(self.drop_path, seed, ids, br), dtype=torch.float32, device=dev) for br in (0, 1))
        x = x_nhwc.contiguous().view(B * H * W, C)
        t = self.t
        with torch.cuda.device(dev):
            x = _SsmBranchFn.apply(x, s1, (B, H, W), t("norm.weight"), t("norm.bias"), t("op.x_proj_weight"), t("op.A_logs"), t("op.Ds"),
                                   t("op.dt_projs_weight"), t("op.dt_projs_bias"), t("op.out_norm.weight"), t("op.out_norm.bias"),
                                   t("op.in_proj.weight"), t("op.conv2d.weight"), t("op.out_proj.weight"))
            x = _MlpBranchFn.apply(x, s2, B, t("norm2.weight"), t("norm2.bias"), t("mlp.fc1.weight"), t("mlp.fc1.bias"), t("mlp.fc2.weight"),
                                   t("mlp.fc2.bias"))
        return x.view(B, H, W, C)
