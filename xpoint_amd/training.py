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
Not built: autocast / GradScaler training, the RegNet head's training, a training command line."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import ptr

__all__ = ["XPointHeads", "finetune_step", "gemm_tn", "conv3x3_wgrad", "bn_train_fwd", "bn_train_bwd", "colsum_rows", "l2norm_rows_bwd"]

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


def _split_h2(w_nk, stream=None):
    N, K = w_nk.shape
    out = torch.empty(_lib.load().xp_split_weights_h2_bytes(N, K), dtype=torch.uint8, device=w_nk.device)
    _lib.call("xp_split_weights_h2", ptr(w_nk.contiguous()), ctypes.c_void_p(out.data_ptr()), N, K, _lib.current_stream(w_nk) if stream is None else stream)
    return out


def _gemm_nt_h2(a, wsplit, N, K, out, bias=None, scale=None, shift=None, act=0, stream=None):
    """out (M, N; ld) = epilogue(a (M, K; ld) @ W^T) on the forward's split-fp16 engine."""
    _lib.call("xp_gemm_nt_h2", _vp(a), ctypes.c_void_p(wsplit.data_ptr()), _vp(out), ptr(bias), ptr(scale), ptr(shift), None, a.shape[0], N, K,
              int(a.stride(0)), int(out.stride(0)), 0, act, _lib.current_stream(a) if stream is None else stream)
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


def finetune_step(net, heads, data, loss_fn, optimizer):
    """One head fine-tuning step on a pair batch `data` = {'optical': {'image', 'keypoints', 'valid_mask', 'homography', ...}, 'thermal': {...}}
    (augmentation.augment_pair_batch's dict).  The frozen `net` (eval) produces the encoder output of both spectra in one forward; `heads` runs
    once per spectrum, so each spectrum has its own batch statistics and the running statistics update twice, as the reference's forward_impl
    does per call (XPoint.py:283-323).  Returns (loss, loss_components)."""
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
    loss, components = loss_fn({'data': data, 'pred': pred, 'pred2': pred2})
    loss.backward()
    optimizer.step()
    return loss.detach(), components
