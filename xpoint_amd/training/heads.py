"""Head fine-tuning over a frozen encoder: the detector and descriptor heads of the reference's XPoint (XPoint.py:112-138, 348-371) in
training mode, forward and backward on the HIP library (csrc/train_dense.hip, the trunk's input gradient in csrc/train_dgrad.hip; DESIGN.md sections 14, 20).

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
gradient by xp_gemm_nt_h2 on the transposed weight, F.normalize by xp_l2norm_rows_bwd, the trunk's input gradient by xp_conv3x3_rp_dgrad_h2.  Torch
only concatenates / permutes parameters and gradients.  There is no CPU fallback.  The public `forward` is the frozen-encoder path: an `enc_nhwc` that
requires grad raises NotImplementedError; training.XPointNet (model.py) is what passes the heads' gradient on to the encoder.
Activations must stay below 65504 in magnitude (the encoder output and the trunk's BatchNorm output: O(1) in this network)."""
import torch

from .. import _lib
from .ops import (BN_EPS, TrainModule, _conv3x3_h2, _gemm_nt_h2, _l2norm_rows, _L2NormFn, _linear, _linear_dgrad, _need_device, _pad4, _split_h2, bn_train_bwd,
                  bn_train_fwd, colsum_rows, conv3x3_dgrad_reflect, conv3x3_wgrad, gemm_tn)

_DET, _DSC = "detector_head_convolutions.", "descriptor_head_convolutions."


class _TrunkFn(torch.autograd.Function):
    """enc (B, Hc, Wc, Ci), w (Co, 3, 3, Ci), b, gamma, beta (Co) -> h = BN(relu(conv(enc))) (B, Hc, Wc, Co), batch mean, biased batch var."""

    @staticmethod
    def forward(ctx, enc, w, b, gamma, beta):
        B, H, W, _ = enc.shape
        Co = w.shape[0]
        st = _lib.current_stream(enc)            # looked up once per call: every launch below goes to it
        w = w.contiguous()
        a = _conv3x3_h2(enc, w, b.contiguous(), stream=st)
        h, mean, invstd, var = bn_train_fwd(a.view(B * H * W, Co), gamma.contiguous(), beta.contiguous(), stream=st)
        ctx.save_for_backward(enc, a, gamma, mean, invstd, w)
        ctx.mark_non_differentiable(mean, var)
        return h.view(B, H, W, Co), mean, var

    @staticmethod
    def backward(ctx, dh, _dm, _dv):
        enc, a, gamma, mean, invstd, w = ctx.saved_tensors
        B, H, W, Co = a.shape
        dh = dh.contiguous().view(B * H * W, Co)
        # the trunk's order is conv -> ReLU -> BatchNorm: the masked, scaled dx is the gradient of the convolution's output
        st = _lib.current_stream(enc)
        da, dgamma, dbeta, scale = bn_train_bwd(dh, a.view(B * H * W, Co), gamma.contiguous(), mean, invstd, relu_mask=True, scaled=True, stream=st)
        db = colsum_rows(da, scale, stream=st)
        dw = conv3x3_wgrad(enc, da.view(B, H, W, Co), scale, stream=st)
        denc = conv3x3_dgrad_reflect(da.view(B, H, W, Co), w, scale, stream=st) if ctx.needs_input_grad[0] else None
        return denc, dw, db, dgamma, dbeta


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
        for k, (do, w, g, z, mean, invstd) in enumerate(((do_det, w_det, g_det, z0, m0, i0), (do_dsc, w_dsc, g_dsc, z1, m1, i1))):
            C = w.shape[0]
            Cp = _pad4(C)
            do = torch.zeros((rows, C), dtype=torch.float32, device=h.device) if do is None else do.contiguous()
            dzp = torch.empty((rows, Cp), dtype=torch.float32, device=h.device)
            if Cp != C:
                dzp[:, C:] = 0.0                                                                # the pad columns of the A operand
            dz, dg, dbe, scale = bn_train_bwd(do, z, g.contiguous(), mean, invstd, scaled=True, dx=dzp[:, :C], stream=st)
            db = colsum_rows(dz, scale, stream=st)
            dw = gemm_tn(dz, h[:, k * Ch:(k + 1) * Ch], p_scale=scale, stream=st)
            _linear_dgrad(dzp, scale, w, st, out=dh[:, k * Ch:(k + 1) * Ch])                     # (S dz) W / S over the padded reduction length
            grads += [dw, db, dg, dbe]
        return (dh,) + tuple(grads)


class XPointHeads(TrainModule):
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

    @classmethod
    def from_model(cls, net):
        """The heads of a loaded models.XPoint (VMamba: Ci = EMBED_DIM / 2 = 48; conv encoder: Ci = 128), as a copy."""
        sd = net.state_dict()
        w1 = sd[_DET + "1.weight"]
        heads = cls(in_channels=w1.shape[1], head_channels=w1.shape[0], descriptor_size=sd[_DSC + "4.weight"].shape[0],
                    detector_channels=sd[_DET + "4.weight"].shape[0])
        return heads._load_slice(sd, exempt="num_batches_tracked", strict=False)

    def _affine(self, pre):
        scale = self.t(pre + "weight").double() / torch.sqrt(self.t(pre + "running_var").double() + BN_EPS)
        shift = self.t(pre + "bias").double() - self.t(pre + "running_mean").double() * scale
        return scale.float().contiguous(), shift.float().contiguous()

    def forward(self, enc_nhwc):
        """enc_nhwc (B, Hc, Wc, Ci) on the GPU -> {'logits': (B, 65, Hc, Wc), 'desc': (B, D, Hc, Wc)} (channel-last memory, NCHW shape)."""
        _need_device(enc_nhwc, "XPointHeads")
        if enc_nhwc.requires_grad:
            raise NotImplementedError("XPointHeads: the encoder is frozen on this path (training.XPointNet trains it); pass a detached enc_nhwc")
        if enc_nhwc.dim() != 4 or enc_nhwc.shape[-1] != self.in_channels:
            raise ValueError(f"XPointHeads: enc_nhwc must be (B, Hc, Wc, {self.in_channels}), got {tuple(enc_nhwc.shape)}")
        if self.t(_DET + "1.weight").device != enc_nhwc.device:
            raise _lib.XPointHipError("XPointHeads: parameters and enc_nhwc live on different devices")
        return self._forward(enc_nhwc.detach())

    def _forward(self, enc_nhwc):
        """forward's body on the tensor as it is: an enc_nhwc that requires grad receives the trunk's input gradient (training.XPointNet's path)."""
        enc = enc_nhwc.to(torch.float32).contiguous()
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
                        outs.append(_linear(h[:, k * Ch:(k + 1) * Ch], w4[k], None, bias=self.t(p + "4.bias"), scale=sc, shift=sh))
                    o_det, desc = outs[0], _l2norm_rows(outs[1])
        return {'logits': o_det.view(B, Hc, Wc, -1).permute(0, 3, 1, 2), 'desc': desc.view(B, Hc, Wc, -1).permute(0, 3, 1, 2)}


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
