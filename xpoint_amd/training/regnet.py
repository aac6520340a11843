"""The homography regression head (reference xpoint/models/RegNet.py) in training mode behind the same frozen encoder as the heads
(csrc/train_dense.hip, csrc/train_dgrad.hip, csrc/train_regnet.hip): two zero-padded 3x3 convolutions in the order conv -> BatchNorm -> ReLU, max
pool, F.normalize, the cost volume's global mean, and two linear layers with dropout.  Next to the heads' operators its backward uses the zero-padded
convolution's weight gradient (xp_conv3x3_zp_wgrad_h2) and INPUT gradient (xp_conv3x3_dgrad_h2: the forward engine on the rotated, transposed
weight), the ReLU / max-pool gates on the BatchNorm output, the cost volume's backward and a counter-based dropout.  The two linear layers take their
input gradient by `_linear_dgrad_tn` (section 15 says why), not by the forward engine."""
import torch

from .. import _lib
from .._lib import ptr
from .ops import (TrainModule, _conv3x3_zp_h2, _L2NormFn, _linear, _linear_dgrad_tn, _need_device, _relu, _split_h2, bn_train_bwd, bn_train_fwd,
                  colsum_rows, conv3x3_dgrad, conv3x3_wgrad_zero_pad, costvolume_mean_bwd, dropout_rows, gemm_tn, maxpool2_relu_bwd, relu_bwd)

_HM = "hm_regressor."


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


class _FcFn(torch.autograd.Function):
    """RegNet.fc in training mode: v (B, K) -> Linear(relu(Linear(dropout(v))) dropped again).  masks: (m1 (B, K), m2 (B, N1)) uint8 or None (drawn from
    seed and sample_ids with tags 0 and 1)."""

    @staticmethod
    def forward(ctx, v, w1, b1, w2, b2, p, seed, sample_ids, masks):
        st = _lib.current_stream(v)
        d1, m1 = dropout_rows(v, p, seed, sample_ids, 0, None if masks is None else masks[0], stream=st)
        h = _linear(d1, w1, st, bias=b1, act=2)
        d2, m2 = dropout_rows(h, p, seed, sample_ids, 1, None if masks is None else masks[1], stream=st)
        hm = _linear(d2, w2, st, bias=b2)
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
        dd2 = _linear_dgrad_tn(dhm, w2, st)
        dh, _ = dropout_rows(dd2, ctx.p, mask=m2, stream=st)
        dpre = relu_bwd(dh, h, stream=st)
        dw1 = gemm_tn(dpre, d1, stream=st)
        db1 = colsum_rows(dpre, stream=st)
        dd1 = _linear_dgrad_tn(dpre, w1, st)
        dv, _ = dropout_rows(dd1, ctx.p, mask=m1, stream=st)
        return dv, dw1, db1, dw2, db2, None, None, None, None


class RegNetHead(TrainModule):
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

    @classmethod
    def from_model(cls, net):
        """The homography head of a loaded models.XPoint (configuration with homography_regression_head), as a copy."""
        return cls()._load_slice(net.state_dict(), exempt="num_batches_tracked", strict=False)

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
                from ..convmodels import regnet_forward, regnet_weights
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
                self._update_running([(_HM + "layer1.1.", m1[0], v1), (_HM + "layer1.4.", m2[0], v2)], rows)
                feats.append(_L2NormFn.apply(a.view(B * hw, -1)).view(B, hw, -1))
                taps['y1'].append(y1); taps['y2'].append(y2)
            self.last_taps = taps if keep_taps else None
            v = _CostVolumeFn.apply(feats[0], feats[1])
            return _FcFn.apply(v, fw1, self.t(_HM + "fc.1.bias"), fw2, self.t(_HM + "fc.4.bias"), self.DROPOUT_P, int(seed), sample_ids, dropout_masks)
