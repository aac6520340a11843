"""Training losses on the HIP library: `XPointLoss` and `FocalLoss`, mirroring reference xpoint/utils/losses.py.

    from xpoint_amd import losses
    loss_fn = losses.XPointLoss(config['loss'])
    loss, loss_components = loss_fn({'data': data, 'pred': pred, 'pred2': pred2})
    loss.backward()

Same `default_config`, the same `dict_update` merge, the same `forward(loss_input_dict) -> (loss, loss_components)` with the same keys,
and the same `descriptor_loss(...) -> (loss, positive_dist, negative_dist)` / `detector_loss(fn, logits, keypoint_map, valid_mask) ->
(loss, components)` methods.  The two hot losses are `torch.autograd.Function`s whose forward and backward are HIP kernels
(csrc/desc_loss.hip, csrc/det_loss.hip); there is no eager fallback: without the library these raise.  The dense
descriptor loss never builds an (HW x HW) tensor, forward or backward.  Inputs are ordinary device tensors; `keypoints` and `valid_mask`
may be bool, uint8 or float.

Quirks of the reference that are reproduced (losses.py:688-755, homographies.py:498-508):
  - cell centres are (y, x) = (8 r + 4, 8 c + 4) with the hard-coded 8.0 / 4.0 whatever `space_to_depth_ratio` says; they are flipped to
    (x, y, 1), multiplied by `homography.inverse()`, divided by the third coordinate and flipped back (warp_points_pytorch);
  - a pair corresponds when the distance is `<=` the threshold; `homography*` may be None (the centres themselves), `valid_mask*` may be
    None (all valid), `descriptor_loss_use_mask: false` ignores the masks and divides by (Hc Wc)^2;
  - `norm_b = sum v2 * sum v1` is not clamped: a sample without a valid pair gives nan, as in the reference;
  - the loss runs in float32 whatever autocast produced (tensors_to_dtype(pred, torch.float));
  - the detector statistics compare with `label * valid` while the loss uses the unmasked label and masks the loss value; both
    detector losses of `forward` use the class-weighted criterion (`detector_loss_fn2`).
Differences, all deliberate: nothing is constructed with `.cuda()` and nothing is printed in `__init__`; `FocalLoss(debug=True)` draws
nothing; the class-level `default_config` is deep-copied before the merge (the reference's `dict_update` writes into it); every value of
`loss_components` is a Python float (the reference leaves the four TP/FP/FN/TN ratios as 0-d tensors) and a detector call costs one
device synchronisation, the descriptor components one more (the reference: three and three).  The 3x3 inverse is the adjugate evaluated in
float64 and rounded to float32 (element-wise, so a sample's geometry does not depend on its batch neighbours); it may differ from LAPACK's
float32 inverse in the last bit, which moves a correspondence only when a distance lies within ~1e-4 px of the threshold.  Cell masks are
the block products of the mask values; the backward carries them in fp16, which is exact for 0/1 masks.
Not built: `sparse_descriptor_loss: true`, `detector_handle_multiple_keypoints: 'soft_assignment'` and `detector_loss_function:
'cross_entropy_focal_blended'` raise NotImplementedError naming the key; any other unsupported value raises the reference's ValueError
(including the class default 'random_selection', which the reference itself rejects at losses.py:439).
"""
from __future__ import annotations

import copy
import ctypes
from typing import Optional, Tuple

import torch
from torch.nn import Module

from . import _lib
from .utils import dict_update

__all__ = ["XPointLoss", "FocalLoss", "DetectorCrossEntropy", "descriptor_loss_sums", "detector_loss_stats"]


def _tensors_to_dtype(data, dtype):
    """reference utils.tensors_to_dtype, without modifying the caller's dict"""
    out = {}
    for k, v in data.items():
        if type(v) is torch.Tensor:
            out[k] = v.to(dtype)
        elif type(v) is dict:
            out[k] = _tensors_to_dtype(v, dtype)
        else:
            out[k] = v
    return out


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------------
# dense descriptor loss
# ------------------------------------------------------------------------------------------------------------------------------------
class _DescriptorLossFn(torch.autograd.Function):
    """(d1, d2) -> per-sample sums of pos + neg (differentiable), [pos, neg] sums and norm_b (not differentiable)."""

    @staticmethod
    def forward(ctx, d1, d2, w1, w2, v1, v2, threshold, positive_margin, negative_margin, lambda_d):
        B, D, Hc, Wc = d1.shape
        lib = _lib.load()
        nbytes = int(lib.xp_descriptor_loss_workspace_bytes(B, D, Hc, Wc))
        if nbytes == 0:
            raise _lib.XPointHipError(f"descriptor loss: unsupported shape {tuple(d1.shape)} (D must be a multiple of 16, at most 256)")
        with torch.cuda.device(d1.device):
            ws = torch.empty(nbytes, dtype=torch.uint8, device=d1.device)
            sums = torch.empty(B, 3, dtype=torch.float32, device=d1.device)
            norm = torch.empty(B, dtype=torch.float32, device=d1.device)
            _lib.call("xp_descriptor_loss_fwd", _lib.ptr(d1), _lib.ptr(d2), _lib.ptr(w1), _lib.ptr(w2), _lib.ptr(v1), _lib.ptr(v2), B, D, Hc, Wc,
                      float(threshold), float(positive_margin), float(negative_margin), float(lambda_d), _lib.ptr(ws), ctypes.c_size_t(nbytes),
                      _lib.ptr(sums), _lib.ptr(norm), _lib.current_stream(d1))
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.ws = ws                      # the staged operand planes: the backward's only state (linear in Hc * Wc)
            ctx.args = (B, D, Hc, Wc, float(threshold), float(positive_margin), float(negative_margin), float(lambda_d))
        total, parts = sums[:, 0].contiguous(), sums[:, 1:].contiguous()
        ctx.mark_non_differentiable(parts, norm)
        return total, parts, norm

    @staticmethod
    def backward(ctx, g_total, _g_parts, _g_norm):
        B, D, Hc, Wc, thr, mp, mn, lam = ctx.args
        ws = ctx.ws
        coef = _f32c(g_total)
        with torch.cuda.device(ws.device):
            g1 = torch.empty(B, D, Hc, Wc, dtype=torch.float32, device=ws.device) if ctx.needs_input_grad[0] else None
            g2 = torch.empty(B, D, Hc, Wc, dtype=torch.float32, device=ws.device) if ctx.needs_input_grad[1] else None
            _lib.call("xp_descriptor_loss_bwd", _lib.ptr(coef), B, D, Hc, Wc, thr, mp, mn, lam, _lib.ptr(ws), ctypes.c_size_t(ws.numel()),
                      _lib.ptr(g1), _lib.ptr(g2), _lib.current_stream(ws))
        return (g1, g2) + (None,) * 8


def descriptor_loss_sums(d1, d2, w1=None, w2=None, v1=None, v2=None, threshold=8.0, positive_margin=1.0, negative_margin=0.2, lambda_d=250.0):
    """The kernel-level operator.  d1, d2 (B, D, Hc, Wc); w1, w2 (B, Hc*Wc, 2) warped cell centres (y, x) or None; v1, v2 (B, Hc*Wc) cell
    masks or None.  Returns (total (B), parts (B, 2) = [pos, neg], norm (B)): per-sample sums over all pairs and sum v2 * sum v1; `total` is
    differentiable with respect to d1 and d2."""
    assert d1.shape == d2.shape and d1.dim() == 4, "Descriptor shapes must match."
    if not d1.is_cuda:
        raise _lib.XPointHipError("descriptor loss: tensors must live on the GPU (xpoint_amd has no CPU fallback)")
    B, D, Hc, Wc = d1.shape
    d1 = d1.to(torch.float32).contiguous()
    d2 = d2.to(torch.float32).contiguous()
    w1, w2 = (None if w is None else _f32c(w).reshape(B, Hc * Wc, 2) for w in (w1, w2))
    v1, v2 = (None if v is None else _f32c(v).reshape(B, Hc * Wc) for v in (v1, v2))
    return _DescriptorLossFn.apply(d1, d2, w1, w2, v1, v2, threshold, positive_margin, negative_margin, lambda_d)


def _inverse3(h):
    """(B, 3, 3) inverse by the adjugate, element-wise in float64, rounded to float32."""
    m = h.detach().to(torch.float64)
    a, b, c, d, e, f, g, hh, i = (m[:, r, k] for r in range(3) for k in range(3))
    co = [e * i - f * hh, c * hh - b * i, b * f - c * e,
          f * g - d * i, a * i - c * g, c * d - a * f,
          d * hh - e * g, b * g - a * hh, a * e - b * d]
    det = a * co[0] + b * co[3] + c * co[6]
    return (torch.stack(co, dim=1) / det[:, None]).reshape(-1, 3, 3).to(torch.float32)


def warped_cell_centres(homography, B, Hc, Wc, device):
    """(B, Hc*Wc, 2) float32: the cell centres (8 r + 4, 8 c + 4) through homography.inverse() the way warp_points_pytorch does it,
    (y, x) order.  None for a None homography (the kernel then uses the centres themselves)."""
    if homography is None:
        return None
    hi = _inverse3(homography.to(device))
    y = (torch.arange(Hc, device=device, dtype=torch.float32) * 8.0 + 4.0).repeat_interleave(Wc)[None]
    x = (torch.arange(Wc, device=device, dtype=torch.float32) * 8.0 + 4.0).repeat(Hc)[None]
    row = lambda r: (hi[:, r, 0, None] * x + hi[:, r, 1, None] * y) + hi[:, r, 2, None]      # noqa: E731
    X, Y, Z = row(0), row(1), row(2)
    return torch.stack((Y / Z, X / Z), dim=-1).contiguous()


def cell_mask(mask, B, Hc, Wc):
    """prod over every 8x8 block of a (B, 1, 8Hc, 8Wc) or (B, 8Hc, 8Wc) mask -> (B, Hc*Wc) float32 (space_to_depth + prod)."""
    m = mask.detach().to(torch.float32).reshape(B, Hc, 8, Wc, 8)
    return m.permute(0, 1, 3, 2, 4).reshape(B, Hc * Wc, 64).prod(dim=-1)


# ------------------------------------------------------------------------------------------------------------------------------------
# detector loss
# ------------------------------------------------------------------------------------------------------------------------------------
class _DetectorLossFn(torch.autograd.Function):
    """logits -> per-sample sum of loss * valid (differentiable) and the (B, 8) float64 statistics."""

    @staticmethod
    def forward(ctx, logits, kp, mask, noise, kind, dustbin_weight, alpha, gamma):
        B, C, Hc, Wc = logits.shape
        dev = logits.device
        with torch.cuda.device(dev):
            labels = torch.empty(B, Hc * Wc, dtype=torch.int32, device=dev)
            valid = torch.empty(B, Hc * Wc, dtype=torch.float32, device=dev)
            cell_loss = torch.empty(B, Hc * Wc, dtype=torch.float32, device=dev)
            code = torch.empty(B, Hc * Wc, dtype=torch.int32, device=dev)
            stats = torch.empty(B, 8, dtype=torch.float64, device=dev)
            _lib.call("xp_detector_loss_fwd", _lib.ptr(logits), _lib.ptr(kp), _lib.ptr(mask), _lib.ptr(noise), B, Hc, Wc, int(kind),
                      float(dustbin_weight), float(alpha), float(gamma), _lib.ptr(labels), _lib.ptr(valid), _lib.ptr(cell_loss), _lib.ptr(code),
                      _lib.ptr(stats), _lib.current_stream(logits))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(logits, labels, valid)
            ctx.args = (B, Hc, Wc, int(kind), float(dustbin_weight), float(alpha), float(gamma))
        total = stats[:, 0].to(torch.float32)
        ctx.mark_non_differentiable(stats)
        return total, stats

    @staticmethod
    def backward(ctx, g_total, _g_stats):
        logits, labels, valid = ctx.saved_tensors
        B, Hc, Wc, kind, w, alpha, gamma = ctx.args
        coef = _f32c(g_total)
        with torch.cuda.device(logits.device):
            dlogits = torch.empty_like(logits)
            _lib.call("xp_detector_loss_bwd", _lib.ptr(logits), _lib.ptr(labels), _lib.ptr(valid), _lib.ptr(coef), B, Hc, Wc, kind, w, alpha, gamma,
                      _lib.ptr(dlogits), _lib.current_stream(logits))
        return (dlogits,) + (None,) * 7


def detector_loss_stats(logits, keypoint_map, valid_mask, noise, kind, dustbin_weight=1.0, alpha=0.25, gamma=2.0):
    """The kernel-level operator.  logits (B, 65, Hc, Wc); keypoint_map (B, 8Hc, 8Wc); valid_mask the same (or with a unit channel axis) or
    None; noise (B, 64, Hc, Wc).  kind 0 cross entropy (dustbin class weight), 1 focal.  Returns (total (B) = sum of loss * valid,
    differentiable in logits; stats (B, 8) float64 = [total, sum valid, correct, TP, FP, FN, TN, 0])."""
    assert logits.dim() == 4, f"Logits must be a 4D tensor, got {logits.dim()}D."
    assert keypoint_map.dim() == 3, f"Keypoint map must be a 3D tensor, got {keypoint_map.dim()}D."
    if not logits.is_cuda:
        raise _lib.XPointHipError("detector loss: tensors must live on the GPU (xpoint_amd has no CPU fallback)")
    B, C, Hc, Wc = logits.shape
    assert C == 65, f"Logits must have 65 channels, got {C}."
    assert tuple(keypoint_map.shape) == (B, Hc * 8, Wc * 8), "Keypoint map must be (batch_size, 8 * Hc, 8 * Wc)."
    kp = _f32c(keypoint_map)
    mask = None
    if valid_mask is not None:
        assert valid_mask.numel() == kp.numel(), "Valid mask must have the same shape as keypoint_map."
        mask = _f32c(valid_mask).reshape(B, Hc * 8, Wc * 8)
    assert tuple(noise.shape) == (B, 64, Hc, Wc), "noise must be (batch_size, 64, Hc, Wc)."
    return _DetectorLossFn.apply(logits.to(torch.float32).contiguous(), kp, mask, _f32c(noise), kind, dustbin_weight, alpha, gamma)


class FocalLoss(Module):
    """Focal loss (https://arxiv.org/pdf/1708.02002.pdf) with the reference's interface.  As a detector criterion of XPointLoss only its
    alpha / gamma are read (the fused kernel evaluates it); `forward` is the plain torch statement for stand-alone use.  `debug` is
    accepted and ignored (the reference prints and plots)."""

    def __init__(self, alpha: float = 0.25, gamma: float = 2.0, reduction: str = 'none', debug=False):
        super().__init__()
        self.alpha = alpha
        self.gamma = gamma
        self.reduction = reduction
        self.debug = debug

    def forward(self, inputs: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        ce_loss = torch.nn.functional.cross_entropy(inputs, targets, reduction='none', weight=None)
        pt = torch.exp(-ce_loss)
        focal_loss = self.alpha * (1 - pt) ** self.gamma * ce_loss
        if self.reduction == 'mean':
            return focal_loss.mean()
        if self.reduction == 'sum':
            return focal_loss.sum()
        return focal_loss


class DetectorCrossEntropy(Module):
    """torch.nn.CrossEntropyLoss(weight=[1] * 64 + [dustbin_weight], reduction='none') as a detector criterion: the weights stay on the host
    (the reference's `_get_class_weights` calls `.cuda()`); `forward` is the plain torch statement for stand-alone use."""

    def __init__(self, dustbin_weight: float = 1.0):
        super().__init__()
        self.dustbin_weight = float(dustbin_weight)

    def forward(self, inputs: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        weight = torch.tensor([1.0] * 64 + [self.dustbin_weight], dtype=inputs.dtype, device=inputs.device)
        return torch.nn.functional.cross_entropy(inputs, targets, weight=weight, reduction='none')


class XPointLoss(Module):
    '''
    Loss to train the XPoint model with configurable detector and descriptor losses.
    '''
    default_config = {
        'detector_loss': True,
        'detector_loss_function': 'focal_loss',  # Options: 'cross_entropy', 'focal_loss'
        'detector_handle_multiple_keypoints': 'random_selection',  # the reference's default, which it rejects; use 'hard_assignment'
        'detector_dustbin_loss_weight': 1.0,
        'detector_label_normalization': False,
        'detector_focal_loss': {
            'use': True,
            'alpha': 0.25,
            'gamma': 2.0,
        },
        'descriptor_loss': True,
        'descriptor_loss_threshold': 8.0,
        'sparse_descriptor_loss': False,
        'sparse_descriptor_loss_num_cell_divisor': 64,
        'descriptor_loss_use_mask': True,
        'positive_margin': 1.0,
        'negative_margin': 0.2,
        'lambda_d': 250,
        'lambda': 0.0001,
        'space_to_depth_ratio': 8,
        'use_encoder_similarity': False,
        'homography_regression_loss': {
            'check': False,
            'gamma': 1.0,
        },
    }

    def __init__(self, config: Optional[dict] = None):
        super().__init__()
        self.config = copy.deepcopy(self.default_config)
        if config:
            self.config = dict_update(self.config, copy.deepcopy(dict(config)))
        self.cross_entropy_weights = [1] * 64 + [self.config['detector_dustbin_loss_weight']]
        self.criterion_encoder_similarity = torch.nn.CosineSimilarity(dim=1) if self.config['use_encoder_similarity'] else None
        self.criterion_hm_regressor = torch.nn.MSELoss() if self.config['homography_regression_loss']['check'] else None
        if self.config['space_to_depth_ratio'] != 8:
            raise NotImplementedError("space_to_depth_ratio: only 8 is built (the reference's descriptor loss hard-codes 8.0 / 4.0 as well)")
        if self.config['detector_loss']:
            loss_function = self.config['detector_loss_function']
            if loss_function == 'cross_entropy':
                self.detector_loss_fn1 = DetectorCrossEntropy(1.0)
                self.detector_loss_fn2 = DetectorCrossEntropy(self.config['detector_dustbin_loss_weight'])
            elif loss_function == 'focal_loss':
                focal_config = self.config['detector_focal_loss']
                if focal_config['use']:
                    self.detector_loss_fn1 = FocalLoss(alpha=focal_config['alpha'], gamma=focal_config['gamma'], reduction="none")
                    self.detector_loss_fn2 = self.detector_loss_fn1
                else:
                    raise ValueError("Focal Loss is not enabled in 'detector_focal_loss' config.")
            elif loss_function == 'cross_entropy_focal_blended':
                raise NotImplementedError("detector_loss_function: 'cross_entropy_focal_blended' is not built")
            else:
                raise ValueError(f"Unsupported detector_loss_function: {loss_function}")

    def forward(self, loss_input_dict: dict) -> Tuple[torch.Tensor, dict]:
        original_data_dict = loss_input_dict['data']
        data = original_data_dict['optical'] if "optical" in original_data_dict.keys() else original_data_dict
        data2 = original_data_dict['thermal'] if "optical" in original_data_dict.keys() else None
        pred = loss_input_dict['pred']
        pred2 = loss_input_dict['pred2'] if 'pred2' in loss_input_dict.keys() else None
        gt_hm = original_data_dict["hfour_points"] if "hfour_points" in original_data_dict.keys() else None
        pred_hm = loss_input_dict['pred_hm'] if 'pred_hm' in loss_input_dict.keys() else None

        if (pred2 is None and data2 is not None) or (pred2 is not None and data2 is None):
            raise ValueError('Both pred2 and data2 must be provided together to compute the loss.')
        if self.config["homography_regression_loss"]["check"] and (
                (gt_hm is not None and pred_hm is None) or (gt_hm is None and pred_hm is not None)):
            raise ValueError('Both ground truth homography and predicted homography must be provided for homography regression loss.')
        if self.config['use_encoder_similarity'] and pred2 is None:
            raise ValueError('Encoder similarity loss requires predictions from two images (pred and pred2).')

        pred = _tensors_to_dtype(pred, torch.float)
        if pred2 is not None:
            pred2 = _tensors_to_dtype(pred2, torch.float)

        device = data['keypoints'].device
        loss_components = {}
        loss = torch.tensor(0.0, device=device)

        if self.config['detector_loss']:
            detector_loss1, det1_components = self.detector_loss(self.detector_loss_fn2, pred['logits'], data['keypoints'], data['valid_mask'])
            loss = loss + detector_loss1
            loss_components.update({key + '1': value for key, value in det1_components.items()})
            if pred2 is not None:
                detector_loss2, det2_components = self.detector_loss(self.detector_loss_fn2, pred2['logits'], data2['keypoints'],
                                                                     data2['valid_mask'])
                loss = loss + detector_loss2
                loss_components.update({key + '2': value for key, value in det2_components.items()})

        if self.config['descriptor_loss']:
            if pred2 is None:
                raise ValueError('The descriptor loss requires predictions from two images.')
            descriptor_loss, positive_dist, negative_dist = self.descriptor_loss(
                pred['desc'], pred2['desc'], data.get('homography', None), data2.get('homography', None),
                data.get('valid_mask', None), data2.get('valid_mask', None))
            vals = torch.stack((descriptor_loss.detach(), positive_dist, negative_dist)).tolist()
            loss_components['descriptor_loss'], loss_components['positive_dist'], loss_components['negative_dist'] = vals
            loss = loss + self.config['lambda'] * descriptor_loss

        if self.config['homography_regression_loss']['check']:
            assert gt_hm is not None and pred_hm is not None, "Homography regression loss requires both gt_hm and pred_hm."
            gt_hm_processed = torch.nn.functional.normalize(gt_hm.view(-1, 8).float())
            homography_loss = self.criterion_hm_regressor(pred_hm, gt_hm_processed)
            loss = loss + self.config["homography_regression_loss"]["gamma"] * homography_loss
            loss_components['homography_regression_loss'] = homography_loss.item()

        if self.config['use_encoder_similarity']:
            assert pred2 is not None, "Encoder similarity loss requires predictions from two images."
            opt_flatten = pred['encoder_output'].flatten(start_dim=1)
            th_flatten = pred2['encoder_output'].flatten(start_dim=1)
            loss_encoder_sim = 1 - self.criterion_encoder_similarity(opt_flatten, th_flatten).mean()
            loss = loss + loss_encoder_sim
            loss_components['encoder_similarity_loss'] = loss_encoder_sim.item()

        return loss, loss_components

    def detector_loss(self, detector_loss_function, logits: torch.Tensor, keypoint_map: torch.Tensor, valid_mask: Optional[torch.Tensor] = None,
                      noise: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, dict]:
        """detector_loss_function: a FocalLoss or a DetectorCrossEntropy (self.detector_loss_fn1 / fn2).  noise: the (B, 64, Hc, Wc) uniform
        tensor that breaks ties between several keypoints of a cell; by default drawn like the reference does (torch.rand on the logits'
        device from the global generator)."""
        assert logits.dim() == 4, f"Logits must be a 4D tensor, got {logits.dim()}D."
        assert keypoint_map.dim() == 3, f"Keypoint map must be a 3D tensor, got {keypoint_map.dim()}D."
        handle_method = self.config['detector_handle_multiple_keypoints']
        if handle_method == 'soft_assignment':
            raise NotImplementedError("detector_handle_multiple_keypoints: 'soft_assignment' is not built")
        if handle_method != 'hard_assignment':
            raise ValueError(f"Unsupported detector_handle_multiple_keypoints method: {handle_method}")
        loss_function = self.config['detector_loss_function']
        if loss_function == 'cross_entropy' and isinstance(detector_loss_function, DetectorCrossEntropy):
            kind, w, alpha, gamma = 0, detector_loss_function.dustbin_weight, 0.0, 0.0
        elif loss_function == 'focal_loss' and isinstance(detector_loss_function, FocalLoss):
            kind, w, alpha, gamma = 1, 1.0, float(detector_loss_function.alpha), float(detector_loss_function.gamma)
        else:
            raise ValueError(f"Unsupported detector_loss_function: {loss_function}")
        B, _, Hc, Wc = logits.shape
        if noise is None:
            noise = torch.rand((B, 64, Hc, Wc), device=logits.device)
        total, stats = detector_loss_stats(logits, keypoint_map, valid_mask, noise, kind, w, alpha, gamma)
        normalized_loss = (total / stats[:, 1].to(torch.float32).clamp(min=1.0)).mean()
        host = torch.cat((stats.sum(dim=0), normalized_loss.detach().to(torch.float64).view(1))).tolist()      # the call's one synchronisation
        n = float(B * Hc * Wc)
        correct = host[2]
        loss_components = {
            'correct_ratio': correct / n,
            'incorrect_ratio': (n - correct) / n,
            'TP_ratio': host[3] / n,
            'FP_ratio': host[4] / n,
            'FN_ratio': host[5] / n,
            'TN_ratio': host[6] / n,
            'detector_loss': host[0] / n,
            'detector_normalized_loss': host[8],
        }
        return normalized_loss, loss_components

    def descriptor_loss(self, descriptor1: torch.Tensor, descriptor2: torch.Tensor, homography1: Optional[torch.Tensor],
                        homography2: Optional[torch.Tensor], valid_mask1: Optional[torch.Tensor] = None,
                        valid_mask2: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        assert descriptor1.shape == descriptor2.shape, "Descriptor shapes must match."
        if homography1 is not None and homography2 is not None:
            assert homography1.shape == homography2.shape, "Homography shapes must match."
            assert descriptor1.shape[0] == homography1.shape[0], "Batch size of descriptors and homographies must match."
        if self.config['sparse_descriptor_loss']:
            raise NotImplementedError("sparse_descriptor_loss: true is not built (only the dense descriptor loss is)")
        B, _, Hc, Wc = descriptor1.shape
        dev = descriptor1.device
        w1 = warped_cell_centres(homography1, B, Hc, Wc, dev)
        w2 = warped_cell_centres(homography2, B, Hc, Wc, dev)
        v1 = v2 = None
        if self.config['descriptor_loss_use_mask']:
            v1 = None if valid_mask1 is None else cell_mask(valid_mask1.to(dev), B, Hc, Wc)
            v2 = None if valid_mask2 is None else cell_mask(valid_mask2.to(dev), B, Hc, Wc)
        total, parts, norm = descriptor_loss_sums(descriptor1, descriptor2, w1, w2, v1, v2, self.config['descriptor_loss_threshold'],
                                                  self.config['positive_margin'], self.config['negative_margin'], self.config['lambda_d'])
        loss = (total / norm).mean()
        positive_dist = (parts[:, 0] / norm).mean()
        negative_dist = (parts[:, 1] / norm).mean()
        return loss, positive_dist, negative_dist
