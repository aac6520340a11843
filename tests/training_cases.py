"""Helpers shared by tests/test_gpu_head_training.py, tests/test_gpu_regnet_training.py and tests/test_gpu_vss_training.py: the comparison at the
project's f32 bar, seeded inputs, bit views, the materialised im2col of the two 3x3 paddings, the synthetic inference model and the loss / augmentation
configurations of the fine-tuning runs.  Nothing here calls a kernel of the training library."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import heads_f64 as Hd, regnet_f64 as Rg

TOL = 1e-4


def _close(got, ref, what, tol=TOL, scale=None):
    got = torch.as_tensor(np.asarray(got.detach().cpu() if torch.is_tensor(got) else got)).double()
    ref = torch.as_tensor(np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref)).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err, sc = float((got - ref).abs().max()), float(ref.abs().max()) if scale is None else scale
    print(f"{what}: err / scale = {err / max(sc, 1e-300):.2e} (scale {sc:.3e})")
    assert err <= tol * max(sc, 1e-30), (what, err, sc)


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _im2col(x_nhwc, mode="reflect"):
    """(B, H, W, Ci) -> (B H W, 9 Ci): the A operand of the 3x3 convolution with padding 1 of `mode`, taps row-major"""
    B, H, W, Ci = x_nhwc.shape
    xp = F.pad(x_nhwc.permute(0, 3, 1, 2), (1, 1, 1, 1), mode=mode)
    return torch.cat([xp[:, :, ky:ky + H, kx:kx + W].permute(0, 2, 3, 1).reshape(B * H * W, Ci) for ky in range(3) for kx in range(3)], 1).contiguous()


def _im2col_zero(x_nhwc):
    return _im2col(x_nhwc, mode="constant")


def _net(kind="regnet"):
    """The inference model on synthetic weights, on the GPU, in eval mode: 'vmamba' / 'conv' (the heads' configurations) or the one with the
    homography head."""
    from xpoint_amd import models, synth
    cfg = Rg.model_config() if kind == "regnet" else Hd.model_config(kind)
    net = models.XPoint(cfg)
    net.load_state_dict({k: torch.from_numpy(np.array(v, copy=True)) for k, v in synth.make_conv_xpoint_state_dict(cfg).items()} if kind == "conv" else
                        synth.make_torch_state_dict(cfg), strict=True)
    return net.to("cuda").eval()


LOSS_CFG = {'detector_loss': True, 'detector_use_cross_entropy': True, 'descriptor_loss': True, 'descriptor_loss_threshold': 4.0,
            'descriptor_loss_use_mask': True, 'sparse_descriptor_loss': False, 'sparse_descriptor_loss_num_cell_divisor': 64,
            'positive_margin': 1.0, 'negative_margin': 0.2, 'lambda_d': 250, 'lambda': 1.0, 'use_encoder_similarity': False,
            'homography_regression_loss': {'check': False, 'gamma': 1.0}, 'detector_loss_function': 'cross_entropy',
            'detector_handle_multiple_keypoints': 'hard_assignment', 'detector_dustbin_loss_weight': 1,
            'detector_focal_loss': {'use': False, 'alpha': 0.25, 'gamma': 2.0, 'reduction': 'mean'}}
AUG_CFG = {'photometric': {'enable': True, 'primitives': ['random_brightness', 'random_contrast', 'additive_gaussian_noise'], 'random_order': False,
                           'params': {'random_brightness': {'max_abs_change': 0.15}, 'random_contrast': {'strength_range': [0.3, 1.8]},
                                      'additive_gaussian_noise': {'stddev_range': [0, 0.06]}}},
           'homographic': {'enable': False}}         # the homographic branch needs room for a 128 x 128 crop; the heads' pair is 64 x 96
# the run with the homography head: the same two, with the regression term and the homographic branch switched on (256 x 256 pairs)
LOSS_CFG_HM = dict(LOSS_CFG, homography_regression_loss={'check': True, 'gamma': 1.0})
AUG_CFG_HM = dict(AUG_CFG, homographic={'enable': True, 'valid_border_margin': 0, 'border_reflect': True,
                                        'params': {'corner_homography': {'enable': False, 'params': {'patch_size': 128, 'rho': 32}}, 'translation': True,
                                                   'rotation': True, 'scaling': True, 'perspective': True, 'scaling_amplitude': 0.2,
                                                   'perspective_amplitude_x': 0.2, 'perspective_amplitude_y': 0.2, 'patch_ratio': 0.85, 'max_angle': 1.57,
                                                   'allow_artifacts': True, 'translation_overflow': 0.05}})
