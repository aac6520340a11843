"""Training on the HIP library, of the whole VMamba XPoint or of its parts over a frozen encoder: forward and backward of the trainable modules, HIP
only, no CPU fallback.

    ops.py      the operator level: one wrapper per training kernel, the shared forward launches, the module base
    heads.py    XPointHeads, finetune_step: the detector and descriptor heads (section 14)
    regnet.py   RegNetHead: the homography regression head (section 15)
    vss.py      VSSBlock: one block of the VMamba encoder, with its input gradient (section 16); set_ss2d_core: the form of its SS2D core (section 24)
    encoder.py  VSSEncoder: the whole VMamba encoder, patch embed and the downsamplers included (section 19)
    model.py    XPointNet, train_step, pretrain_step: encoder(s), heads and homography head as one model, the heads' loss reaching the encoder through the
                input gradient of the trunk's reflection-padded convolution (section 20)
    optim.py    Adam: the optimiser step as three kinds of launch, with a global-norm clip and a device-side guard against non-finite gradients
                (section 21)
    fit.py      fit: the training run of the reference's train.py (epochs, augmentation, schedule, validation, checkpoints); `cli train`

Not built: conv-encoder training, autocast / GradScaler training."""
from .encoder import VSSEncoder
from .fit import fit
from .heads import XPointHeads, finetune_step
from .model import XPointNet, pretrain_step, train_step
from .ops import (add_scaled_rows, bn_train_bwd, bn_train_fwd, colsum_rows, conv3x3_dgrad, conv3x3_dgrad_reflect, conv3x3_s2_dgrad, conv3x3_s2_fwd, conv3x3_s2_wgrad,
                  conv3x3_wgrad, conv3x3_wgrad_zero_pad, costvolume_mean_bwd, dropout_rows, dwconv3x3_silu_bwd, gelu_bwd, gelu_fwd, gemm_tn,
                  l2norm_rows_bwd, layernorm_bwd, maxpool2_relu_bwd, relu_bwd, scale_grad, ss2d_core, stem_conv, stem_conv_wgrad)
from .optim import Adam
from .regnet import RegNetHead
from .vss import VSSBlock, drop_path_rates, set_ss2d_core

__all__ = ["XPointHeads", "RegNetHead", "finetune_step", "gemm_tn", "conv3x3_wgrad", "bn_train_fwd", "bn_train_bwd", "colsum_rows", "l2norm_rows_bwd",
           "conv3x3_wgrad_zero_pad", "conv3x3_dgrad", "relu_bwd", "maxpool2_relu_bwd", "costvolume_mean_bwd", "dropout_rows",
           "VSSBlock", "layernorm_bwd", "dwconv3x3_silu_bwd", "gelu_fwd", "gelu_bwd", "add_scaled_rows", "scale_grad",
           "VSSEncoder", "conv3x3_s2_wgrad", "conv3x3_s2_dgrad", "conv3x3_s2_fwd", "stem_conv", "stem_conv_wgrad",
           "conv3x3_dgrad_reflect", "XPointNet", "train_step", "pretrain_step", "Adam", "fit", "ss2d_core", "set_ss2d_core"]
