"""A float64 restatement of the whole VMamba encoder (reference xpoint/models/vmamba_src/VMamba.py:1507-1525 VSSM.forward: patch embed :1405-1420,
the VSS blocks, downsample v3 :1433-1440, depth_to_space(4) :1500-1505) in plain torch on the CPU: F.conv2d, F.layer_norm, F.gelu, vss_block64 of
tests/vss_f64.py and the reference's depth_to_space.  The test side of xpoint_amd.training.VSSEncoder: tests/test_cpu_encoder_training.py pins it
against the real reference (tests/golden/g33_encoder_training.npz, tools/make_golden_encoder_training.py) and by gradcheck;
tests/test_gpu_encoder_training.py compares the HIP encoder against it.

Inputs are hash uniforms (synth.uniform); weights are those of synth.make_state_dict for the reference's XPoint with the case's EMBED_DIM and DEPTHS."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import vss_f64 as V
from xpoint_amd import synth

# case -> (EMBED_DIM, DEPTHS, image shape (B, 1, H, W))
CASES = {
    "S": (32, [1, 1, 1, 1], (2, 1, 64, 96)),
    "R": (96, [1, 1, 1, 1], (1, 1, 32, 64)),       # the real channel counts 48 / 96 / ... / 768
    "D": (32, [2, 1, 1, 1], (2, 1, 32, 32)),       # stacking inside a stage, with given stochastic-depth factors
}
GOLDEN_CASES = ("S",)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g33_encoder_training.npz")
PRE = "encoder."
# the per-sample factors (s1, s2) of case D's five blocks in its given-factor run: a dropped branch, a dropped sample, both kept
D_FACTORS = [([1.0, 1.0], [1.0, 1.0]), ([0.0, 1.25], [1.25, 0.0]), ([1.25, 1.25], [0.0, 0.0]), ([1.0, 0.5], [1.0, 1.0]), ([1.25, 0.0], [1.25, 0.0])]


def model_config(case):
    E, depths, (_, _, H, W) = CASES[case]
    return synth.xpoint_exp1_config(H, W, vssm={"EMBED_DIM": int(E), "DEPTHS": list(depths)})


def encoder_keys(case):
    """The reference's `encoder.*` names of the case's model, in its order."""
    return [k for k in synth.xpoint_state_spec(model_config(case)) if k.startswith(PRE)]


@functools.lru_cache(maxsize=None)
def _state(case):
    return synth.make_state_dict(model_config(case))


def encoder_state(case, dtype=torch.float64):
    """{name: tensor} of every `encoder.*` tensor of the case's model, full names, the reference's order."""
    sd = _state(case)
    return {k: torch.from_numpy(np.array(sd[k], copy=True)).to(dtype) for k in encoder_keys(case)}


def case_inputs(case):
    """images (B, 1, H, W) in [0, 1] and the weights R (B, H / 8, W / 8, E / 2) of the scalar sum(out * R), float32."""
    E, _, shape = CASES[case]
    B, _, H, W = shape
    return (torch.from_numpy(synth.uniform(f"enc/{case}/img", shape, 0.0, 1.0)),
            torch.from_numpy(synth.uniform(f"enc/{case}/R", (B, H // 8, W // 8, E // 2), -1.0, 1.0)))


def conv_s2_ln64(x_nhwc, w, b, ln_w, ln_b):
    """LayerNorm(conv3x3 stride 2 padding 1): (B, H, W, Ci) -> (B, Ho, Wo, Co); w (Co, Ci, 3, 3)."""
    y = F.conv2d(x_nhwc.permute(0, 3, 1, 2), w, b, stride=2, padding=1).permute(0, 2, 3, 1)
    return F.layer_norm(y, (w.shape[0],), ln_w, ln_b, 1e-5)


def stem64(images, w, b, ln_w, ln_b):
    """GELU(LayerNorm(conv3x3 stride 2 of the gray image replicated to 3 channels)): (B, 1, H, W) -> (B, Ho, Wo, E / 2); w (E / 2, 3, 3, 3)."""
    y = F.conv2d(torch.cat((images, images, images), 1), w, b, stride=2, padding=1).permute(0, 2, 3, 1)
    return F.gelu(F.layer_norm(y, (w.shape[0],), ln_w, ln_b, 1e-5))


def depth_to_space_ref(x, block_size):
    """VMamba.py:1500-1505 on (N, C, H, W)."""
    N, C, H, W = x.shape
    x = x.view(N, block_size, block_size, C // (block_size ** 2), H, W)
    x = x.permute(0, 3, 4, 1, 5, 2).contiguous()
    return x.view(N, C // (block_size ** 2), H * block_size, W * block_size)


def encoder64(p, images, depths, factors=None):
    """enc_nhwc (B, H / 8, W / 8, E / 2) from images (B, 1, H, W) and p = {full name: tensor}; factors: [(s1, s2)] per block or None.  Differentiable
    in every tensor of p."""
    g = lambda k: p[PRE + k]          # noqa: E731
    x = stem64(images, g("patch_embed.0.weight"), g("patch_embed.0.bias"), g("patch_embed.2.weight"), g("patch_embed.2.bias"))
    x = conv_s2_ln64(x, g("patch_embed.5.weight"), g("patch_embed.5.bias"), g("patch_embed.7.weight"), g("patch_embed.7.bias"))
    i = 0
    for s, depth in enumerate(depths):
        for j in range(depth):
            pre = f"{PRE}layers.{s}.blocks.{j}."
            s1, s2 = (None, None) if factors is None else (torch.as_tensor(f, dtype=x.dtype) for f in factors[i])
            x = V.vss_block64({k: p[pre + k] for k in V.LEAVES}, x, s1, s2)
            i += 1
        if s < len(depths) - 1:
            d = f"layers.{s}.downsample."
            x = conv_s2_ln64(x, g(d + "1.weight"), g(d + "1.bias"), g(d + "3.weight"), g(d + "3.bias"))
    return depth_to_space_ref(x.permute(0, 3, 1, 2), 4).permute(0, 2, 3, 1)


def encoder_step64(p, images, Rw, depths, factors=None):
    """{'out', 'grad/<full name>'} of sum(out * Rw), float64."""
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in p.items()}
    out = encoder64(p, images.double(), depths, factors)
    names = list(p)
    grads = torch.autograd.grad((out * Rw.double()).sum(), [p[k] for k in names])
    res = {"out": out.detach()}
    res.update({"grad/" + k: g for k, g in zip(names, grads)})
    return res


@functools.lru_cache(maxsize=None)
def case_reference(case, given_factors=False):
    """The restatement's step on the case's inputs (computed once per process; callers must not modify it)."""
    images, Rw = case_inputs(case)
    return encoder_step64(encoder_state(case), images, Rw, CASES[case][1], D_FACTORS if given_factors else None)


def golden():
    return np.load(GOLDEN)
