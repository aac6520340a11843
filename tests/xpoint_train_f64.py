"""A float64 restatement of one training step of the whole VMamba XPoint (reference XPoint.py:181-214 forward over a pair, :283-323 forward_impl) in
plain torch on the CPU: encoder_f64.encoder64 -> the heads of heads_f64 in training mode with the encoder output IN the graph -> the scalar
sum logits R1 + sum desc R2, per spectrum, summed over the two spectra.  The test side of xpoint_amd.training.XPointNet:
tests/test_cpu_xpoint_training.py pins it against the real reference (tests/golden/g34_xpoint_training.npz, tools/make_golden_xpoint_training.py),
tests/test_gpu_xpoint_training.py compares the HIP model against it.  The property all of this pins: the heads' loss reaches `encoder.*` through the
reflection-padded trunk convolution.

heads_f64.heads_f64 returns detached outputs and differentiates its own copies of the parameters, so the heads are restated here on the caller's
tensors (`heads64`); the CPU test checks that the two agree.  Also here: the fold identity of the reflection-padded convolution's input gradient
(`reflect_dgrad_by_fold`), the arithmetic of xp_conv3x3_rp_dgrad_h2 stated with zero-padded pieces only."""
import copy
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import encoder_f64 as En, heads_f64 as Hd
from xpoint_amd import synth

CASE = "S"          # encoder_f64's case: EMBED_DIM 32, DEPTHS [1, 1, 1, 1], images (2, 1, 64, 96)
SPECTRA = ("optical", "thermal")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g34_xpoint_training.npz")
FOLD_SHAPES = [(2, 2), (3, 3), (2, 9), (9, 2), (4, 5), (9, 7)]


def model_config(case=CASE, drop_path_rate=0.0, **over):
    """The case's configuration for training: the f32 class (`mixed_precision: false`; XPointNet refuses the autocast configuration) and, by default,
    no stochastic depth (the restatement and the reference's eval-mode encoder have none)."""
    return training_config(En.model_config(case), drop_path_rate, **over)


def training_config(cfg, drop_path_rate=0.0, **over):
    cfg = copy.deepcopy(cfg)
    cfg["mixed_precision"] = False
    cfg.update(over)
    cfg["use_attention"]["model_parameters"]["MODEL"]["DROP_PATH_RATE"] = float(drop_path_rate)
    return cfg


@functools.lru_cache(maxsize=None)
def _state(case):
    return synth.make_state_dict(model_config(case))


def model_state(case=CASE, dtype=torch.float64):
    """{name: tensor} of the case's model: every `encoder.*` tensor and the heads' parameters and buffers, the reference's names."""
    sd = _state(case)
    keep = [k for k in sd if k.startswith((En.PRE, Hd.DET, Hd.DSC))]
    return {k: (lambda t: t.to(dtype) if t.is_floating_point() else t)(torch.from_numpy(np.array(sd[k], copy=True))) for k in keep}


def is_parameter(name):
    return name.startswith(En.PRE) or name.endswith((".weight", ".bias"))


def case_inputs(case=CASE, seed=None):
    """{spectrum: (images (B, 1, H, W) in [0, 1], R1 (B, 65, Hc, Wc), R2 (B, D, Hc, Wc))}, float32 hash uniforms named by case and seed (default:
    case_seed)."""
    seed = case_seed(case) if seed is None else seed
    _, _, shape = En.CASES[case]
    B, _, H, W = shape
    D = _state(case)[Hd.DSC + "4.weight"].shape[0]
    u = lambda what, s, lo=-1.0, hi=1.0: torch.from_numpy(synth.uniform(f"xpt/{case}/{what}/{seed}", s, lo, hi))          # noqa: E731
    return {sp: (u(f"img/{sp}", shape, 0.0, 1.0), u(f"r1/{sp}", (B, 65, H // 8, W // 8)), u(f"r2/{sp}", (B, D, H // 8, W // 8))) for sp in SPECTRA}


@functools.lru_cache(maxsize=None)
def case_seed(case=CASE):
    """The first of the first eight seeds at which the float64 trunk pre-activations of BOTH spectra meet heads_f64's ReLU floor: the gradient jumps
    where a pre-activation is 0, so a comparison is only defined away from it (heads_f64.case_seed's rule, here behind the encoder)."""
    p = model_state(case)
    for seed in range(8):
        with torch.no_grad():
            margins = [Hd.relu_margin(heads64(p, En.encoder64(p, img.double(), En.CASES[case][1]).permute(0, 3, 1, 2))[2])
                       for img, _, _ in case_inputs(case, seed).values()]
        if min(margins) >= Hd.RELU_FLOOR:
            return seed
    raise RuntimeError(f"{case}: none of the first eight seeds meets the ReLU floor")


def heads64(p, x_nchw):
    """(logits, desc, trunk pre-activations) of the heads in training mode (batch statistics) on the tensors of p; differentiable in p and x."""
    def bn(z, pfx):
        return F.batch_norm(z, None, None, p[pfx + "weight"], p[pfx + "bias"], True, 0.1, 1e-5)

    pre = []

    def head(pfx):
        a = F.conv2d(F.pad(x_nchw, (1, 1, 1, 1), mode="reflect"), p[pfx + "1.weight"], p[pfx + "1.bias"])
        pre.append(a.detach())
        return bn(F.conv2d(bn(F.relu(a), pfx + "3."), p[pfx + "4.weight"], p[pfx + "4.bias"]), pfx + "5.")

    logits = head(Hd.DET)
    desc = F.normalize(head(Hd.DSC), p=2, dim=1)
    return logits, desc, torch.cat(pre, 1)


def model_step64(sd, inputs, depths):
    """One step of sum over spectra of (sum logits R1 + sum desc R2) in float64 -> {'logits/<spectrum>', 'desc/<spectrum>' (NCHW),
    'denc/<spectrum>' (the gradient of enc_nhwc), 'pre/<spectrum>', 'grad/<name>' of every parameter}."""
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items() if is_parameter(k)}
    res, encs, loss = {}, {}, 0.0
    for sp in SPECTRA:
        img, r1, r2 = inputs[sp]
        enc = En.encoder64(p, img.double(), depths)
        enc.retain_grad()
        logits, desc, pre = heads64(p, enc.permute(0, 3, 1, 2))
        loss = loss + (logits * r1.double()).sum() + (desc * r2.double()).sum()
        encs[sp] = enc
        res[f"logits/{sp}"], res[f"desc/{sp}"], res[f"pre/{sp}"] = logits.detach(), desc.detach(), pre
    loss.backward()
    for sp in SPECTRA:
        res[f"denc/{sp}"] = encs[sp].grad
    for k, v in p.items():
        res["grad/" + k] = v.grad
    return res


@functools.lru_cache(maxsize=None)
def case_reference(case=CASE):
    """The restatement's step on the case's inputs (computed once per process; callers must not modify it)."""
    return model_step64(model_state(case), case_inputs(case), En.CASES[case][1])


def zero_gradient_bias(name):
    """Whether `name` (a parameter name, with or without `grad/`) is one of the HEADS' `3.bias` / `4.bias`, whose gradient is zero in exact arithmetic
    (heads_f64.tensor_scale).  The encoder's `downsample.3.bias` shares the suffix and is an ordinary LayerNorm bias: it is not one of them."""
    name = name[len("grad/"):] if name.startswith("grad/") else name
    return name.startswith((Hd.DET, Hd.DSC)) and name.endswith(("3.bias", "4.bias"))


def tensor_scale(res, name):
    """The scale a comparison of `name` is measured on: the tensor's own largest magnitude — except for the heads' two zero-gradient biases, which
    heads_f64.tensor_scale measures on their sibling weight gradient's scale.  Every encoder tensor is measured on its own scale."""
    if zero_gradient_bias(name):
        return Hd.tensor_scale(res, name)
    return float(torch.as_tensor(np.asarray(res[name])).double().abs().max())


def golden():
    return np.load(GOLDEN)


# ---- the fold identity behind xp_conv3x3_rp_dgrad_h2
def zero_pad_dgrad_on_frame(dy, w):
    """g on the padded frame: (B, Ci, H + 2, W + 2) from dy (B, Co, H, W) and w (Co, Ci, 3, 3); g[..., v + 1, u + 1] = sum_k w[k]^T dy[v - ky + 1][u - kx + 1]
    with the terms outside dy absent (the full transposed convolution)."""
    return F.conv_transpose2d(dy, w)


def reflect_dgrad_by_fold(dy, w):
    """dx (B, Ci, H, W) of conv2d(reflection_pad(x), w): per axis dx[q] = g[q] + [q == 1] g[-1] + [q == n - 2] g[n]."""
    g = zero_pad_dgrad_on_frame(dy, w)
    for axis in (2, 3):
        n = g.shape[axis] - 2
        inner = g.narrow(axis, 1, n).clone()
        inner.narrow(axis, 1, 1).add_(g.narrow(axis, 0, 1))
        inner.narrow(axis, n - 2, 1).add_(g.narrow(axis, n + 1, 1))
        g = inner
    return g


def reflect_dgrad_autograd(dy, w):
    x = torch.zeros(dy.shape[0], w.shape[1], dy.shape[2], dy.shape[3], dtype=dy.dtype, requires_grad=True)
    (gx,) = torch.autograd.grad(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w), [x], dy)
    return gx
