"""Float64 restatement of the homography head in training mode (reference xpoint/models/RegNet.py:12-42: layer1 on each image with its own batch
statistics, F.normalize, the cost volume's global mean, fc with dropout) with torch autograd on the CPU, and the case table of its tests.  Pinned
against the real reference by tests/test_cpu_regnet_training.py (tests/golden/g31_regnet_training.npz, written by
tools/make_golden_regnet_training.py); the GPU tests compare xpoint_amd.training.RegNetHead with this restatement.

Inputs come from the hash RNG of xpoint_amd.synth: the weights are the synthetic state dict's `hm_regressor.*` slice, the two encoder tensors and the
cotangent R are hash uniforms named by case.  The objective of a case is  sum hm * R; the dropout masks are the ones the reference drew (stored in
the golden file) and are an INPUT here.

The gradient jumps where a ReLU input is 0 and where the two largest values of a pooling window meet.  A case has 3e5 to 1e6 such decisions, so no
seed keeps all of them away from the jump; instead `gates` lets a caller impose the decisions another implementation took —
{'relu1': [bool (B, 96, H, W)] * 2, 'relu2': [bool (B, 192, H / 2, W / 2)] * 2 (the window's maximum is > 0), 'pool': [int64 index 0..3 of the
window's winner, row-major] * 2}, one entry per image — on the BACKWARD pass only: the forward values never depend on them."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from xpoint_amd import synth

HM = "hm_regressor."
SHAPES = collections.OrderedDict((("1x32x32", (1, 32, 32)), ("3x16x64", (3, 16, 64)), ("2x64x16", (2, 64, 16))))      # B x H' x W' per spectrum
CASES = list(SHAPES)
# what the golden file keeps of the two convolution weights' gradients: [::stride] along the two leading dimensions
GOLDEN_STRIDES = {"layer1.0.weight": (4, 3), "layer1.3.weight": (8, 5)}
DROPOUT_P = 0.5


def model_config():
    return synth.xpoint_exp1_config(256, 256, hm_head=True)


@functools.lru_cache(maxsize=None)
def head_state():
    """The `hm_regressor.*` slice of the synthetic state dict, float32 torch tensors keyed by the reference's names, in its order."""
    out = collections.OrderedDict()
    for k, v in synth.make_torch_state_dict(model_config()).items():
        if k.startswith(HM):
            out[k] = v.clone()
    return out


def case_inputs(case):
    """(enc1, enc2 (B, 48, H', W'), R (B, 8)) float32 CPU tensors."""
    B, H, W = SHAPES[case]
    t = lambda what, shape: torch.from_numpy(synth.uniform(f"g31/{case}/{what}", shape, -1.0, 1.0))
    return t("enc1", (B, 48, H, W)), t("enc2", (B, 48, H, W)), t("r", (B, 8))


def windows(y):
    """(B, C, H, W) -> (B, C, H / 2, W / 2, 4): the 2 x 2 pooling windows, row-major inside the window (MaxPool2d floors odd sizes)."""
    B, C, H, W = y.shape
    y = y[:, :, :H // 2 * 2, :W // 2 * 2]
    return y.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def gates_of(y1, y2):
    """The decisions an implementation took, from its BatchNorm outputs y1, y2 (B, C, H, W) of ONE image: (relu1, relu2, pool).  The winner of a
    window is the FIRST position that attains the maximum (torch's max_pool2d)."""
    win = windows(y2)
    top = win.max(-1).values
    eq = win == top[..., None]
    first = eq & (eq.cumsum(-1) == 1)
    return y1 > 0, top > 0, first.to(torch.int64).argmax(-1)


def _impose(value, surrogate):
    """`value` in the forward pass, the derivative of `surrogate` in the backward pass."""
    return value.detach() + surrogate - surrogate.detach()


def regnet_f64(sd, enc1, enc2, m1, m2, R=None, gates=None, dtype=torch.float64):
    """The head on the CPU in `dtype`, training mode.  sd: the `hm_regressor.*` state dict; m1 (B, 256), m2 (B, 64): the kept elements of the two
    dropouts.  Returns a dict: hm, y1 / y2 (lists of the two images' BatchNorm outputs before the ReLUs, NCHW), the BatchNorm buffers after the step
    under their names, and with R the gradient of sum hm * R per parameter ('grad/<name>')."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(k.endswith(".weight") or k.endswith(".bias")) if v.is_floating_point() else v.clone()
         for k, v in sd.items()}
    keep = 1.0 / (1.0 - DROPOUT_P)
    res = {"y1": [], "y2": []}

    def bn(z, pfx):
        return F.batch_norm(z, p[pfx + "running_mean"], p[pfx + "running_var"], p[pfx + "weight"], p[pfx + "bias"], True, 0.1, 1e-5)

    def layer1(x, i):
        y1 = bn(F.conv2d(x, p[HM + "layer1.0.weight"], padding=1), HM + "layer1.1.")
        r1 = F.relu(y1)
        if gates is not None:
            r1 = _impose(r1, y1 * gates["relu1"][i].to(dtype))
        y2 = bn(F.conv2d(r1, p[HM + "layer1.3.weight"], padding=1), HM + "layer1.4.")
        a = F.max_pool2d(F.relu(y2), 2)
        if gates is not None:
            a = _impose(a, windows(y2).gather(-1, gates["pool"][i][..., None])[..., 0] * gates["relu2"][i].to(dtype))
        res["y1"].append(y1.detach()); res["y2"].append(y2.detach())
        return a

    with torch.enable_grad():
        a, b = layer1(enc1.to(dtype), 0), layer1(enc2.to(dtype), 1)
        N, C, H, W = a.shape
        a, b = F.normalize(a).reshape(N, C, H * W), F.normalize(b).reshape(N, C, H * W)
        v = torch.bmm(a.transpose(1, 2), b).mean(-1)                                    # the cost volume, averaged over the second image's positions
        h = F.relu(F.linear(v * m1.to(dtype) * keep, p[HM + "fc.1.weight"], p[HM + "fc.1.bias"]))
        hm = F.linear(h * m2.to(dtype) * keep, p[HM + "fc.4.weight"], p[HM + "fc.4.bias"])
        if R is not None:
            names = [k for k in p if p[k].is_floating_point() and p[k].requires_grad]
            for k, g in zip(names, torch.autograd.grad((hm * R.to(dtype)).sum(), [p[k] for k in names])):
                res["grad/" + k] = g
    res["hm"] = hm.detach()
    for k in p:
        if "running_" in k:
            res[k] = p[k].detach()
        elif k.endswith("num_batches_tracked"):
            res[k] = p[k] + 2
    return res


@functools.lru_cache(maxsize=None)
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g31_regnet_training.npz"))


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(inputs, masks, float64 results with the restatement's own decisions) of a case, computed once and shared by the tests (read-only)."""
    g = golden()
    enc1, enc2, R = case_inputs(case)
    m1, m2 = torch.from_numpy(g[f"{case}/mask1"]), torch.from_numpy(g[f"{case}/mask2"])
    return (enc1, enc2, R), (m1, m2), regnet_f64(head_state(), enc1, enc2, m1, m2, R)


def tensor_scale(res, name):
    """The scale a comparison of tensor `name` of the result dict is measured on: its largest magnitude."""
    return float(torch.as_tensor(np.asarray(res[name])).double().abs().max())


def golden_view(name, t):
    """The part of tensor `name` the golden file stores."""
    for suffix, (s0, s1) in GOLDEN_STRIDES.items():
        if name.endswith(suffix):
            return t[::s0, ::s1]
    return t
