"""A float64 restatement of one VSS encoder block (reference xpoint/models/vmamba_src/VMamba.py:1153-1234 with the SS2D of forwardv2 /
forward_corev2: v05_noz, d_state 1, SSM_RATIO 1.0, no convolution bias), forward and backward, in plain torch on the CPU: the test side of
xpoint_amd.training.VSSBlock.  The selective scan is the restatement of tests/test_cpu_scan_grad.py (Scan64: a float64 forward loop and its analytic
backward); everything else is torch's float64 autograd.  tests/test_cpu_vss_training.py pins it against the real reference
(tests/golden/g32_vss_training.npz, tools/make_golden_vss_training.py) and by gradcheck; tests/test_gpu_vss_training.py compares the HIP block against it.

Inputs are hash uniforms (synth.uniform) the tests regenerate; weights are those of synth.make_state_dict for the reference's XPoint with
EMBED_DIM = E and DEPTHS [1, 1, 1, 1], block 0 of the stage whose width is the case's channel count."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.test_cpu_scan_grad import Scan64
from xpoint_amd import synth

# case -> ((B, H, W, C), dt_rank, EMBED_DIM, stage)
CASES = {
    "A": ((2, 5, 7, 32), 2, 32, 0),        # odd sizes, two samples, the smallest rank
    "B": ((1, 8, 12, 96), 6, 96, 0),       # the real stage-0 channel count, K = R not a multiple of 4
    "C": ((2, 2, 3, 768), 48, 96, 3),      # the real stage-3 width
    "D": ((1, 45, 46, 32), 2, 32, 0),      # L = 2070 crosses the scan's 2048-element chunk boundary
}
GOLDEN_CASES = ("A", "B")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g32_vss_training.npz")
LEAVES = ("norm.weight", "norm.bias", "op.x_proj_weight", "op.A_logs", "op.Ds", "op.dt_projs_weight", "op.dt_projs_bias", "op.out_norm.weight",
          "op.out_norm.bias", "op.in_proj.weight", "op.conv2d.weight", "op.out_proj.weight", "norm2.weight", "norm2.bias", "mlp.fc1.weight",
          "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def model_config(E):
    return synth.xpoint_exp1_config(256, 256, vssm={"EMBED_DIM": int(E), "DEPTHS": [1, 1, 1, 1]})


def prefix(case):
    return f"encoder.layers.{CASES[case][3]}.blocks.0."


@functools.lru_cache(maxsize=None)
def _state(E):
    return synth.make_state_dict(model_config(E))


def block_state(case, dtype=torch.float64):
    """{leaf: tensor} of the case's block, the reference's names without the prefix, in the reference's order."""
    sd, pre = _state(CASES[case][2]), prefix(case)
    return {k: torch.from_numpy(np.array(sd[pre + k], copy=True)).to(dtype) for k in LEAVES}


def case_inputs(case):
    """x (B, H, W, C) and the weights R of the scalar sum(out * R) that is back-propagated, float32."""
    shape = CASES[case][0]
    return (torch.from_numpy(synth.uniform(f"vss/{case}/x", shape, -1.0, 1.0)), torch.from_numpy(synth.uniform(f"vss/{case}/R", shape, -1.0, 1.0)))


def cross_scan64(x):
    """(B, C, H, W) -> (B, 4, C, L): rows, columns, and both reversed (csm_triton.py cross_scan_fn, scans 0)."""
    B, C, H, W = x.shape
    y = x.new_empty((B, 4, C, H * W))
    y[:, 0] = x.flatten(2, 3)
    y[:, 1] = x.transpose(2, 3).flatten(2, 3)
    y[:, 2:4] = torch.flip(y[:, 0:2], dims=[-1])
    return y


def cross_merge64(y, H, W):
    """(B, 4, C, L) -> (B, C, L)."""
    B, K, C, L = y.shape
    y = y[:, 0:2] + y[:, 2:4].flip(dims=[-1])
    return y[:, 0] + y[:, 1].view(B, C, W, H).transpose(2, 3).contiguous().view(B, C, L)


def vss_block64(p, x, s1=None, s2=None):
    """The block's output (B, H, W, C) from x (B, H, W, C) and p = {leaf: tensor}; s1, s2: per-sample factors (B,) of the two branches (stochastic
    depth: keep / (1 - p)) or None.  Differentiable in x and every tensor of p."""
    B, H, W, C = x.shape
    L = H * W
    R = p["op.dt_projs_weight"].shape[2]
    one = x.new_ones(B)
    s1 = one if s1 is None else s1.to(x.dtype)
    s2 = one if s2 is None else s2.to(x.dtype)
    t = F.layer_norm(x, (C,), p["norm.weight"], p["norm.bias"], 1e-5)
    t = t @ p["op.in_proj.weight"].t()
    t = F.silu(F.conv2d(t.permute(0, 3, 1, 2), p["op.conv2d.weight"], padding=1, groups=C))          # (B, C, H, W)
    xs = cross_scan64(t)
    x_dbl = torch.einsum("bkdl,kcd->bkcl", xs, p["op.x_proj_weight"])
    dts, Bs, Cs = torch.split(x_dbl, [R, 1, 1], dim=2)
    dts = torch.einsum("bkrl,kdr->bkdl", dts, p["op.dt_projs_weight"])
    ys = Scan64.apply(xs.reshape(B, 4 * C, L), dts.reshape(B, 4 * C, L), -torch.exp(p["op.A_logs"]), Bs.contiguous(), Cs.contiguous(), p["op.Ds"],
                      p["op.dt_projs_bias"].reshape(-1), True)
    y = cross_merge64(ys.view(B, 4, C, L), H, W).transpose(1, 2).reshape(B, H, W, C)
    y = F.layer_norm(y, (C,), p["op.out_norm.weight"], p["op.out_norm.bias"], 1e-5)
    x = x + s1.view(B, 1, 1, 1) * (y @ p["op.out_proj.weight"].t())
    t = F.layer_norm(x, (C,), p["norm2.weight"], p["norm2.bias"], 1e-5)
    t = F.gelu(t @ p["mlp.fc1.weight"].t() + p["mlp.fc1.bias"])
    return x + s2.view(B, 1, 1, 1) * (t @ p["mlp.fc2.weight"].t() + p["mlp.fc2.bias"])


def vss_step64(p, x, Rw, s1=None, s2=None):
    """{'out', 'grad/x', 'grad/<leaf>'} of sum(out * Rw), float64."""
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in p.items()}
    x = x.detach().double().clone().requires_grad_(True)
    out = vss_block64(p, x, s1, s2)
    grads = torch.autograd.grad((out * Rw.double()).sum(), [x] + [p[k] for k in LEAVES])
    res = {"out": out.detach(), "grad/x": grads[0]}
    res.update({"grad/" + k: g for k, g in zip(LEAVES, grads[1:])})
    return res


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """The restatement's step on the case's inputs (computed once per process; callers must not modify it)."""
    x, Rw = case_inputs(case)
    return vss_step64(block_state(case), x, Rw)


def golden():
    return np.load(GOLDEN)
