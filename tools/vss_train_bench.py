"""Timing and peak memory of one VSS block's training step on the HIP library (xpoint_amd.training.VSSBlock, forward + backward with the input gradient)
against torch eager autograd of the same block, f32, on the same GPU.

    python tools/vss_train_bench.py [--iters 20] [--batch 16] [--core routes|pixel|both] [--stages 0 3]

Shapes: the reference's training crop (256 x 256, batch 16) at the first and the last encoder stage — (16, 64, 64, 96) and (16, 8, 8, 768).  The eager
side is the reference's forward_corev2 written with torch here, its selective scan and cross scan / merge bound to xpoint_amd.kernels (the only way the
reference trains on ROCm); everything else — LayerNorm, the linear layers, the depthwise convolution, the einsums, GELU — is
torch.  Both sides hold the same weights, so the two results are compared as a sanity figure.  The method is
tools/train_bench_common.py's.  --core: the form of the HIP block's SS2D core (training.set_ss2d_core; default routes); `both`: the block under
"pixel" against the block under "routes" instead of against eager, alternating in the same call, with each side's spread over its two rounds.
--stages: which of the four training shapes, (16, 64, 64, 96) ... (16, 8, 8, 768).  One JSON line per shape; nothing is asserted."""
import argparse
import copy
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xpoint_amd import training  # noqa: E402
from train_bench_common import alternate, kernel_split  # noqa: E402
from xpoint_amd.kernels import cross_merge_fn, cross_scan_fn, selective_scan_fn  # noqa: E402


def eager_forward(blk, x):
    """VMamba.py:1222-1234 with forwardv2 / forward_corev2 (v05_noz, d_state 1) on the parameters of `blk`; x (B, H, W, C)"""
    t = blk.t
    B, H, W, C = x.shape
    L = H * W
    R = blk.dt_rank
    y = F.layer_norm(x, (C,), t("norm.weight"), t("norm.bias"), 1e-5)
    y = F.silu(F.conv2d(F.linear(y, t("op.in_proj.weight")).permute(0, 3, 1, 2).contiguous(), t("op.conv2d.weight"), padding=1, groups=C))
    xs = cross_scan_fn(y, in_channel_first=True, out_channel_first=True, scans=0)
    x_dbl = torch.einsum("b k d l, k c d -> b k c l", xs, t("op.x_proj_weight"))
    dts, Bs, Cs = torch.split(x_dbl, [R, 1, 1], dim=2)
    dts = torch.einsum("b k r l, k d r -> b k d l", dts, t("op.dt_projs_weight"))
    ys = selective_scan_fn(xs.view(B, -1, L), dts.contiguous().view(B, -1, L), -t("op.A_logs").float().exp(), Bs.contiguous(), Cs.contiguous(),
                           t("op.Ds").float(), t("op.dt_projs_bias").view(-1).float(), True)
    y = cross_merge_fn(ys.view(B, 4, C, H, W), in_channel_first=True, out_channel_first=True, scans=0)
    y = y.view(B, C, L).transpose(1, 2).contiguous().view(B, H, W, C)
    y = F.layer_norm(y, (C,), t("op.out_norm.weight"), t("op.out_norm.bias"), 1e-5)
    x = x + F.linear(y, t("op.out_proj.weight"))
    y = F.layer_norm(x, (C,), t("norm2.weight"), t("norm2.bias"), 1e-5)
    return x + F.linear(F.gelu(F.linear(y, t("mlp.fc1.weight"), t("mlp.fc1.bias"))), t("mlp.fc2.weight"), t("mlp.fc2.bias"))


def bench(shape, iters, core):
    B, H, W, C = shape
    torch.manual_seed(0)                                     # the block's initialisation: the same weights in every run
    hip = training.set_ss2d_core(training.VSSBlock(C), "pixel" if core == "both" else core).cuda().train()
    eager = copy.deepcopy(hip)
    if core == "both":
        training.set_ss2d_core(eager, "routes")
    g = torch.Generator(device="cuda").manual_seed(0)
    x0 = torch.randn(shape, device="cuda", generator=g)
    R = torch.randn(shape, device="cuda", generator=g)
    grads = {}

    def run(tag, mod, forward):
        def step():
            for p in mod.parameters():
                p.grad = None
            x = x0.clone().requires_grad_(True)
            (forward(x) * R).sum().backward()
            grads[tag] = x.grad
        return step
    step_hip = run("hip", hip, hip)
    step_eager = run("eager", eager, lambda x: eager_forward(eager, x))
    res = {"shape": list(shape), "rows": B * H * W, "iters": iters, "core": core, "route_tensor_MiB": round(B * 4 * C * H * W * 4 / 2**20, 1)}
    if core == "both":
        step_routes = run("eager", eager, eager)
        alternate(res, step_hip, step_routes, iters, tags=("pixel", "routes"))
        pairs = list(zip(hip.parameters(), eager.parameters())) + [(type("G", (), {"grad": grads["hip"]}), type("G", (), {"grad": grads["eager"]}))]
        res["max_grad_diff_pixel_vs_routes_over_scale"] = max(float((a.grad - b.grad).abs().max() / b.grad.abs().max().clamp(min=1e-30)) for a, b in pairs)
        res["pixel_kernel_split"] = kernel_split(step_hip)
        res["routes_kernel_split"] = kernel_split(step_routes)
        print(json.dumps(res), flush=True)
        return
    alternate(res, step_hip, step_eager, iters)
    # a sanity figure, not a parity check (tests/test_gpu_vss_training.py is): eager f32 is the other side
    pairs = list(zip(hip.parameters(), eager.parameters())) + [(type("G", (), {"grad": grads["hip"]}), type("G", (), {"grad": grads["eager"]}))]
    res["max_grad_diff_vs_eager_over_scale"] = max(float((a.grad - b.grad).abs().max() / b.grad.abs().max().clamp(min=1e-30)) for a, b in pairs)
    res["hip_kernel_split"] = kernel_split(step_hip)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--core", choices=("routes", "pixel", "both"), default="routes")
    ap.add_argument("--stages", type=int, nargs="+", default=[0, 3])
    args = ap.parse_args()
    for s in args.stages:
        bench((args.batch, 64 >> s, 64 >> s, 96 << s), args.iters, args.core)


if __name__ == "__main__":
    main()
