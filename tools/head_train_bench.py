"""Timing and peak memory of the heads' training step on the HIP library (xpoint_amd.training.XPointHeads, forward + backward) against torch
eager autograd of the same heads written with torch.nn here, f32, on the same GPU.

    python tools/head_train_bench.py [--iters 20] [--batch 16] [--size 256] [--no-step]

Shape: the training crop of the reference's configs/cmt.yaml — 256x256, batch 16: 16 384 rows of Ci = 48 per spectrum.  The method is
tools/train_bench_common.py's; then one `finetune_step` at that shape (synthetic weights, Adam) as a time per step
with the frozen encoder's share.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xpoint_amd import losses, models, synth, training  # noqa: E402
from train_bench_common import alternate, kernel_split, measure  # noqa: E402


class EagerHeads(torch.nn.Module):
    def __init__(self, ci=48, ch=256, d=256):
        super().__init__()
        nn = torch.nn

        def head(co):
            return nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(ci, ch, 3), nn.ReLU(inplace=True), nn.BatchNorm2d(ch), nn.Conv2d(ch, co, 1), nn.BatchNorm2d(co))
        self.detector_head_convolutions, self.descriptor_head_convolutions = head(65), head(d)

    def forward(self, x_nchw):
        return {'logits': self.detector_head_convolutions(x_nchw),
                'desc': torch.nn.functional.normalize(self.descriptor_head_convolutions(x_nchw), p=2, dim=1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    B, Hc = args.batch, args.size // 8
    torch.manual_seed(0)                                     # the eager heads' initialisation: the same weights in every run
    g = torch.Generator(device="cuda").manual_seed(0)
    enc = torch.randn(B, Hc, Hc, 48, device="cuda", generator=g)
    r1 = torch.randn(B, 65, Hc, Hc, device="cuda", generator=g) * 1e-3
    r2 = torch.randn(B, 256, Hc, Hc, device="cuda", generator=g) * 1e-3
    eager = EagerHeads().cuda().train()
    hip = training.XPointHeads().cuda().train()
    hip.load_state_dict(eager.state_dict())
    enc_nchw = enc.permute(0, 3, 1, 2).contiguous()

    def run(mod, x):
        def step():
            for p in mod.parameters():
                p.grad = None
            out = mod(x)
            ((out['logits'] * r1).sum() + (out['desc'] * r2).sum()).backward()
        return step
    step_hip, step_eager = run(hip, enc), run(eager, enc_nchw)
    res = {"shape": f"{args.size}x{args.size} batch {B}", "rows": B * Hc * Hc, "iters": args.iters}
    alternate(res, step_hip, step_eager, args.iters)
    # a sanity figure, not a parity check (tests/test_gpu_head_training.py is): eager f32 is the other side, and with 8.4 million trunk outputs a
    # pre-activation within rounding of 0 is likely — where the two sides disagree on its sign a bias gradient moves by one term of its sum (~1e-2 of
    # its scale at 16 384 rows).  3.bias / 4.bias gradients are zero in exact arithmetic (the BatchNorm behind the 1x1 layer removes a per-channel constant): left out of this figure
    worst = max(float((a.grad - b.grad).abs().max() / b.grad.abs().max().clamp(min=1e-30))
                for (k, a), b in zip(hip.named_parameters(), eager.parameters()) if not (k.endswith("3.bias") or k.endswith("4.bias")))
    res["max_grad_diff_vs_eager_over_scale"] = worst
    res["hip_kernel_split"] = kernel_split(step_hip)
    if not args.no_step:
        H = W = args.size
        cfg = synth.xpoint_exp1_config(H, W)
        net = models.XPoint(cfg)
        net.load_state_dict(synth.make_torch_state_dict(cfg), strict=True)
        net.to("cuda").eval()
        rng = np.random.default_rng(0)
        data = {}
        for k, flag in (('optical', True), ('thermal', False)):
            data[k] = {'image': torch.from_numpy(rng.random((B, 1, H, W), dtype=np.float32)).cuda(),
                       'valid_mask': torch.ones((B, 1, H, W), dtype=torch.bool, device="cuda"), 'is_optical': torch.full((B, 1), flag, device="cuda"),
                       'keypoints': torch.from_numpy(rng.random((B, H, W)) < 0.01).cuda(), 'homography': torch.eye(3, device="cuda").repeat(B, 1, 1)}
        heads = training.XPointHeads.from_model(net).cuda().train()
        loss_fn = losses.XPointLoss({'detector_handle_multiple_keypoints': 'hard_assignment', 'detector_loss_function': 'cross_entropy',
                                     'homography_regression_loss': {'check': False, 'gamma': 1.0}})
        opt = torch.optim.Adam(heads.parameters(), lr=1e-4)
        flags = [True] * B + [False] * B if net.config['multispectral'] else None
        images = torch.cat([data['optical']['image'], data['thermal']['image']], 0)
        ms_step, mib = measure(lambda: training.finetune_step(net, heads, data, loss_fn, opt), max(3, args.iters // 4))
        with torch.no_grad():
            ms_enc, _ = measure(lambda: net.forward_raw(images, want_prob=False, want_desc=False, is_optical=flags), max(3, args.iters // 4))
        res["finetune_step_ms"], res["finetune_step_peak_MiB"] = round(ms_step, 3), round(mib, 1)
        res["encoder_forward_ms"], res["encoder_share"] = round(ms_enc, 3), round(ms_enc / ms_step, 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
