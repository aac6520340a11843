"""Timing and peak memory of the homography head's training step on the HIP library (xpoint_amd.training.RegNetHead, forward + backward) against
torch eager autograd of the same head written with torch.nn here, f32, on the same GPU.

    python tools/regnet_train_bench.py [--iters 20] [--batch 16]

Shape: the only map size the head accepts — 32 x 32 x 48 per spectrum (a 256 x 256 crop), batch 16.  Both sides apply the SAME dropout masks (the eager
side multiplies by them), so the two results can be compared as a sanity figure.  The method is tools/train_bench_common.py's.  One JSON line; nothing is
asserted."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xpoint_amd import training  # noqa: E402
from train_bench_common import alternate, kernel_split  # noqa: E402


class EagerRegNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        nn = torch.nn
        hm = nn.Module()
        hm.layer1 = nn.Sequential(nn.Conv2d(48, 96, 3, padding=1, bias=False), nn.BatchNorm2d(96), nn.ReLU(inplace=True),
                                  nn.Conv2d(96, 192, 3, padding=1, bias=False), nn.BatchNorm2d(192), nn.ReLU(inplace=True), nn.MaxPool2d(2))
        hm.fc = nn.Sequential(nn.Dropout(0.5), nn.Linear(256, 64), nn.ReLU(True), nn.Dropout(0.5), nn.Linear(64, 8))
        self.hm_regressor = hm

    def forward(self, x1, x2, m1, m2):
        hm = self.hm_regressor
        a, b = hm.layer1(x1), hm.layer1(x2)
        N, C, H, W = a.shape
        a, b = F.normalize(a).reshape(N, C, H * W), F.normalize(b).reshape(N, C, H * W)
        v = torch.bmm(a.transpose(1, 2), b).mean(-1)           # the cost volume and its global average pool, as RegNet.forward forms them
        h = F.relu(hm.fc[1](v * m1 * 2.0))
        return hm.fc[4](h * m2 * 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    B, Hc = args.batch, 32
    torch.manual_seed(0)                                     # the eager head's initialisation: the same weights in every run
    g = torch.Generator(device="cuda").manual_seed(0)
    enc1, enc2 = (torch.randn(B, Hc, Hc, 48, device="cuda", generator=g) for _ in range(2))
    R = torch.randn(B, 8, device="cuda", generator=g)
    m1 = (torch.rand(B, 256, device="cuda", generator=g) >= 0.5).to(torch.uint8)
    m2 = (torch.rand(B, 64, device="cuda", generator=g) >= 0.5).to(torch.uint8)
    eager = EagerRegNet().cuda().train()
    hip = training.RegNetHead().cuda().train()
    hip.load_state_dict(eager.state_dict())
    x1, x2 = (e.permute(0, 3, 1, 2).contiguous() for e in (enc1, enc2))
    f1, f2 = m1.float(), m2.float()

    def run(mod, forward):
        def step():
            for p in mod.parameters():
                p.grad = None
            (forward() * R).sum().backward()
        return step
    step_hip = run(hip, lambda: hip(enc1, enc2, dropout_masks=(m1, m2)))
    step_eager = run(eager, lambda: eager(x1, x2, f1, f2))
    res = {"shape": f"32x32x48 maps, batch {B}", "rows_per_image": B * Hc * Hc, "iters": args.iters}
    alternate(res, step_hip, step_eager, args.iters)
    # a sanity figure, not a parity check (tests/test_gpu_regnet_training.py is): eager f32 is the other side, and among 5 million ReLU / max-pool
    # decisions some fall within rounding of the jump and go different ways on the two sides
    res["max_grad_diff_vs_eager_over_scale"] = max(float((a.grad - b.grad).abs().max() / b.grad.abs().max().clamp(min=1e-30))
                                                   for a, b in zip(hip.parameters(), eager.parameters()))
    res["hip_kernel_split"] = kernel_split(step_hip)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
