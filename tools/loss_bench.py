"""Timing and peak memory of the fused dense descriptor loss (xp_descriptor_loss_fwd / _bwd) against an eager torch restatement of the
reference's formulation (losses.py:688-755, written here: the whole pair tensor, autograd) on the same GPU.

    python tools/loss_bench.py [--iters 20] [--shapes a,b] [--no-eager-b]

Shapes: (a) the 256x256 training crop of configs/cmt.yaml, batch 16 (1 024 cells); (b) 480x640, batch 8 (4 800 cells).  D = 256, f32,
unit-norm descriptors, identity geometry, threshold 8.  Per shape, from device events after a warm-up, fused and eager alternating in the
same call: forward and forward + backward time, torch.cuda.max_memory_allocated beyond the inputs, and the achieved matrix rate of the
fused kernels (operations from the shapes: the Gram tile is three fp16 products of 2 HW^2 K each and is evaluated once in the forward and
once per gradient sweep; a sweep's gradient product is two more) over the device-event time.  If the eager side does not fit in memory
that is reported instead of a time.  One JSON line per shape."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xpoint_amd import losses  # noqa: E402

SHAPES = {"a": ("256x256 batch 16", 16, 256, 32, 32), "b": ("480x640 batch 8", 8, 256, 60, 80)}


def eager_loss(d1, d2, thr=8.0, mp=1.0, mn=0.2, lam=250.0):
    B, D, Hc, Wc = d1.shape
    c = torch.stack(torch.meshgrid(torch.arange(Hc), torch.arange(Wc), indexing="ij"), dim=-1) * 8.0 + 4.0
    c = c.unsqueeze(0).expand(B, -1, -1, -1).clone().to(d1.device)
    dist = (c.unsqueeze(1).unsqueeze(1) - c.unsqueeze(-2).unsqueeze(-2)).norm(dim=-1)
    s = (dist <= thr).float()
    dot = torch.matmul(d2.view(B, D, -1).permute(0, 2, 1), d1.view(B, D, -1)).view(B, Hc, Wc, Hc, Wc)
    zero = torch.zeros(1, device=d1.device)
    pos = lam * s * torch.max(zero, mp - dot)
    neg = (1 - s) * torch.max(zero, dot - mn)
    del dot
    loss = pos + neg
    v = torch.matmul(torch.ones(B, Hc * Wc, 1, device=d1.device), torch.ones(B, 1, Hc * Wc, device=d1.device)).view(B, Hc, Wc, Hc, Wc)
    loss = loss * v
    norm = v.sum(-1).sum(-1).sum(-1).sum(-1)
    return (loss.sum(-1).sum(-1).sum(-1).sum(-1) / norm).mean()


def measure(fn, d1, d2, iters, backward):
    def step():
        d1.grad = d2.grad = None
        out = fn(d1, d2)
        if backward:
            out.backward()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--no-eager-b", action="store_true")
    args = ap.parse_args()
    crit = losses.XPointLoss({"detector_handle_multiple_keypoints": "hard_assignment"})
    fused = lambda a, b: crit.descriptor_loss(a, b, None, None, None, None)[0]          # noqa: E731
    for key in args.shapes.split(","):
        label, B, D, Hc, Wc = SHAPES[key]
        g = torch.Generator(device="cuda").manual_seed(0)
        d1 = torch.nn.functional.normalize(torch.randn(B, D, Hc, Wc, device="cuda", generator=g), dim=1).requires_grad_(True)
        d2 = torch.nn.functional.normalize(d1.detach() + 0.6 * torch.randn(B, D, Hc, Wc, device="cuda", generator=g), dim=1).requires_grad_(True)
        HW = Hc * Wc
        gram = 3 * 2.0 * B * HW * HW * D
        res = {"shape": label, "B": B, "D": D, "Hc": Hc, "Wc": Wc, "pair_tensor_MiB": B * HW * HW * 4 / 2**20}
        for backward in (False, True):
            tag = "fwd_bwd" if backward else "fwd"
            ms, mib = measure(fused, d1, d2, args.iters, backward)
            res[f"fused_{tag}_ms"], res[f"fused_{tag}_peak_MiB"] = round(ms, 4), round(mib, 1)
            flops = gram * (3 if backward else 1) + (2 * 2 * 2.0 * B * HW * HW * D if backward else 0)
            res[f"fused_{tag}_matrix_TFLOPs"] = round(flops / ms / 1e9, 1)
            if key == "b" and args.no_eager_b:
                continue
            try:
                ms, mib = measure(eager_loss, d1, d2, args.iters, backward)
                res[f"eager_{tag}_ms"], res[f"eager_{tag}_peak_MiB"] = round(ms, 4), round(mib, 1)
            except torch.cuda.OutOfMemoryError:
                res[f"eager_{tag}_ms"] = "out of memory"
                torch.cuda.empty_cache()
        with torch.no_grad():
            res["loss_fused"], res["loss_eager"] = float(fused(d1, d2)), (float(eager_loss(d1, d2)) if key == "a" else None)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
