"""Timing and peak memory of the heads' training step on the HIP library (xpoint_amd.training.XPointHeads, forward + backward) against torch
eager autograd of the same heads written with torch.nn here, f32, on the same GPU.

    python tools/head_train_bench.py [--iters 20] [--batch 16] [--size 256] [--no-step]

Shape: the training crop of the reference's configs/cmt.yaml — 256x256, batch 16: 16 384 rows of Ci = 48 per spectrum.  The two sides alternate
in the same call; device events after a warm-up, `--iters` iterations each (the method of tools/loss_bench.py), and next to each the time the
host needs to issue an iteration.  Then the HIP side's per-kernel
split from the library's event profiler (one profiled iteration), and one `finetune_step` at that shape (synthetic weights, Adam) as a time per step
with the frozen encoder's share.  One JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xpoint_amd import _lib, losses, models, synth, training  # noqa: E402


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


def measure(step, iters):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    host_ms = (time.perf_counter() - t0) * 1e3 / iters          # time the host needs to ISSUE an iteration (no synchronisation inside)
    e1.record()
    torch.cuda.synchronize()
    measure.host_ms = host_ms
    return e0.elapsed_time(e1) / iters, (torch.cuda.max_memory_allocated() - base) / 2**20


def kernel_split(step):
    lib = _lib.load()
    lib.xp_prof_reset(); lib.xp_prof_filter(None); lib.xp_prof_enable(1)
    step(); torch.cuda.synchronize()
    lib.xp_prof_enable(0)
    name = ctypes.create_string_buffer(96); ms = ctypes.c_double(); cnt = ctypes.c_int(); fl = ctypes.c_double(); by = ctypes.c_double()
    rows = {}
    for i in range(lib.xp_prof_count()):
        lib.xp_prof_get(i, name, 96, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by))
        rows[name.value.decode()] = {"us": round(ms.value * 1e3, 1), "launches": cnt.value}
    return dict(sorted(rows.items(), key=lambda kv: -kv[1]["us"]))


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
    for rep in range(2):                                     # alternate: hip, eager, hip, eager
        for tag, st in (("hip", step_hip), ("eager", step_eager)):
            ms, mib = measure(st, args.iters)
            res.setdefault(f"{tag}_fwd_bwd_ms", []).append(round(ms, 4))
            res[f"{tag}_peak_MiB"] = round(mib, 1)
            res[f"{tag}_host_issue_ms"] = round(measure.host_ms, 4)
    res["ratio_hip_over_eager"] = round(min(res["hip_fwd_bwd_ms"]) / min(res["eager_fwd_bwd_ms"]), 3)
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
