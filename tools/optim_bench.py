"""Timing of the optimiser step of xpoint_amd.training.Adam (csrc/optim.hip) against torch.optim.Adam in its default (foreach) form and with
fused=True, on the parameter set of the VMamba XPoint with EMBED_DIM 96, DEPTHS [2, 2, 2, 2] and the homography head, f32, on the same GPU.

    python tools/optim_bench.py [--iters 50] [--batch 8] [--size 256] [--only step|train|rate]

(a) step: optimizer.step() alone on fixed gradients.  `device_ms`: device events around --iters steps that were enqueued BEHIND a spinning kernel, so
    the queue is full when the first one starts and the host's issue time is not in the window; `host_issue_ms`: the host clock around the same
    calls, nothing synchronised inside; `wall_ms`: events around back-to-back steps on an idle queue (the larger of the two, as a training loop
    sees it).  The three optimisers alternate, three rounds; `spread` is (max - min) / min of a side's device_ms.
(b) train: one training.train_step (both spectra forward and backward, XPointLoss with the regression term, the optimiser) with each of the three,
    tools/train_bench_common.py's method.
(c) rate: the apply launches' bytes / s (7 x 4 bytes per parameter element over the library's event-profiler time of `optim_adam_apply`) and the
    norm launches' (4 bytes per element, `optim_grad_sumsq`) next to the device's copy rate, measured here the way tools/hbm_copy_rate.py does
    (y.copy_(x) of 118 MB, read + write).
One JSON line per measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests.training_cases import AUG_CFG_HM, LOSS_CFG_HM  # noqa: E402
from xpoint_amd import augmentation, losses, models, synth, training  # noqa: E402
from train_bench_common import kernel_split, measure  # noqa: E402

OPTIMISERS = (("hip", lambda p: training.Adam(p, lr=1e-5, weight_decay=5e-4)),
              ("torch_foreach", lambda p: torch.optim.Adam(p, lr=1e-5, weight_decay=5e-4)),
              ("torch_fused", lambda p: torch.optim.Adam(p, lr=1e-5, weight_decay=5e-4, fused=True)))


def build_model(size):
    cfg = synth.xpoint_exp1_config(size, size, hm_head=True, vssm={"DEPTHS": [2, 2, 2, 2]})
    cfg["mixed_precision"] = False
    cfg["use_attention"]["model_parameters"]["MODEL"]["DROP_PATH_RATE"] = 0.0
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    return training.XPointNet.from_model(net).cuda().train()


def behind_a_spin(step, iters, spin_cycles):
    """device ms per step with the host's issue time out of the window, and the host's ms to issue one step"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(spin_cycles)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    host_ms = (time.perf_counter() - t0) * 1e3
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, host_ms / iters, host_ms


def bench_step(size, iters):
    model = build_model(size)
    params = list(model.parameters())
    g = torch.Generator(device="cuda").manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-3
    n = sum(p.numel() for p in params)
    res = {"what": "optimizer.step() alone", "tensors": len(params), "parameters": n, "iters": iters}
    opts = [(tag, make(params)) for tag, make in OPTIMISERS]
    for _, opt in opts:
        for _ in range(3):
            opt.step()
    for rep in range(3):
        for tag, opt in opts:
            _, host_ms, _ = behind_a_spin(opt.step, iters, 1000)                        # the host's pace first: it sizes the spin
            spin = int(2.0e6 * max(2.0 * host_ms * iters, 5.0))                         # ~2 GHz: twice the time the host needs to issue the window
            dev_ms, host_ms, total_host = behind_a_spin(opt.step, iters, spin)
            wall_ms, _ = measure(opt.step, iters)
            res.setdefault(f"{tag}_device_ms", []).append(round(dev_ms, 4))
            res.setdefault(f"{tag}_host_issue_ms", []).append(round(host_ms, 4))
            res.setdefault(f"{tag}_wall_ms", []).append(round(wall_ms, 4))
    for tag, _ in opts:
        d = res[f"{tag}_device_ms"]
        res[f"{tag}_spread"] = round((max(d) - min(d)) / min(d), 3)
    for tag in ("torch_foreach", "torch_fused"):
        res[f"device_ratio_hip_over_{tag}"] = round(min(res["hip_device_ms"]) / min(res[f"{tag}_device_ms"]), 3)
        res[f"host_ratio_hip_over_{tag}"] = round(min(res["hip_host_issue_ms"]) / min(res[f"{tag}_host_issue_ms"]), 3)
    print(json.dumps(res), flush=True)
    return params, opts[0][1]


def bench_rate(params, opt, iters):
    n = sum(p.numel() for p in params)
    split = kernel_split(opt.step)
    res = {"what": "bytes / s of the optimiser launches (library event profiler, one step) against the device copy rate", "parameters": n,
           "kernel_split_us": split}
    apply_s, norm_s = split["optim_adam_apply"]["us"] * 1e-6, split["optim_grad_sumsq"]["us"] * 1e-6
    res["apply_TBps"] = round(28.0 * n / apply_s / 1e12, 3)
    res["norm_TBps"] = round(4.0 * n / norm_s / 1e12, 3)
    x = torch.randn(29491200, device="cuda"); y = torch.empty_like(x)
    for _ in range(5):
        y.copy_(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        y.copy_(x)
    e1.record(); torch.cuda.synchronize()
    res["copy_118MB_TBps"] = round(2 * x.numel() * 4 / (e0.elapsed_time(e1) / 50 * 1e-3) / 1e12, 3)
    # the same traffic as one apply pass, as torch copies: the rate a streaming kernel of this SIZE can reach (the parameter set is far smaller than 118 MB)
    a = torch.randn(7 * n // 2, device="cuda"); b = torch.empty_like(a)
    for _ in range(5):
        b.copy_(a)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        b.copy_(a)
    e1.record(); torch.cuda.synchronize()
    res["copy_same_bytes_TBps"] = round(2 * a.numel() * 4 / (e0.elapsed_time(e1) / iters * 1e-3) / 1e12, 3)
    res["apply_over_copy_118MB"] = round(res["apply_TBps"] / res["copy_118MB_TBps"], 3)
    res["apply_over_copy_same_bytes"] = round(res["apply_TBps"] / res["copy_same_bytes_TBps"], 3)
    print(json.dumps(res), flush=True)


def bench_train(batch, size, iters):
    import random
    rng = np.random.default_rng(0)
    raw = synth.to_torch(synth.make_pair_batch(0, batch, size, size), "cuda")
    for k, flag in (('optical', True), ('thermal', False)):
        raw[k] = {'image': raw[k]['image'].float().contiguous(), 'valid_mask': torch.ones((batch, 1, size, size), dtype=torch.bool, device="cuda"),
                  'is_optical': torch.full((batch, 1), flag, device="cuda"), 'keypoints': torch.from_numpy(rng.random((batch, size, size)) < 0.02).cuda()}
    np.random.seed(5); random.seed(5)
    data = augmentation.augment_pair_batch({'optical': raw['optical'], 'thermal': raw['thermal']}, AUG_CFG_HM, np.random.default_rng(1), seed=7)
    loss_fn = losses.XPointLoss(LOSS_CFG_HM)
    res = {"what": "XPoint train_step (2 spectra fwd+bwd, loss, optimiser) by optimiser", "images": [2, batch, 1, size, size], "iters": iters}
    sides = []
    for tag, make in OPTIMISERS:
        model = build_model(size)
        opt = make(model.parameters())

        def step(model=model, opt=opt):
            torch.manual_seed(3)
            training.train_step(model, data, loss_fn, opt)
        sides.append((tag, step))
    for rep in range(4):
        for tag, step in sides:
            ms, _ = measure(step, iters)
            res.setdefault(f"{tag}_step_ms", []).append(round(ms, 3))
            res.setdefault(f"{tag}_host_issue_ms", []).append(round(measure.host_ms, 3))
    for tag, _ in sides:
        t = res[f"{tag}_step_ms"]
        res[f"{tag}_spread"] = round((max(t) - min(t)) / min(t), 3)
    for tag in ("torch_foreach", "torch_fused"):
        res[f"ratio_hip_over_{tag}"] = round(min(res["hip_step_ms"]) / min(res[f"{tag}_step_ms"]), 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--only", choices=("step", "train", "rate"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_bench.py measures on the GPU; there is no CPU path")
    if args.only in (None, "step", "rate"):
        params, opt = bench_step(args.size, args.iters if args.only != "rate" else 3)
        if args.only != "step":
            bench_rate(params, opt, args.iters)
    if args.only in (None, "train"):
        bench_train(args.batch, args.size, max(args.iters // 5, 3))


if __name__ == "__main__":
    main()
