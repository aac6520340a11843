"""Timing of the whole VMamba XPoint's training step on the HIP library (xpoint_amd.training.XPointNet / train_step: both spectra through the encoder
and the heads, XPointLoss, backward into every parameter, Adam) against torch eager autograd of the same model, f32, on the same GPU; and the input
gradient of the reflection-padded 3x3 convolution against what the operators could do before it existed.

    python tools/xpoint_train_bench.py [--iters 5] [--batch 16] [--size 256] [--only kernel|step] [--core routes|pixel|both]

(a) Kernel: conv3x3_dgrad_reflect at the trunk's shapes, dy (batch, size / 8, size / 8, 512), Ci 48 (VMamba) and 128 (conv encoder), against the
composition: dy copied into a zero (H + 2) x (W + 2) frame, conv3x3_dgrad (the zero-padded input gradient) on the frame, the frame folded back with
torch.  Both take the dy_scale that xp_bn_train_bwd hands the trunk.  Three runs of each, alternating; `spread` is (max - min) / min over a side's
three runs.  A call takes well under a millisecond, so this part runs 40 x --iters iterations.
(b) Step: the real configuration (synth.xpoint_exp1_config: EMBED_DIM 96, its DEPTHS, no homography head) on --size crops, stochastic depth off on
both sides.  The eager side is tools/encoder_train_bench.py's eager encoder (its selective scan and cross scan / merge bound to xpoint_amd.kernels,
the only way the reference trains on ROCm), the heads' torch modules (ReflectionPad2d, Conv2d, ReLU, BatchNorm2d, Conv2d, BatchNorm2d, F.normalize)
and the same XPointLoss and Adam.  The method is tools/train_bench_common.py's: device events after a warm-up, the host's issue time next to them,
then the HIP side's per-kernel split from the library's event profiler.  --core: the form of the HIP model's SS2D cores (training.set_ss2d_core;
default routes); `both`: the model under "pixel" against the model under "routes" instead of against eager, alternating in the same call, with each
side's spread over its two rounds and both kernel splits.  One JSON line per measurement; nothing is asserted."""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.training_cases import AUG_CFG, LOSS_CFG  # noqa: E402
from xpoint_amd import augmentation, losses, models, synth, training  # noqa: E402
from encoder_train_bench import eager_encoder  # noqa: E402
from train_bench_common import alternate, kernel_split, measure  # noqa: E402


def composition(dy, w, scale):
    B, H, W, Co = dy.shape
    frame = torch.zeros((B, H + 2, W + 2, Co), dtype=dy.dtype, device=dy.device)
    frame[:, 1:-1, 1:-1] = dy
    g = training.conv3x3_dgrad(frame, w, dy_scale=scale)
    for axis, n in ((1, H), (2, W)):
        inner = g.narrow(axis, 1, n).clone()
        inner.narrow(axis, 1, 1).add_(g.narrow(axis, 0, 1))
        inner.narrow(axis, n - 2, 1).add_(g.narrow(axis, n + 1, 1))
        g = inner
    return g


def bench_kernel(batch, size, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    H, Co = size // 8, 512
    for Ci in (48, 128):
        dy, scale = training.scale_grad(torch.randn((batch, H, H, Co), device="cuda", generator=g) * 1e-2)
        w = torch.randn((Co, 3, 3, Ci), device="cuda", generator=g) * 0.05
        sides = (("reflect", lambda: training.conv3x3_dgrad_reflect(dy, w, dy_scale=scale)), ("composition", lambda: composition(dy, w, scale)))
        res = {"what": "conv3x3_dgrad_reflect vs zero-padded dgrad on a framed dy + torch fold", "dx": [batch, H, H, Ci], "Co": Co, "iters": iters}
        for rep in range(3):
            for tag, st in sides:
                ms, _ = measure(st, iters)
                res.setdefault(f"{tag}_ms", []).append(round(ms, 4))
                res[f"{tag}_host_issue_ms"] = round(measure.host_ms, 4)
        for tag, _ in sides:
            res[f"{tag}_spread"] = round((max(res[f"{tag}_ms"]) - min(res[f"{tag}_ms"])) / min(res[f"{tag}_ms"]), 3)
        res["ratio_reflect_over_composition"] = round(min(res["reflect_ms"]) / min(res["composition_ms"]), 3)
        a, b = sides[0][1](), sides[1][1]()
        res["max_diff_over_scale"] = float((a - b).abs().max() / b.abs().max())
        res["reflect_kernel_split"] = kernel_split(sides[0][1])
        res["composition_kernel_split"] = kernel_split(sides[1][1])          # the library's launches only: the frame copy and the fold are torch's
        print(json.dumps(res), flush=True)


def pair_batch(batch, size):
    rng = np.random.default_rng(0)
    raw = synth.to_torch(synth.make_pair_batch(0, batch, size, size), "cuda")
    for k, flag in (('optical', True), ('thermal', False)):
        raw[k] = {'image': raw[k]['image'].float().contiguous(), 'valid_mask': torch.ones((batch, 1, size, size), dtype=torch.bool, device="cuda"),
                  'is_optical': torch.full((batch, 1), flag, device="cuda"), 'keypoints': torch.from_numpy(rng.random((batch, size, size)) < 0.02).cuda()}
    return augmentation.augment_pair_batch({'optical': raw['optical'], 'thermal': raw['thermal']}, AUG_CFG, np.random.default_rng(1), seed=7)


def eager_model(model, data):
    """XPointNet.forward in training mode with torch's operators (the scan and cross ops bound to the HIP kernels)."""
    enc = model._encoders["encoder."]
    preds = []
    for sp in ("optical", "thermal"):
        x = eager_encoder(enc, data[sp]["image"]).permute(0, 3, 1, 2)
        preds.append({"logits": model.detector_head_convolutions(x), "desc": F.normalize(model.descriptor_head_convolutions(x), p=2, dim=1),
                      "encoder_output": x.detach()})
    return preds


def bench_step(batch, size, iters, core="routes"):
    cfg = synth.xpoint_exp1_config(size, size)
    cfg["mixed_precision"] = False
    cfg["use_attention"]["model_parameters"]["MODEL"]["DROP_PATH_RATE"] = 0.0
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    hip = training.set_ss2d_core(training.XPointNet.from_model(net), "pixel" if core == "both" else core).cuda().train()
    eager = training.set_ss2d_core(training.XPointNet.from_model(net), "routes").cuda().train() if core == "both" else copy.deepcopy(hip)
    data = pair_batch(batch, size)
    loss_fn = losses.XPointLoss(LOSS_CFG)
    opts = {id(m): torch.optim.Adam(m.parameters(), lr=1e-5) for m in (hip, eager)}
    last = {}

    def step_hip():
        torch.manual_seed(3)
        last["hip"], _ = training.train_step(hip, data, loss_fn, opts[id(hip)])

    def step_eager():
        torch.manual_seed(3)
        opts[id(eager)].zero_grad(set_to_none=True)
        pred, pred2 = eager_model(eager, data)
        loss, _ = loss_fn({'data': data, 'pred': pred, 'pred2': pred2})
        loss.backward()
        opts[id(eager)].step()
        last["eager"] = loss.detach()

    enc = hip._encoders["encoder."]
    res = {"what": "XPoint train_step (2 spectra fwd+bwd, loss, Adam)", "embed_dim": enc.embed_dim, "depths": enc.depths, "images": [2, batch, 1, size, size],
           "iters": iters, "core": core, "parameters": sum(p.numel() for p in hip.parameters())}
    if core == "both":
        def step_routes():
            torch.manual_seed(3)
            last["routes"], _ = training.train_step(eager, data, loss_fn, opts[id(eager)])
        alternate(res, step_hip, step_routes, iters, tags=("pixel", "routes"))
        res["last_loss"] = {"pixel": float(last["hip"]), "routes": float(last["routes"])}
        for tag, st in (("pixel", step_hip), ("routes", step_routes)):
            split = kernel_split(st)
            res[f"{tag}_kernel_ms"] = round(sum(v["us"] for v in split.values()) / 1e3, 3)
            res[f"{tag}_launches"] = sum(v["launches"] for v in split.values())
            res[f"{tag}_kernel_split_top"] = dict(list(split.items())[:14])
        print(json.dumps(res), flush=True)
        return
    alternate(res, step_hip, step_eager, iters)
    res["last_loss"] = {k: float(v) for k, v in last.items()}          # both sides took the same number of steps from the same state
    split = kernel_split(step_hip)
    res["hip_kernel_ms"] = round(sum(v["us"] for v in split.values()) / 1e3, 3)
    res["hip_launches"] = sum(v["launches"] for v in split.values())
    res["hip_kernel_split_top"] = dict(list(split.items())[:14])
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--only", choices=("kernel", "step"), default=None)
    ap.add_argument("--core", choices=("routes", "pixel", "both"), default="routes")
    args = ap.parse_args()
    if args.only != "step":
        bench_kernel(args.batch, args.size, 40 * args.iters)          # a call takes ~0.2 ms: 40 x the iterations for a window of tens of ms
    if args.only != "kernel":
        bench_step(args.batch, args.size, args.iters, args.core)


if __name__ == "__main__":
    main()
