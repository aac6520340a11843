"""Timing and peak memory of the whole VMamba encoder's training step on the HIP library (xpoint_amd.training.VSSEncoder, forward + backward of every
`encoder.*` parameter) against torch eager autograd of the same encoder, f32, on the same GPU; and the stride-2 input gradient against the stride-1
one on a zero-stuffed dy.

    python tools/encoder_train_bench.py [--iters 10] [--batch 16] [--size 256]

Encoder: the real configuration (synth.xpoint_exp1_config: EMBED_DIM 96, its DEPTHS) on a 256 x 256 crop, batch 16, stochastic depth off on both
sides.  The eager side is VSSM.forward written with torch here: F.conv2d / F.layer_norm / F.gelu for the strided layers, tools/vss_train_bench.py's
eager block (its selective scan and cross scan / merge bound to xpoint_amd.kernels, the only way the reference trains on ROCm) for the blocks.  Both
sides hold the same weights, so the two results are compared as a sanity figure.  The method is tools/train_bench_common.py's.

Input gradient: conv3x3_s2_dgrad at the three downsampler shapes against conv3x3_dgrad (the stride-1 zero-padded input gradient) on a dy that was
zero-stuffed to the input grid beforehand — the stuffing itself is not timed, which favours the stride-1 side; a call takes about 0.1 ms, so this part
runs 20 x --iters iterations.  One JSON line per measurement; nothing is asserted."""
import argparse
import copy
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xpoint_amd import synth, training  # noqa: E402
from train_bench_common import alternate, kernel_split, measure  # noqa: E402
from vss_train_bench import eager_forward  # noqa: E402


class _BlockView:
    """What vss_train_bench.eager_forward reads of a VSSBlock: t(leaf) and dt_rank, over the encoder's parameters."""

    def __init__(self, enc, s, j):
        self.enc, self.pre = enc, f"layers.{s}.blocks.{j}."
        self.dt_rank = enc.t(self.pre + "op.dt_projs_weight").shape[2]

    def t(self, leaf):
        return self.enc.t(self.pre + leaf)


def eager_encoder(enc, images):
    t = enc.t
    ln = lambda x, p: F.layer_norm(x, (x.shape[-1],), t(p + ".weight"), t(p + ".bias"), 1e-5)          # noqa: E731
    conv = lambda x, p: F.conv2d(x, t(p + ".weight"), t(p + ".bias"), stride=2, padding=1).permute(0, 2, 3, 1)          # noqa: E731
    x = F.gelu(ln(conv(torch.cat((images, images, images), 1), "patch_embed.0"), "patch_embed.2"))
    x = ln(conv(x.permute(0, 3, 1, 2), "patch_embed.5"), "patch_embed.7")
    for s, depth in enumerate(enc.depths):
        for j in range(depth):
            x = eager_forward(_BlockView(enc, s, j), x)
        if s < 3:
            x = ln(conv(x.permute(0, 3, 1, 2), f"layers.{s}.downsample.1"), f"layers.{s}.downsample.3")
    B, H, W, C = x.shape
    return x.view(B, H, W, 4, 4, C // 16).permute(0, 1, 3, 2, 4, 5).reshape(B, 4 * H, 4 * W, C // 16)


def bench_encoder(batch, size, iters):
    cfg = synth.xpoint_exp1_config(size, size)
    vssm = cfg["use_attention"]["model_parameters"]["MODEL"]["VSSM"]
    torch.manual_seed(0)
    hip = training.VSSEncoder(int(vssm["EMBED_DIM"]), list(vssm["DEPTHS"]), float(vssm.get("MLP_RATIO", 4.0)))
    sd = synth.make_torch_state_dict(cfg)
    hip.load_state_dict({k: sd[k] for k in hip.state_dict()})
    hip = hip.cuda().train()
    eager = copy.deepcopy(hip)
    g = torch.Generator(device="cuda").manual_seed(0)
    images = torch.rand((batch, 1, size, size), device="cuda", generator=g)
    R = torch.randn((batch, size // 8, size // 8, hip.embed_dim // 2), device="cuda", generator=g)

    def run(mod, forward):
        def step():
            for p in mod.parameters():
                p.grad = None
            (forward(images) * R).sum().backward()
        return step
    step_hip, step_eager = run(hip, hip), run(eager, lambda im: eager_encoder(eager, im))
    res = {"what": "encoder fwd+bwd", "embed_dim": hip.embed_dim, "depths": hip.depths, "images": [batch, 1, size, size], "iters": iters}
    alternate(res, step_hip, step_eager, iters)
    res["max_grad_diff_vs_eager_over_scale"] = max(float((a.grad - b.grad).abs().max() / b.grad.abs().max().clamp(min=1e-30))
                                                   for a, b in zip(hip.parameters(), eager.parameters()))
    split = kernel_split(step_hip)
    res["hip_kernel_ms"] = round(sum(v["us"] for v in split.values()) / 1e3, 3)
    res["hip_launches"] = sum(v["launches"] for v in split.values())
    res["hip_kernel_split_top"] = dict(list(split.items())[:12])
    print(json.dumps(res), flush=True)


def bench_dgrad(batch, size, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    for s, C in enumerate((96, 192, 384)):
        H = size // 4 >> s
        Ho, Co = H // 2, 2 * C
        dy = torch.randn((batch, Ho, Ho, Co), device="cuda", generator=g) * 1e-2
        w = torch.randn((Co, 3, 3, C), device="cuda", generator=g) * 0.05
        stuffed = torch.zeros((batch, H, H, Co), device="cuda")
        stuffed[:, ::2, ::2] = dy
        res = {"what": "conv3x3_s2_dgrad vs conv3x3_dgrad on zero-stuffed dy", "dx": [batch, H, H, C], "Co": Co, "iters": iters}
        for rep in range(2):
            for tag, st in (("s2", lambda: training.conv3x3_s2_dgrad(dy, w, (H, H))), ("stuffed_s1", lambda: training.conv3x3_dgrad(stuffed, w))):
                ms, _ = measure(st, iters)
                res.setdefault(f"{tag}_ms", []).append(round(ms, 4))
                res[f"{tag}_host_issue_ms"] = round(measure.host_ms, 4)
        res["ratio_s2_over_stuffed"] = round(min(res["s2_ms"]) / min(res["stuffed_s1_ms"]), 3)
        a, b = training.conv3x3_s2_dgrad(dy, w, (H, H)), training.conv3x3_dgrad(stuffed, w)
        res["max_diff_over_scale"] = float((a - b).abs().max() / b.abs().max())
        split = kernel_split(lambda: training.conv3x3_s2_dgrad(dy, w, (H, H)))
        res["s2_kernel_split"] = split
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--only", choices=("encoder", "dgrad"), default=None)
    args = ap.parse_args()
    if args.only != "encoder":
        bench_dgrad(args.batch, args.size, 20 * args.iters)          # a call takes ~0.1 ms: 20 x the iterations for a window of tens of ms
    if args.only != "dgrad":
        bench_encoder(args.batch, args.size, args.iters)


if __name__ == "__main__":
    main()
