"""Timing of the training SS2D core alone, forward + backward: the pixel-layout operator (xpoint_amd.training.ss2d_core's launches, csrc/train_ss2d.hip)
against the routes composition that training.VSSBlock runs by default (three cross-scans, the selective scan, the cross-merge, and their adjoints), at
the same inputs, on the same GPU.

    python tools/ss2d_train_bench.py [--iters 20] [--batch 16] [--size 256] [--chunks 0 ...]

Shapes: the four stages of the reference's training crop (batch 16 at 256 x 256, EMBED_DIM 96): (16, 64, 64, 96), (16, 32, 32, 192), (16, 16, 16, 384),
(16, 8, 8, 768).  Method (tools/train_bench_common.py): the two sides alternate in one process — routes, pixel, routes, pixel — device events after a
warm-up of 3, --iters iterations each; `spread` is (max - min) / min over a side's two rounds.  --chunks: the pixel form's chunk argument, one
measurement per value (0: the library's choice).  `GBps`: the ALGORITHMIC bytes of the core — u, dtp and the B / C pairs read and ym written in the
forward; u, dtp, B / C and dym read, du, ddtp and dbc written in the backward — over the best time; the same numerator for both sides.
`max_diff_over_scale`: the largest difference between the two sides' ym and six gradients, each over the routes side's scale.  Then each side's
per-kernel split from the library's event profiler (one profiled iteration).  One JSON line per shape and chunk; nothing is asserted."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xpoint_amd import _lib  # noqa: E402
from xpoint_amd.training import ops, vss  # noqa: E402
from train_bench_common import kernel_split, measure  # noqa: E402


def inputs(shape):
    B, H, W, C = shape
    M, R = B * H * W, (C + 15) // 16
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(s, device="cuda", generator=g) * 2.0 - 1.0          # noqa: E731
    return {"u": rnd(M, C), "dtp": rnd(M, 4 * C) * 2.0, "xd": rnd(M, 4 * (R + 2)), "A": -torch.exp(rnd(4 * C, 1)), "Ds": rnd(4 * C) * 0.5 + 1.0,
            "dt_bias": rnd(4, C) * 1.5 - 2.5, "dym": rnd(M, C)}, R


def bench(shape, iters, chunk):
    B, H, W, C = shape
    t, R = inputs(shape)
    dims = (B, H, W)
    st = _lib.current_stream(t["u"])
    out = {}

    def routes():
        ym, kept = vss._core_routes_fwd(t["u"], t["dtp"], t["xd"], R, t["A"], t["Ds"], t["dt_bias"], dims)
        out["routes"] = (ym,) + tuple(vss._core_routes_bwd(t["dym"], kept, t["A"], t["Ds"], t["dt_bias"], dims))

    def pixel():
        ym, ws = ops._ss2d_core_fwd(t["u"], t["dtp"], t["xd"], R, t["A"], t["Ds"], t["dt_bias"], dims, chunk, st)
        out["pixel"] = (ym,) + tuple(ops._ss2d_core_bwd(t["dym"], t["u"], t["dtp"], t["xd"], R, t["A"], t["Ds"], t["dt_bias"], ws, dims, chunk, st))

    M = B * H * W
    res = {"what": "training SS2D core fwd+bwd: pixel-layout operator vs routes composition", "shape": list(shape), "chunk": chunk, "iters": iters,
           "route_tensor_MiB": round(M * 4 * C * 4 / 2**20, 1), "algorithmic_MiB": round(4 * (17 * M * C + 3 * 8 * M) / 2**20, 1)}
    sides = (("routes", routes), ("pixel", pixel))
    for rep in range(2):
        for tag, fn in sides:
            ms, mib = measure(fn, iters)
            res.setdefault(f"{tag}_ms", []).append(round(ms, 4))
            res[f"{tag}_peak_MiB"] = round(mib, 1)
            res[f"{tag}_host_issue_ms"] = round(measure.host_ms, 4)
    for tag, _ in sides:
        best = min(res[f"{tag}_ms"])
        res[f"{tag}_spread"] = round((max(res[f"{tag}_ms"]) - best) / best, 3)
        res[f"{tag}_GBps"] = round(4 * (17 * M * C + 3 * 8 * M) / (best * 1e-3) / 1e9, 1)
    res["ratio_pixel_over_routes"] = round(min(res["pixel_ms"]) / min(res["routes_ms"]), 3)
    names = ("ym", "du", "ddtp", "dbc", "dA", "dD", "ddt_bias")
    res["max_diff_over_scale"] = {n: float((a.reshape(-1) - b.reshape(-1)).abs().max() / b.abs().max().clamp(min=1e-30))
                                  for n, a, b in zip(names, out["pixel"], out["routes"])}
    res["pixel_kernel_split"] = kernel_split(pixel)
    res["routes_kernel_split"] = kernel_split(routes)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--chunks", type=int, nargs="+", default=[0])
    ap.add_argument("--stages", type=int, nargs="+", default=[0, 1, 2, 3])
    args = ap.parse_args()
    for s in args.stages:
        side, C = args.size // (4 * 2 ** s), 96 * 2 ** s
        for chunk in args.chunks:
            if chunk == 0 or int(_lib.load().xp_ss2d_train_workspace_bytes(args.batch, side, side, C, chunk)):
                bench((args.batch, side, side, C), args.iters, chunk)


if __name__ == "__main__":
    main()
