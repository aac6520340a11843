"""Time the batched detector evaluation (xpoint_amd.evaluation.tp_fp_dist_batched) at 8 x 480 x 640 with nms 0 — every pixel above
zero_threshold is a prediction — and ~500 labels per image, against a host numpy run of the same rule on ONE image
(tests/test_cpu_detector_eval.py:tp_fp_rule, vectorised over the window: no loop over predictions).

    python tools/detector_eval_bench.py [--batch 8] [--iters 20] [--reference-loop]

--reference-loop additionally times the reference's formulation on one image on the host: the dense (predictions x labels) float32
distance matrix in row blocks and the sequential Python loop over all predictions (xpoint/utils/evaluation.py:78-93).  It takes minutes.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_cpu_detector_eval import tp_fp_rule  # noqa: E402
from xpoint_amd import synth  # noqa: E402


def make_inputs(B, H, W, n_labels=500):
    prob = synth.uniform("detector_eval_bench/prob", (B, H, W), 0.001, 1.0)
    kp = synth.uniform("detector_eval_bench/kp", (B, H, W), 0.0, 1.0) < n_labels / (H * W)
    return prob, kp


def reference_loop(prob, kp, zero_threshold=1e-4, distance_thresh=2.0):
    """The reference's formulation on the host: all-pairs distances (in row blocks, so that the matrix fits), then the greedy loop."""
    lab = np.argwhere(kp)
    cand = np.argwhere(prob > zero_threshold)
    order = np.argsort(-prob[cand[:, 0], cand[:, 1]], kind="stable")
    pred = cand[order]
    matched = np.zeros(len(lab), bool)
    tp = np.zeros(len(pred), bool)
    for i0 in range(0, len(pred), 4096):
        d = np.linalg.norm((pred[i0:i0 + 4096, None, :] - lab[None, :, :]).astype(np.float32), axis=-1)
        for j, m in enumerate(d <= distance_thresh):
            if m.any() and not matched.all():
                gi = int(np.argmax(m))
                tp[i0 + j] = not matched[gi]
                matched[gi] = True
    return tp


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reference-loop", action="store_true")
    args = ap.parse_args()
    B, H, W = args.batch, 480, 640
    prob, kp = make_inputs(B, H, W)
    out = {"shape": [B, H, W], "labels_per_image": float(kp.reshape(B, -1).sum(1).mean())}
    t0 = time.perf_counter()
    want = tp_fp_rule(prob[0], kp[0])
    out["host_numpy_one_image_ms"] = (time.perf_counter() - t0) * 1e3
    if args.reference_loop:
        t0 = time.perf_counter()
        tp_ref = reference_loop(prob[0], kp[0])
        out["host_reference_loop_one_image_s"] = time.perf_counter() - t0
        out["reference_loop_tp_equal"] = bool(tp_ref.sum() == want[0].sum())
    if torch.cuda.is_available():
        from xpoint_amd import evaluation
        p, k = torch.from_numpy(prob).cuda(), torch.from_numpy(kp).cuda()
        for _ in range(args.warmup):
            res = evaluation.tp_fp_dist_batched(p, k)
        assert np.array_equal(res[0][0].cpu().numpy(), want[0])
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            evaluation.tp_fp_dist_batched(p, k)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        times.sort()
        out["gpu_batched_ms_median"] = times[len(times) // 2]
        out["gpu_batched_ms_min"] = times[0]
        out["gpu_ms_per_image"] = out["gpu_batched_ms_median"] / B
        out["speedup_vs_host_numpy_per_image"] = out["host_numpy_one_image_ms"] / out["gpu_ms_per_image"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
