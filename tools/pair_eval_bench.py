"""Time the matching evaluation end to end: evaluation.compute_metrics (per-sample) against evaluation.compute_metrics_batched on the SAME
16 pairs at 480 x 640 — synthetic weights, prediction.nms 4, topk 1024, two batches of 8, benchmark.py's ten-threshold lists (1..10 for
repeatability, keypoint distance and warp error, [2] for RANSAC).

    python tools/pair_eval_bench.py [--pairs 16] [--batch 8] [--rounds 5] [--warmup 1] [--height 480 --width 640] [--out FILE]

The two sides alternate in one process after a warm-up; each timed call ends in a device synchronise (host clock around the whole call: the
host work IS what differs).  Reports per side the median, minimum, maximum and (max - min) / median of the rounds, the speed-up of the medians
with the verdict whether it exceeds both spreads, whether the two sides agree on the repeatability and descriptor dictionaries, and — from
one extra profiled pass per side — the number of device kernel launches and of host synchronisations per batch (torch's sync debug mode: the
.item() / .cpu() / nonzero() calls; the stream synchronise of the final copy counts as one).  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xpoint_amd import synth  # noqa: E402

THS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]


def _tree_equal(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_tree_equal(a[k], b[k]) for k in a)
    return bool(np.array_equal(np.asarray(a), np.asarray(b)))


def _count(fn):
    """(kernel launches, host synchronisations) of one call of fn."""
    from torch.profiler import ProfilerActivity, profile
    syncs = None
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
        syncs = sum(1 for w in caught if "synchron" in str(w.message).lower())
    except Exception as exc:
        print(f"sync debug mode unavailable: {exc!r}", file=sys.stderr)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    launches = None
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                       and "memset" not in e.name.lower())
    except Exception as exc:          # the profiler is optional: say so instead of failing the timing
        print(f"profiler unavailable: {exc!r}", file=sys.stderr)
    return launches, syncs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--topk", type=int, default=1024)
    ap.add_argument("--no-counts", action="store_true", help="skip the profiled passes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_eval_bench needs a GPU (no CPU fallback)")
    from xpoint_amd import evaluation as ev, models
    H, W = args.height, args.width
    cfg = synth.xpoint_exp1_config(H, W)
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg), strict=True)
    net = net.to("cuda").eval()
    config = {"prediction": {"nms": 4, "topk": args.topk, "cpu_nms": False,
                             "matching": {"method": "bfmatcher", "knn_matches": False, "method_kwargs": {"crossCheck": True}}}}
    n_batches = args.pairs // args.batch
    batches = [synth.to_torch(synth.make_pair_batch(i, args.batch, H, W)) for i in range(n_batches)]      # host tensors, as a data loader gives them

    def loader():
        for d in batches:
            yield {s: dict(d[s]) for s in ("optical", "thermal")}

    def run(fn):
        with torch.no_grad():
            return fn(net, loader(), "cuda", config, 0.015, list(THS), list(THS), list(THS), [2])

    sides = {"per_sample": ev.compute_metrics, "batched": ev.compute_metrics_batched}
    results, times = {}, {k: [] for k in sides}
    for _ in range(args.warmup):
        for k, fn in sides.items():
            results[k] = run(fn)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(fn)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    out = {"shape": [args.pairs, H, W], "batch": args.batch, "nms": 4, "topk": args.topk, "thresholds": len(THS), "rounds": args.rounds,
           "n_kp_avg": float(results["batched"]["repeatability"]["n_kp_avg"]),
           "same_repeatability": _tree_equal(results["batched"]["repeatability"], results["per_sample"]["repeatability"]),
           "same_descriptor": _tree_equal(results["batched"]["descriptor"], results["per_sample"]["descriptor"])}
    for k, v in times.items():
        s = sorted(v)
        med = s[len(s) // 2]
        out[k] = {"ms_median": med, "ms_min": s[0], "ms_max": s[-1], "spread": (s[-1] - s[0]) / med, "ms_per_pair": med / args.pairs}
    sp = out["per_sample"]["ms_median"] / out["batched"]["ms_median"]
    out["speedup_of_medians"] = sp
    out["speedup_exceeds_both_spreads"] = bool(abs(sp - 1.0) > max(out["per_sample"]["spread"], out["batched"]["spread"]))
    if not args.no_counts:
        for k, fn in sides.items():
            launches, syncs = _count(lambda: run(fn))
            out[k]["kernel_launches_per_batch"] = None if launches is None else launches / n_batches
            out[k]["host_syncs_per_batch"] = None if syncs is None else syncs / n_batches
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
