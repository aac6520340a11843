"""Homographic adaptation at 480 x 640 (one pair, the full XPoint-EXP1 model with synthetic weights, export_keypoints config: window
aggregation, window 5, erosion 3, mask_border, min_count 5): ms per pair for num = 10 and 100, with the default chunk and with chunk = 1
(one homography per forward: the reference's loop shape); the HIP-event split forwards vs the HA kernels; achieved bytes/s of the warp
(a) and the fused accumulate (c) against the measured 6.29 TB/s copy rate.  Prints one JSON line.

    python tools/ha_bench.py [--steps 3] [--warmup 1]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from xpoint_amd import _lib, homographies as ha, models, synth, utils  # noqa: E402

COPY_RATE = 6.29e12
HA_TAGS = ("ha_warp", "ha_valid_mask", "ha_accumulate", "ha_gaussian")
CFG = {"aggregation": "window", "weighted_window": True, "window_size": 5, "erosion_radius": 3, "mask_border": True, "min_count": 5,
       "filter_size": 0, "homographies": {"translation": True, "rotation": True, "scaling": True, "perspective": True, "scaling_amplitude": 0.2,
                                          "perspective_amplitude_x": 0.2, "perspective_amplitude_y": 0.2, "patch_ratio": 0.85,
                                          "max_angle": 1.57, "allow_artifacts": True}}


def prof_rows(lib):
    name = ctypes.create_string_buffer(64)
    ms, cnt, fl, by = ctypes.c_double(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    rows = {}
    for i in range(lib.xp_prof_count()):
        lib.xp_prof_get(i, name, 64, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by))
        rows[name.value.decode()] = dict(ms=ms.value, launches=cnt.value, bytes=by.value)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--nums", default="10,100")
    args = ap.parse_args()
    H, W = 480, 640
    cfg = synth.xpoint_exp1_config(H, W)
    cfg["takes_pair"] = False
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg), strict=True)
    net.to("cuda").eval()
    data = synth.to_torch(synth.make_pair_batch(0, 1, H, W), "cuda")
    lib = _lib.load()
    res = {"what": "homographic adaptation, 480x640, 1 pair, window aggregation", "copy_rate_tb_s": COPY_RATE / 1e12, "runs": []}
    with torch.no_grad():
        for num in [int(v) for v in args.nums.split(",")]:
            np.random.seed(0)
            hs = [ha.sample_homography(np.array([H, W]), **CFG["homographies"]) for _ in range(num - 1)]
            c = dict(CFG, num=num)
            for chunk in (None, 1):
                run = lambda: utils.homographic_adaptation_multispectral(data, net, c, homographies=hs, chunk=chunk)  # noqa: E731
                for _ in range(args.warmup):
                    run()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / args.steps * 1e3
                lib.xp_prof_reset(); lib.xp_prof_filter(None); lib.xp_prof_enable(1)
                run(); torch.cuda.synchronize()
                lib.xp_prof_enable(0)
                rows = prof_rows(lib)
                ha_ms = sum(r["ms"] for t, r in rows.items() if t in HA_TAGS)
                fwd_ms = sum(r["ms"] for t, r in rows.items() if t not in HA_TAGS)
                bw = {t: (rows[t]["bytes"] / (rows[t]["ms"] * 1e-3) if t in rows and rows[t]["ms"] > 0 else None) for t in ("ha_warp", "ha_accumulate")}
                res["runs"].append({
                    "num": num, "chunk": chunk if chunk else min(num, 16), "ms_per_pair": round(ms, 3),
                    "event_ms": {"forwards": round(fwd_ms, 3), "ha_kernels": round(ha_ms, 3),
                                 **{t: round(rows[t]["ms"], 4) for t in HA_TAGS if t in rows}},
                    "ha_share_of_events": round(ha_ms / (ha_ms + fwd_ms), 4) if ha_ms + fwd_ms > 0 else None,
                    "achieved_tb_s": {t: (round(v / 1e12, 3) if v else None) for t, v in bw.items()},
                    "frac_of_copy_rate": {t: (round(v / COPY_RATE, 3) if v else None) for t, v in bw.items()},
                })
        for num in sorted({r["num"] for r in res["runs"]}):
            d, one = [r["ms_per_pair"] for r in res["runs"] if r["num"] == num]
            res[f"speedup_default_vs_chunk1_num{num}"] = round(one / d, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
