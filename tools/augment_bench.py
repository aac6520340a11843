"""Measure one `augment_pair_batch` of 16 and of 32 pairs at 256 x 256 (cmt.yaml's crop and batch), photometric off and on.

    python tools/augment_bench.py [--seconds 1.0] [--host-samples 4]

Per case one JSON line: ms per batch (device events around a synchronised region of at least `--seconds`, after warm-up: the region
includes the host's scalar draws and table uploads, which are part of a batch), entry-point calls per batch (xp_prof_* rows), the
algorithmic bytes of those calls over the event time as a share of the MI355X's 8 TB/s HBM bandwidth, and, for context, the host time
of the numpy restatement (tests/augmentation_f64.py) of the same work on this machine, measured on `--host-samples` pairs and scaled to
the batch."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import augmentation_f64 as A  # noqa: E402
from xpoint_amd import augmentation as aug, homographies as hom  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
H = W = 256
CONFIG = {'photometric': {'enable': True, 'random_order': True,
                          'primitives': ['random_brightness', 'random_contrast', 'additive_speckle_noise', 'additive_gaussian_noise',
                                         'additive_shade', 'motion_blur'],
                          'params': {'random_brightness': {'max_abs_change': 0.15}, 'random_contrast': {'strength_range': [0.3, 1.8]},
                                     'additive_gaussian_noise': {'stddev_range': [0, 0.06]}, 'additive_speckle_noise': {'prob_range': [0, 0.0035]},
                                     'additive_shade': {'transparency_range': [-0.5, 0.8], 'kernel_size_range': [50, 100]},
                                     'motion_blur': {'max_kernel_size': 3}}},
          'homographic': {'enable': True, 'valid_border_margin': 0, 'border_reflect': True,
                          'params': {'translation': True, 'rotation': True, 'scaling': True, 'perspective': True, 'scaling_amplitude': 0.2,
                                     'perspective_amplitude_x': 0.2, 'perspective_amplitude_y': 0.2, 'patch_ratio': 0.85, 'max_angle': 1.57,
                                     'allow_artifacts': True, 'translation_overflow': 0.05}}}


def make_batch(B, dev):
    rng = np.random.default_rng(0)
    batch = {}
    for k, flag in (('optical', True), ('thermal', False)):
        img = torch.from_numpy(rng.random((B, 1, H, W), dtype=np.float32)).to(dev)
        batch[k] = {'image': img, 'valid_mask': torch.ones_like(img, dtype=torch.bool), 'is_optical': torch.full((B, 1), flag, device=dev),
                    'keypoints': torch.from_numpy(rng.random((B, H, W)) < 0.005).to(dev)}
    return batch


def host_restatement(n, photometric):
    """the numpy restatement of one pair's augmentation, n times; seconds per pair"""
    rng = np.random.default_rng(0)
    np.random.seed(0)
    prog = aug.sample_photometric_params(CONFIG['photometric'], 2 * n, (H, W), rng)
    fields = {'additive_gaussian_noise': rng.standard_normal((2 * n, H, W)), 'additive_speckle_noise': rng.random((2 * n, H, W))}
    imgs = rng.random((2 * n, H, W), dtype=np.float32)
    maps = rng.random((n, H, W)) < 0.005
    t0 = time.perf_counter()
    for i in range(n):
        pair = [imgs[i], imgs[n + i]]
        if photometric:
            pair = [A.run_program(pair[0], prog, i, fields).astype(np.float32), A.run_program(pair[1], prog, n + i, fields).astype(np.float32)]
        Hm = hom.sample_homography((H, W), **CONFIG['homographic']['params'])
        A.warp_perspective_f32(pair[0], Hm, True)
        A.compute_valid_mask((H, W), Hm, 0, True)
        A.warp_label_map(maps[i], Hm)
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--host-samples", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for B in (16, 32):
        batch = make_batch(B, dev)
        for photometric in (False, True):
            cfg = {'photometric': dict(CONFIG['photometric'], enable=photometric), 'homographic': CONFIG['homographic']}
            rng = np.random.default_rng(1)
            np.random.seed(1); random.seed(1)
            step = lambda: aug.augment_pair_batch(batch, cfg, rng, seed=3)
            for _ in range(3):
                step()
            rows = aug.profile_launches(step)
            calls = sum(v[0] for v in rows.values())
            kernel_ms, bytes_ = sum(v[1] for v in rows.values()), sum(v[2] for v in rows.values())
            torch.cuda.synchronize()
            n, elapsed = 0, 0.0
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            t0 = time.perf_counter()
            while elapsed < args.seconds:
                for _ in range(8):
                    step()
                n += 8
                torch.cuda.synchronize()
                elapsed = time.perf_counter() - t0
            stop.record()
            torch.cuda.synchronize()
            ms = start.elapsed_time(stop) / n
            host = host_restatement(args.host_samples, photometric) * B * 1e3
            print(json.dumps({"pairs": B, "size": [H, W], "photometric": photometric, "ms_per_batch": round(ms, 4), "batches": n,
                              "region_s": round(elapsed, 3), "calls_per_batch": calls, "calls": {k: v[0] for k, v in sorted(rows.items())},
                              "kernel_ms_per_batch": round(kernel_ms, 4), "algorithmic_bytes": bytes_,
                              "hbm_share_of_event_time": round(bytes_ / (ms * 1e-3) / HBM_BYTES_PER_S, 5),
                              "hbm_share_of_kernel_time": round(bytes_ / (kernel_ms * 1e-3) / HBM_BYTES_PER_S, 5) if kernel_ms > 0 else None,
                              "host_numpy_restatement_ms_per_batch": round(host, 1)}), flush=True)


if __name__ == "__main__":
    main()
