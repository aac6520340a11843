"""Measure SyntheticShapes generation at the reference's sizes (960 x 1280 -> 240 x 320, batch 32), per primitive and for 'all', next to one
`training.pretrain_step` at 256 x 320, batch 32 (the model of XPoint-EXP1's params.yaml, f32-grade training; the VMamba encoder takes multiples
of 32 only, so the reference's 240 rows become 256: the step's batch is generated at 1024 x 1280 -> 256 x 320).

    python tools/synth_shapes_bench.py [--runs 3] [--reps 5] [--steps 3] [--restatement-images 1]

Per case one JSON line: host ms per batch (`sample_draw_lists` + `pack_draw_lists`, a host clock; fresh indices every batch), device ms per
batch (`render` between device events, after a warm-up: the uploads of the tables are part of a batch), kernel launches per batch (DERIVED, not
counted: the entry-point calls of the xp_prof_* rows times the kernels each entry point launches, a table kept in this file) and images / s
of the slower of the two sides; every time as median [min, max] over `--runs` windows of `--reps` batches.  After the eight primitives and
their 'all', the same for draw_multiple_polygons alone and for the 'all' of nine (the dataset key textured_polygons), with the arena of the
texture jobs (MiB per batch) and the three texture launches' own time (the xp_prof_* row of xp_synth_texture, a run with the event timing on)
against their algorithmic bytes: every float of the arena written once and read once.  Then the
pretrain step's ms the same way, the sentence that matters (is a batch generated in less time than it is consumed, host side and device side
separately), and, for context, the CPU seconds per image of the numpy restatement (tests/synthetic_shapes_f64.py) on this machine: that is
NOT the reference's time (OpenCV is not installed; its generator cannot run here)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xpoint_amd import augmentation as aug, losses, synth, synthetic_shapes as ss, training  # noqa: E402

GEN, IMG, B = [960, 1280], [240, 320], 32
STEP_GEN, STEP_IMG = [1024, 1280], [256, 320]          # the VMamba encoder takes multiples of 32
DEV = "cuda:0"


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def bench_case(primitives, runs, reps, first_index, textured=False):
    cfg = ss.merge_config({'primitives': primitives, 'textured_polygons': textured, 'generation_size': GEN, 'image_size': IMG})
    host, device = [], []
    index = first_index

    def batch():
        nonlocal index
        t0 = time.perf_counter()
        tables = ss.pack_draw_lists(ss.sample_draw_lists(cfg, range(index, index + B), seed=1), GEN)
        index += B
        return tables, (time.perf_counter() - t0) * 1e3

    tables, _ = batch()
    ss.render(tables, GEN, IMG, 1, DEV)                                   # warm-up: code objects, allocator
    rows = aug.profile_launches(lambda: ss.render(tables, GEN, IMG, 1, DEV))
    two = ("synth_background", "synth_box_blur", "synth_resolve_colours")  # entry points that launch two kernels; every other one launches one
    launches = int(sum(r[0] * (3 if tag == "synth_texture" else 2 if tag in two else 1) for tag, r in rows.items()))
    arena = []
    for _ in range(runs):
        h, batches = [], []
        for _ in range(reps):
            tables, ms = batch()
            h.append(ms)
            batches.append(tables)
            if textured:
                jobs = ss.texture_jobs(tables, GEN)
                arena.append(jobs['arena_floats'] * 4 / 2 ** 20 if jobs else 0.0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for tables in batches:
            ss.render(tables, GEN, IMG, 1, DEV)
        e1.record()
        torch.cuda.synchronize()
        host.append(sum(h) / reps)
        device.append(e0.elapsed_time(e1) / reps)
    slower = max(statistics.median(host), statistics.median(device))
    row = {"primitives": primitives, "batch": B, "host_ms_per_batch": spread(host), "device_ms_per_batch": spread(device),
           "kernel_launches_per_batch_derived": launches, "images_per_s": round(B / slower * 1e3, 1)}
    if textured:
        row["textured_polygons"] = True
        row["texture_arena_mib_per_batch"] = spread(arena)
        tex = [aug.profile_launches(lambda: ss.render(t, GEN, IMG, 1, DEV)).get("synth_texture") for t in batches]
        tex = [t for t in tex if t]
        if tex:          # (calls, ms, algorithmic bytes) of the three texture launches of one batch
            row["texture_launches_ms"] = spread([t[1] for t in tex])
            row["texture_launches_gb_per_s"] = spread([t[2] / (t[1] * 1e-3) / 1e9 for t in tex])
    return row


def bench_pretrain(runs, steps):
    cfg = synth.xpoint_exp1_config(*STEP_IMG)
    cfg["mixed_precision"] = False
    from xpoint_amd import models
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    model = training.XPointNet.from_model(net.to(DEV).eval()).cuda().train()
    ds = ss.SyntheticShapes({'generation_size': STEP_GEN, 'image_size': STEP_IMG})
    data = ds.load_batch(list(range(B)), DEV, seed=1, is_optical=True)
    loss_fn = losses.XPointLoss({'detector_loss': True, 'detector_use_cross_entropy': True, 'descriptor_loss': False, 'detector_loss_function': 'cross_entropy',
                                 'detector_handle_multiple_keypoints': 'hard_assignment', 'detector_focal_loss': {'use': False}})
    opt = training.Adam(model.parameters(), lr=1e-4)
    for s in range(2):
        training.pretrain_step(model, data, loss_fn, opt, seed=s)
    ms = []
    for r in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(steps):
            training.pretrain_step(model, data, loss_fn, opt, seed=2 + r * steps + s)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    return {"pretrain_step_ms": spread(ms), "batch": B, "image": STEP_IMG, "steps_per_window": steps}


def restatement_seconds(n):
    from tests import synthetic_shapes_f64 as ref
    lists = ss.sample_draw_lists({'generation_size': GEN, 'image_size': IMG}, range(n), seed=1)
    tables = ss.pack_draw_lists(lists, GEN)
    field = np.random.default_rng(0).random((n, *GEN), dtype=np.float32)          # any uniform field: the time does not depend on its values
    t0 = time.perf_counter()
    for b in range(n):
        ref.render(tables, b, field[b], field[b], GEN, IMG, 0.1)
    return (time.perf_counter() - t0) / n, [d['primitive'] for d in lists]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--restatement-images", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("synth_shapes_bench needs a GPU: nothing here is measured without one")
    print(f"# SyntheticShapes {GEN[0]} x {GEN[1]} -> {IMG[0]} x {IMG[1]}, batch {B}; median [min, max] over {args.runs} windows of {args.reps} batches; "
          f"{torch.cuda.get_device_name(0)}")
    rows = []
    for k, prims in enumerate([[p] for p in ss.IMPLEMENTED] + ['all']):
        rows.append(bench_case(prims, args.runs, args.reps, first_index=100000 * k))
        print(json.dumps(rows[-1]), flush=True)
    for k, prims in enumerate([['draw_multiple_polygons'], 'all']):
        rows.append(bench_case(prims, args.runs, args.reps, first_index=100000 * (len(ss.ALL_PRIMITIVES) + k), textured=True))
        print(json.dumps(rows[-1]), flush=True)
    step = bench_pretrain(args.runs, args.steps)
    print(json.dumps(step), flush=True)
    ms = step["pretrain_step_ms"]["median"]
    for name, gen in (("'all' of eight", rows[len(ss.IMPLEMENTED)]), ("'all' of nine (textured_polygons)", rows[-1])):
        for side in ("host", "device"):
            g = gen[f"{side}_ms_per_batch"]["median"]
            print(f"# {name}: the {side} side generates a batch in {g:.1f} ms, one pretrain_step consumes it in {ms:.1f} ms: generation is "
                  f"{'FASTER' if g < ms else 'SLOWER'} than consumption on the {side} side ({g / ms:.2f} x)")
    if args.restatement_images > 0:
        sec, prims = restatement_seconds(args.restatement_images)
        print(f"# numpy restatement (tests/synthetic_shapes_f64.py) on this machine's CPU: {sec:.2f} s per image ({prims}); NOT the reference's time")


if __name__ == "__main__":
    main()
