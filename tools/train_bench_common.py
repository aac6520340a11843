"""The method tools/head_train_bench.py, tools/regnet_train_bench.py and tools/vss_train_bench.py share: a training step on the HIP library
(xpoint_amd.training) against torch eager autograd of the same module, f32, on the same GPU.  The two sides alternate in the same call; device events
after a warm-up, `iters` iterations each, and next to each the time the host needs to issue an iteration; then the HIP side's per-kernel split from the
library's event profiler (one profiled iteration).  Nothing is asserted."""
import ctypes
import time

import torch

from xpoint_amd import _lib


def measure(step, iters):
    """-> (device ms per iteration, peak MiB above the resident set); measure.host_ms: the host's ms to issue one iteration"""
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


def alternate(res, step_hip, step_eager, iters, tags=("hip", "eager")):
    """Fill `res` with both sides' times, peak memory and host issue time — hip, eager, hip, eager — and their ratio.  tags: the two sides' names (two
    forms of the HIP side against each other: ("pixel", "routes"))."""
    a, b = tags
    for rep in range(2):
        for tag, st in ((a, step_hip), (b, step_eager)):
            ms, mib = measure(st, iters)
            res.setdefault(f"{tag}_fwd_bwd_ms", []).append(round(ms, 4))
            res[f"{tag}_peak_MiB"] = round(mib, 1)
            res[f"{tag}_host_issue_ms"] = round(measure.host_ms, 4)
    res[f"ratio_{a}_over_{b}"] = round(min(res[f"{a}_fwd_bwd_ms"]) / min(res[f"{b}_fwd_bwd_ms"]), 3)
    if tags != ("hip", "eager"):
        for tag in tags:
            res[f"{tag}_spread"] = round((max(res[f"{tag}_fwd_bwd_ms"]) - min(res[f"{tag}_fwd_bwd_ms"])) / min(res[f"{tag}_fwd_bwd_ms"]), 3)
    return res
