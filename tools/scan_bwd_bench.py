"""Timing of the selective-scan backward (xp_selective_scan_bwd_typed) at the XPoint training / inference shapes.

    python tools/scan_bwd_bench.py [--iters 20] [--no-rocprof] [--no-eager] [--out DIR]

Per shape: forward (selective_scan_fn's differentiable forward, which also writes the chunk states), backward (selective_scan_bwd alone)
and forward + backward through autograd, from device events; the algorithmic bytes of the backward (u, delta, dout read and du, ddelta
written per (b, d, l); B, C read and dB, dC written per (b, g, l); the dB / dC partial slab written and read once), the achieved TB/s and
the share of the 6.29 TB/s copy rate.  Then the same script runs once more under `rocprofv3 --kernel-trace --stats` (a child process) and
prints the per-kernel times, and at shape (b) it times the fallback a reference user has without the extension: eager torch autograd of a
per-step scan (restated here, the shape of the reference's selective_scan_torch) on the same GPU.
Shapes: (a) 480x640 stage 0, B 8, D 384, L 19 200, f32; (b) the 256x256 training crop of configs/cipdp.yaml at stage 0, B 16, D 384,
L 4 096, f32 and f16 inputs with f32 dout (the reference's AMP training); (c) 480x640 stage 2, B 8, D 1 536, L 1 200, f32."""
import argparse
import csv
import glob
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xpoint_amd.kernels import selective_scan_bwd, selective_scan_fn  # noqa: E402

COPY_TBS = 6.29
SHAPES = [("a 480x640 s0 f32", 8, 4, 96, 19200, torch.float32), ("b 256x256 s0 f32", 16, 4, 96, 4096, torch.float32),
          ("b 256x256 s0 f16/f32 dout", 16, 4, 96, 4096, torch.float16), ("c 480x640 s2 f32", 8, 4, 384, 1200, torch.float32)]


def inputs(B, K, C, L, dt):
    g = torch.Generator(device="cuda").manual_seed(0)
    D = K * C
    r = lambda *s: torch.rand(*s, device="cuda", generator=g)          # noqa: E731
    u, delta = (r(B, D, L) * 3.4 - 1.7).to(dt), (0.5 * r(B, D, L)).to(dt)
    A = -0.5 * r(D, 1)
    Bm, Cm = (r(B, K, 1, L) * 3.4 - 1.7).to(dt), (r(B, K, 1, L) * 3.4 - 1.7).to(dt)
    Dv, bias = r(D) * 3.4 - 1.7, 0.5 * r(D)
    dout = r(B, D, L) * 2 - 1
    return [u, delta, A, Bm, Cm, Dv, bias], dout


def bwd_bytes(B, K, C, L, dt):
    isz = 2 if dt != torch.float32 else 4
    D = K * C
    tiles = (C + 7) // 8                   # workgroups of 8 channels (d_state 1)
    return (4 * isz + 4) * B * D * L + 4 * isz * B * K * L + 2 * 2 * 4 * tiles * B * K * L   # u, delta, du, ddelta + f32 dout; B, C, dB, dC; slab


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def eager_scan(u, delta, A, Bm, Cm, Dv, bias):
    """Per-step selective scan in eager torch (the shape of the reference's selective_scan_torch fallback, csms6s.py:25-68)."""
    Bb, K, N, L = Bm.shape
    D = u.shape[1]
    dl = torch.nn.functional.softplus(delta + bias[..., None])
    Bx = Bm.repeat_interleave(D // K, 1)
    Cx = Cm.repeat_interleave(D // K, 1)
    dA = torch.exp(torch.einsum("bdl,dn->bdln", dl, A))
    dBu = torch.einsum("bdl,bdnl,bdl->bdln", dl, Bx, u)
    h = u.new_zeros((Bb, D, N))
    ys = []
    for i in range(L):
        h = dA[:, :, i] * h + dBu[:, :, i]
        ys.append(torch.einsum("bdn,bdn->bd", h, Cx[:, :, :, i]))
    return torch.stack(ys, 2) + u * Dv[:, None]


def run(iters, eager):
    for name, B, K, C, L, dt in SHAPES:
        ins, dout = inputs(B, K, C, L, dt)
        leaves = [t.clone().requires_grad_(True) for t in ins]
        with torch.enable_grad():
            out = selective_scan_fn(*leaves, True)
        x = out.grad_fn.saved_tensors[-1]
        f_ms = timed(lambda: selective_scan_fn(*leaves, True), iters)
        b_ms = timed(lambda: selective_scan_bwd(*ins, dout, x, True, 1), iters)
        fb_ms = timed(lambda: torch.autograd.grad(selective_scan_fn(*leaves, True), leaves, dout), iters)
        by = bwd_bytes(B, K, C, L, dt)
        tbs = by / (b_ms * 1e-3) / 1e12
        print(f"[{name}] B{B} D{K * C} L{L}: fwd {f_ms * 1e3:8.1f} us  bwd {b_ms * 1e3:8.1f} us  fwd+bwd {fb_ms * 1e3:8.1f} us | bwd bytes "
              f"{by / 1e9:.3f} GB -> {tbs:.2f} TB/s = {tbs / COPY_TBS:.2f} of the {COPY_TBS} TB/s copy rate", flush=True)
        if eager and name.startswith("b") and dt == torch.float32:
            el = [t.clone().requires_grad_(True) for t in ins]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.autograd.grad(eager_scan(*el), el, dout)
            e1.record()
            torch.cuda.synchronize()
            e_ms = e0.elapsed_time(e1)
            print(f"[{name}] eager torch autograd per-step scan fwd+bwd {e_ms:10.1f} ms -> HIP fwd+bwd is {e_ms / fb_ms:.0f}x faster", flush=True)
        del ins, dout, leaves, out, x
        torch.cuda.empty_cache()


def rocprof(out_dir, iters):
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "scan_bwd", "--", sys.executable,
           os.path.abspath(__file__), "--iters", str(iters), "--no-rocprof", "--no-eager"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print(f"rocprofv3 exited {r.returncode}:\n{r.stderr[-2000:]}")
        return
    stats = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        print("rocprofv3: no kernel_stats.csv")
        return
    print(f"rocprofv3 --kernel-trace --stats ({stats[-1]}):")
    with open(stats[-1]) as f:
        for row in csv.DictReader(f):
            nm = row["Name"]
            if "selective_scan" in nm:
                print(f"  {row['Calls']:>6} calls  avg {float(row['AverageNs']) / 1e3:9.1f} us  total {float(row['TotalDurationNs']) / 1e6:9.2f} ms  "
                      f"{nm[:110]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "scan_bwd_prof"))
    a = ap.parse_args()
    run(a.iters, not a.no_eager)
    if not a.no_rocprof:
        rocprof(a.out, max(2, a.iters // 4))


if __name__ == "__main__":
    main()
