"""Generate tests/golden/g26_selective_scan_bwd.npz by running the REAL reference selective scan (xpoint.models.vmamba_src.csms6s.
selective_scan_torch, imported from the reference tree with the harness shims of oracle/refharness, which this tool imports and does not
modify) forward and `.backward()` on the CPU.  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_scan_bwd.py

Inputs: oracle.refharness.make_golden.scan_inputs (the recipe of reference test_selective_scan.py:409-444 on the build's hash RNG) and
dout = synth.uniform(name + "/dout", (B, K*C, L), -1, 1).  For each case the seven gradients of reference selective_scan_oflex.bwd's list
[du, ddelta, dA, dB, dC, dD, ddelta_bias] are stored under scan/<B>_<K>_<C>_<N>_<L>/<grad> (with D, delta_bias and softplus) and, on the
cases that are small enough, <grad>_plain for du, ddelta, dA, dB, dC (no D, no delta_bias, no softplus).  The reference casts to float32
internally, so every array is float32.  Cases: the SCAN_CASES of at most 32 768 (batch, channel, position) elements, plus 1x2x16x1x2049 (the
2048-element chunk boundary) with the full variant only, which keeps the file under 1.5 MB.  One thread; the file is written with fixed zip
timestamps, so a re-run is byte-identical.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.refharness import stubs  # noqa: E402
from oracle.refharness.make_golden import SCAN_CASES, savez_deterministic, scan_inputs  # noqa: E402
from xpoint_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g26_selective_scan_bwd.npz")
GRADS = ("du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias")


def cases():
    small = [c for c in SCAN_CASES if c[0] * c[1] * c[2] * c[4] <= 32768]
    return [(c, True) for c in small] + [((1, 2, 16, 1, 2049), False)]


def run(csms6s, u, delta, A, Bm, Cm, Dv, bias, dout, full):
    ins = [t.clone().requires_grad_(True) for t in (u, delta, A, Bm, Cm, Dv, bias)]
    if full:
        out = csms6s.selective_scan_torch(*ins, True, True)
    else:
        out = csms6s.selective_scan_torch(*ins[:5], None, None, False, True)
    out.backward(dout)
    return [t.grad.numpy() if t.grad is not None else None for t in ins]


def main():
    torch.set_num_threads(1)
    stubs.install()
    from xpoint.models.vmamba_src import csms6s
    g = {}
    for case, plain in cases():
        name = "scan/%d_%d_%d_%d_%d" % case
        B, K, C, N, L = case
        inputs = [torch.from_numpy(x) for x in scan_inputs(name, *case)]
        dout = torch.from_numpy(synth.uniform(name + "/dout", (B, K * C, L), -1.0, 1.0))
        for gname, v in zip(GRADS, run(csms6s, *inputs, dout, True)):
            g[f"{name}/{gname}"] = v
        if plain:
            for gname, v in zip(GRADS[:5], run(csms6s, *inputs, dout, False)):
                g[f"{name}/{gname}_plain"] = v
    savez_deterministic(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(g)} arrays)")


if __name__ == "__main__":
    main()
