"""Generate tests/golden/g30_head_training.npz by running the REAL reference heads in training mode (xpoint.models.XPoint.detector_head /
descriptor_head of the reference tree, built by oracle/refharness, which this tool imports and does not modify) forward and `.backward()`
on the CPU, with the two head modules cast to float64 (see below).  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_heads.py

The reference XPoint is built in both configurations (build_reference_xpoint: VMamba, Ci = 48, D = 256; build_reference_conv_xpoint: conv
encoder, Ci = 128, D = 64) with the synthetic weights, put in `.train()`, and its heads are fed the fixed encoder tensor of each case of
tests/heads_f64.py; sum logits R1 + sum desc R2 is back-propagated.  Inputs are hash uniforms the tests regenerate; the file holds, per case,
  <case>/seed                     the input seed (the first of eight whose pre-activations meet the ReLU floor, heads_f64.case_seed)
  <case>/logits, <case>/desc      the outputs (desc with a channel stride)
  <case>/grad/<parameter>         every head parameter's gradient (the convolution weights strided: heads_f64.GOLDEN_STRIDES)
  <case>/<buffer>                 running_mean / running_var / num_batches_tracked of the four BatchNorms after the step
Why the head modules run in float64: a BatchNorm over the 4 values of the (1, 2, 2) cases has channels whose variance is far below eps
(one weakly active row behind the ReLU), so invstd reaches 1 / sqrt(eps) = 316 and the float32 model's own rounding is amplified.  Measured
with the modules in float32: d(detector 1.bias) of conv/1x2x2 differs from float64 by 2.1e-5 of the tensor's scale (2.3e-3 on 110.9) — and a
float32 run of the restatement reproduces that figure digit for digit, i.e. it is the arithmetic's error, not a difference between the two
programs — which is above the 1e-5 bar the CPU test pins the restatement at.  In float64 the same reference code is a reference for that bar.
The reference's own `.to(torch.float)` on both outputs (XPoint.py:349,363) and its float32 F.normalize stay as they are; arrays are stored
as float32.  One thread; fixed zip timestamps: a re-run is byte-identical."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.refharness.build_ref import build_reference_conv_xpoint, build_reference_xpoint  # noqa: E402
from oracle.refharness.make_golden import savez_deterministic  # noqa: E402
from tests import heads_f64 as Hd  # noqa: E402
from xpoint_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g30_head_training.npz")


def main():
    torch.set_num_threads(1)
    g = {}
    for kind in Hd.CONFIGS:
        cfg = Hd.model_config(kind)
        if kind == "vmamba":
            net = build_reference_xpoint(cfg, synth.make_state_dict(cfg))
        else:
            net = build_reference_conv_xpoint(cfg, synth.make_conv_xpoint_state_dict(cfg))
        start = {k: v.detach().clone() for k, v in net.state_dict().items() if k.startswith(Hd.DET) or k.startswith(Hd.DSC)}
        for case in (c for c in Hd.CASES if c.startswith(kind + "/")):
            net.load_state_dict(start, strict=False)
            net.train()
            net.detector_head_convolutions.double(); net.descriptor_head_convolutions.double()
            net.zero_grad()
            seed = Hd.case_seed(case)
            enc, r1, r2 = Hd.case_inputs(case, seed)
            _, logits = net.detector_head(enc.double())
            desc = net.descriptor_head(enc.double())
            ((logits * r1).sum() + (desc * r2).sum()).backward()
            g[f"{case}/seed"] = np.int64(seed)
            g[f"{case}/logits"] = logits.detach().numpy()
            g[f"{case}/desc"] = Hd.golden_view("desc", desc.detach()).numpy()
            params = dict(net.named_parameters())
            for k in start:
                if k in params:
                    g[f"{case}/grad/{k}"] = Hd.golden_view(k, params[k].grad).float().numpy()
                else:
                    v = net.state_dict()[k].detach()
                    g[f"{case}/{k}"] = (v.float() if v.is_floating_point() else v).numpy().copy()
            print(f"{case}: seed {seed}, |logits| {float(logits.abs().max()):.4g}, |dW1| {float(params[Hd.DET + '1.weight'].grad.abs().max()):.4g}")
    savez_deterministic(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(g)} arrays)")


if __name__ == "__main__":
    main()
