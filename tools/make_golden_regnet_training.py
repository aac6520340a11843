"""Generate tests/golden/g31_regnet_training.npz by running the REAL reference homography head in training mode (xpoint.models.RegNet of the
reference tree, as the `hm_regressor` of the XPoint that oracle/refharness builds; this tool imports the harness and does not modify it) forward and
`.backward()` on the CPU, with the module cast to float64.  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_regnet_training.py

The reference XPoint is built with the homography head (synth.xpoint_exp1_config(256, 256, hm_head=True)) and the synthetic weights; its
`hm_regressor` is put in `.train()`, cast to `.double()` and fed the two encoder tensors of each case of tests/regnet_f64.py; sum hm * R is
back-propagated.  Forward hooks on the two nn.Dropout modules record the masks the reference drew: an element is kept where the output is non-zero,
and a position whose INPUT is exactly 0 counts as kept (its output is 0 either way: behind the first dropout such inputs do not occur generically,
behind the second the fc ReLU gates them, so the choice changes no value and no gradient).  Inputs are hash uniforms the tests regenerate; the file
holds, per case,
  <case>/hm                        the output (B, 8)
  <case>/mask1, <case>/mask2       the kept elements of the two dropouts, uint8 (B, 256), (B, 64)
  <case>/grad/<parameter>          every parameter's gradient (the two convolution weights strided: regnet_f64.GOLDEN_STRIDES)
  <case>/<buffer>                  running_mean / running_var / num_batches_tracked of the two BatchNorms after the step (two updates each)
Float64 for the reason tools/make_golden_heads.py gives: the float32 module's own rounding is not a reference for the 1e-5 bar of the CPU test.
Arrays are stored as float32.  One thread, a fixed torch seed per case for the dropout draws, fixed zip timestamps: a re-run is byte-identical."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.refharness.build_ref import build_reference_xpoint  # noqa: E402
from oracle.refharness.make_golden import savez_deterministic  # noqa: E402
from tests import regnet_f64 as Rg  # noqa: E402
from xpoint_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g31_regnet_training.npz")


def main():
    torch.set_num_threads(1)
    cfg = Rg.model_config()
    net = build_reference_xpoint(cfg, synth.make_state_dict(cfg))
    reg = net.hm_regressor
    start = {k: v.detach().clone() for k, v in reg.state_dict().items()}
    masks = []

    def record(_module, inputs, output):
        masks.append(((output != 0) | (inputs[0] == 0)).to(torch.uint8))

    hooks = [m.register_forward_hook(record) for m in reg.modules() if isinstance(m, torch.nn.Dropout)]
    assert len(hooks) == 2
    g = {}
    for n, case in enumerate(Rg.CASES):
        reg.float().load_state_dict(start)
        reg.train().double()
        reg.zero_grad()
        del masks[:]
        torch.manual_seed(3100 + n)
        enc1, enc2, R = Rg.case_inputs(case)
        hm = reg(enc1.double(), enc2.double())
        (hm * R.double()).sum().backward()
        assert len(masks) == 2
        g[f"{case}/hm"] = hm.detach().float().numpy()
        g[f"{case}/mask1"], g[f"{case}/mask2"] = masks[0].numpy().copy(), masks[1].numpy().copy()
        params = dict(reg.named_parameters())
        for k in start:
            name = Rg.HM + k
            if k in params:
                g[f"{case}/grad/{name}"] = Rg.golden_view(name, params[k].grad).float().numpy().copy()
            else:
                v = reg.state_dict()[k].detach()
                g[f"{case}/{name}"] = (v.float() if v.is_floating_point() else v).numpy().copy()
        print(f"{case}: |hm| {float(hm.abs().max()):.4g}, kept {float(masks[0].float().mean()):.3f} / {float(masks[1].float().mean()):.3f}, "
              f"|dW1| {float(params['layer1.0.weight'].grad.abs().max()):.4g}")
    for h in hooks:
        h.remove()
    savez_deterministic(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(g)} arrays)")


if __name__ == "__main__":
    main()
