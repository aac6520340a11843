"""Generate tests/golden/g32_vss_training.npz by running a REAL reference VSS block (xpoint.models.vmamba_src.VMamba.VSSBlock of the reference tree, as
`net.encoder.layers[s].blocks[0]` of the XPoint that oracle/refharness builds; this tool imports the harness and does not modify it) forward and
`.backward()` on the CPU, with the module cast to float64.  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_vss_training.py

For each fixture case of tests/vss_f64.py the reference XPoint is built with EMBED_DIM = E, DEPTHS [1, 1, 1, 1] and the synthetic weights; the block is
cast to `.double()` and kept in `.eval()` (the harness's DropPath shim is eval-only; LayerNorm has no mode, so the block's arithmetic is that of training
without stochastic depth), fed the case input with requires_grad, and sum(out * R) is back-propagated.  The file holds, per case,
  <case>/out                 the output (B, H, W, C)
  <case>/grad/x              the input gradient
  <case>/grad/<parameter>    the gradient of each of the 18 parameters, under the reference's names without the block prefix
The module is float64, but forward_corev2 casts A and D, and selective_scan_torch its other operands, to float32, so the scan runs and returns in float32
and tensors behind it carry that rounding (tests/test_cpu_vss_training.py and DESIGN.md section 16 state the bars).  F.layer_norm refuses a float32
input under float64 parameters, so a forward pre-hook on `op.out_norm` (registered here, on the module instance) widens the scan's output to float64.  Arrays are stored as float32.  One thread, fixed zip timestamps: a
re-run is byte-identical."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.refharness.build_ref import build_reference_xpoint  # noqa: E402
from oracle.refharness.make_golden import savez_deterministic  # noqa: E402
from tests import vss_f64 as V  # noqa: E402
from xpoint_amd import synth  # noqa: E402

OUT = V.GOLDEN


def main():
    torch.set_num_threads(1)
    g = {}
    for case in V.GOLDEN_CASES:
        shape, R, E, stage = V.CASES[case]
        cfg = V.model_config(E)
        net = build_reference_xpoint(cfg, synth.make_state_dict(cfg))
        blk = net.encoder.layers[stage].blocks[0].double().eval()
        # the float32 scan output meets out_norm's float64 parameters: F.layer_norm refuses the mix, so the tensor is widened on its way in
        blk.op.out_norm.register_forward_pre_hook(lambda _module, args: (args[0].double(),))
        assert tuple(blk.op.dt_projs_weight.shape) == (4, shape[3], R)
        blk.zero_grad()
        x, Rw = V.case_inputs(case)
        x = x.double().requires_grad_(True)
        out = blk(x)
        assert out.shape == x.shape
        (out * Rw.double()).sum().backward()
        g[f"{case}/out"] = out.detach().float().numpy()
        g[f"{case}/grad/x"] = x.grad.float().numpy().copy()
        params = dict(blk.named_parameters())
        assert list(params) == list(V.LEAVES), list(params)
        for k in V.LEAVES:
            g[f"{case}/grad/{k}"] = params[k].grad.float().numpy().copy()
        print(f"{case}: |out| {float(out.abs().max()):.4g}, |dx| {float(x.grad.abs().max()):.4g}, "
              f"|dW_in| {float(params['op.in_proj.weight'].grad.abs().max()):.4g}")
    savez_deterministic(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(g)} arrays)")


if __name__ == "__main__":
    main()
