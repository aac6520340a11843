"""Generate tests/golden/g34_xpoint_training.npz by running the REAL reference XPoint (xpoint.models.XPoint of the reference tree, as oracle/refharness
builds it; this tool imports the harness and does not modify it) forward over a pair and `.backward()` on the CPU, with the module cast to float64.
Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_xpoint_training.py

The case is tests/xpoint_train_f64.py's (encoder_f64 case "S": EMBED_DIM 32, DEPTHS [1, 1, 1, 1], images (2, 1, 64, 96), `mixed_precision: false`).
The reference's `forward(data)` runs forward_impl once per spectrum; the heads are in `.train()` (batch statistics), the encoder in `.eval()` (the
harness's DropPath shim is eval-only) with the widening pre-hook on every block's `op.out_norm` that tools/make_golden_encoder_training.py documents.
The scalar  sum over spectra of (sum logits R1 + sum desc R2)  is back-propagated: the heads' loss reaches the encoder through the reflection-padded
trunk convolution, which is what the file pins.  It holds
  seed                                   the input seed (the first of eight at which both spectra's trunk pre-activations meet the ReLU floor)
  logits/<spectrum>, desc/<spectrum>     the outputs (desc strided: heads_f64.GOLDEN_STRIDES)
  denc/<spectrum>                        the gradient of the encoder output, as enc_nhwc (B, H / 8, W / 8, E / 2)
  grad/<head parameter>                  every head parameter's gradient (the convolution weights strided: heads_f64.GOLDEN_STRIDES)
  grad/encoder.<name>                    the encoder gradients that make_golden_encoder_training.stored() selects; one of more than MAX_ELEMS elements is
                                         stored as its leading output channels only (a smaller cap than g33's: the committed file stays below 1 MiB)
Arrays are stored as float32.  One thread, fixed zip timestamps: a re-run is byte-identical."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle.refharness.build_ref import build_reference_xpoint  # noqa: E402
from oracle.refharness.make_golden import savez_deterministic  # noqa: E402
from make_golden_encoder_training import stored  # noqa: E402
from tests import encoder_f64 as En, heads_f64 as Hd, xpoint_train_f64 as Xp  # noqa: E402
from xpoint_amd import synth  # noqa: E402

OUT = Xp.GOLDEN
MAX_ELEMS = 1 << 15


def main():
    torch.set_num_threads(1)
    case = Xp.CASE
    cfg = Xp.model_config(case)
    net = build_reference_xpoint(cfg, synth.make_state_dict(cfg))
    net.double().train()
    enc = net.encoder.eval()
    for layer in enc.layers:
        for blk in layer.blocks:
            blk.op.out_norm.register_forward_pre_hook(lambda _module, args: (args[0].double(),))
    maps = []
    enc.register_forward_hook(lambda _module, _args, out: (out.retain_grad(), maps.append(out))[0])
    net.zero_grad()
    inputs = Xp.case_inputs(case)
    data = {sp: {"image": inputs[sp][0].double()} for sp in Xp.SPECTRA}
    pred = dict(zip(Xp.SPECTRA, net(data)[:2]))
    loss = sum((pred[sp]["logits"] * inputs[sp][1]).sum() + (pred[sp]["desc"] * inputs[sp][2]).sum() for sp in Xp.SPECTRA)
    loss.backward()
    g = {"seed": np.int64(Xp.case_seed(case))}
    assert len(maps) == 2
    for sp, x in zip(Xp.SPECTRA, maps):
        g[f"logits/{sp}"] = pred[sp]["logits"].detach().float().numpy().copy()
        g[f"desc/{sp}"] = Hd.golden_view("desc", pred[sp]["desc"].detach()).float().numpy().copy()
        g[f"denc/{sp}"] = x.grad.permute(0, 2, 3, 1).float().numpy().copy()
    n_enc = 0
    for k, p in net.named_parameters():
        if k.startswith((Hd.DET, Hd.DSC)):
            g["grad/" + k] = Hd.golden_view(k, p.grad).float().numpy().copy()
        elif k.startswith(En.PRE) and stored(k[len(En.PRE):]):
            a = p.grad.float().numpy()
            if a.size > MAX_ELEMS:
                a = a[:max(1, MAX_ELEMS // (a.size // a.shape[0]))]
            g["grad/" + k] = a.copy()
            n_enc += 1
    print(f"{case}: loss {float(loss):.6g}, {n_enc} encoder gradients, |denc| {float(maps[0].grad.abs().max()):.4g}")
    savez_deterministic(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(g)} arrays)")


if __name__ == "__main__":
    main()
