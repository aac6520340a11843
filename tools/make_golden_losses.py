"""Generate tests/golden/g27_losses.npz by running the REAL reference losses (xpoint.utils.losses.XPointLoss, imported from the reference tree
with the harness shims of oracle/refharness, which this tool imports and does not modify) forward and `.backward()` on the CPU.  Build
container only:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_losses.py

Inputs come from tests/losses_f64.py (hash RNG of xpoint_amd.synth), so the tests regenerate them; the file holds outputs and small inputs:
  desc/<case>/{loss, pos, neg, g1, g2, seed, h1, h2}   XPointLoss.descriptor_loss and d1.grad / d2.grad (strided for the large cases)
  det/<case>/{loss, dlogits, seed, c_<component>}     XPointLoss.detector_loss (gradients with a channel stride)
  fwd/<case>/{loss, seed, h1, h2, g_logits1, g_logits2, g_desc1, g_desc2, c_<component>}  the full forward (gradients with channel strides)
  noise/<seed>/<k>    the k-th torch.rand((B, 64, Hc, Wc)) after torch.manual_seed(seed): the noise the reference drew in those calls
The reference's `.cuda()` calls are shimmed to identity here and its prints are swallowed.  Conditions asserted on every stored case (the
homography / input seed is re-drawn until they hold; the seed is stored): no pair of cells within 1e-3 px of the correspondence threshold
unless the geometry is exact (none / identity / translations by multiples of 8 px), no dot product within 1e-5 of a margin wherever
gradients are stored, and the two largest entries of [3 label + noise, 2] differ in every cell.  Both conditions bound the number of pairs a case can have: with P pairs about 1e-3 P of
them fall within 1e-3 px of a threshold under a general homography and about 2e-5 P dot products within 1e-5 of a margin, so the 1 024-cell
case uses exact geometry and unit-norm descriptors, and the 1 200-cell D = 64 projective case stores its three losses but no gradients
(its gradients are pinned at 140 cells by d64_small).  One thread; fixed zip timestamps: a re-run is byte-identical.
"""
import contextlib
import copy
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.refharness import stubs  # noqa: E402
from oracle.refharness.make_golden import savez_deterministic  # noqa: E402
from tests import losses_f64 as L  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g27_losses.npz")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*a, **k)


def threshold_gap(ref_h, h1, h2, B, Hc, Wc, thr):
    """smallest | |w1_i - w2_j| - thr | over all pairs, with the reference's own warp"""
    cc = L.centres(B, Hc, Wc)
    w1 = ref_h.warp_points_pytorch(cc, h1.inverse()) if h1 is not None else cc
    w2 = ref_h.warp_points_pytorch(cc, h2.inverse()) if h2 is not None else cc
    gap = float("inf")
    for j0 in range(0, Hc * Wc, 256):
        d = (w1[:, None, :, :] - w2[:, j0:j0 + 256, None, :]).norm(dim=-1)
        gap = min(gap, float((d - thr).abs().min()))
    return gap


def noise_ok(kp, noise):
    B, H, W = kp.shape
    lab = kp.float().reshape(B, H // 8, 8, W // 8, 8).permute(0, 2, 4, 1, 3).reshape(B, 64, H // 8, W // 8)
    s = torch.cat((3.0 * lab + noise, 2.0 * torch.ones(B, 1, H // 8, W // 8)), 1)
    top = s.topk(2, dim=1).values
    return bool((top[:, 0] > top[:, 1]).all())


def main():
    torch.set_num_threads(1)
    stubs.install()
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    from xpoint.utils import homographies as ref_h
    from xpoint.utils import losses as ref_losses
    g = {}
    pristine = copy.deepcopy(ref_losses.XPointLoss.default_config)

    def make(cfg):          # the reference's dict_update writes into the class-level default_config: start every case from the original
        ref_losses.XPointLoss.default_config = copy.deepcopy(pristine)
        return quiet(ref_losses.XPointLoss, copy.deepcopy(cfg))

    for name, case in L.DESC_CASES.items():
        B, D, Hc, Wc = case[:4]
        for seed in range(64):
            d1, d2, h1, h2, m1, m2, cfg, stride = L.desc_case(name, seed)
            full = dict(cfg, detector_handle_multiple_keypoints="hard_assignment")
            crit = make(full)
            exact = case[8] != "projective"
            if not exact and threshold_gap(ref_h, h1, h2, B, Hc, Wc, cfg["descriptor_loss_threshold"]) < 1e-3:
                continue
            gp, gn = L.margin_gaps(d1, d2, crit.config["positive_margin"], crit.config["negative_margin"])
            if stride is not None and min(gp, gn) < 1e-5:
                continue
            break
        else:
            raise RuntimeError(f"{name}: no seed satisfies the conditions")
        a1, a2 = d1.clone().requires_grad_(True), d2.clone().requires_grad_(True)
        loss, pos, neg = crit.descriptor_loss(a1, a2, h1, h2, m1, m2)
        loss.backward()
        g[f"desc/{name}/seed"] = np.int64(seed)
        for k, v in (("loss", loss), ("pos", pos), ("neg", neg)):
            g[f"desc/{name}/{k}"] = v.detach().numpy()
        if stride is not None:
            sd, sh, sw = stride
            g[f"desc/{name}/g1"] = a1.grad[:, ::sd, ::sh, ::sw].numpy()
            g[f"desc/{name}/g2"] = a2.grad[:, ::sd, ::sh, ::sw].numpy()
        if h1 is not None:
            g[f"desc/{name}/h1"], g[f"desc/{name}/h2"] = h1.numpy(), h2.numpy()
        print(f"desc/{name}: seed {seed}, loss {float(loss):.6g} pos {float(pos):.6g} neg {float(neg):.6g}, margin gaps {gp:.2e} {gn:.2e}")

    for name, case in L.DET_CASES.items():
        logits, kp, m, fn, w = L.det_case(name)
        crit = make(L.det_config(fn, w))
        for seed in range(64):
            torch.manual_seed(seed)
            noise = torch.rand((case[0], 64, case[1], case[2]))
            if noise_ok(kp, noise):
                break
        x = logits.clone().requires_grad_(True)
        torch.manual_seed(seed)
        loss, comp = quiet(crit.detector_loss, crit.detector_loss_fn2, x, kp, m)
        loss.backward()
        g[f"det/{name}/seed"] = np.int64(seed)
        g[f"noise/{seed}/0"] = noise.numpy()
        g[f"det/{name}/loss"] = loss.detach().numpy()
        g[f"det/{name}/dlogits"] = x.grad[:, ::L.LOGIT_STRIDE].numpy()
        for k, v in comp.items():
            g[f"det/{name}/c_{k}"] = np.float64(float(v))
        print(f"det/{name}: seed {seed}, loss {float(loss):.6g}, " + ", ".join(f"{k} {float(v):.4g}" for k, v in comp.items()))

    Bf, _, Hf, Wf = L.FWD_SHAPE
    for name, cfg in L.FORWARD_CASES.items():
        crit = make(cfg)
        for seed in range(64):
            data, pred, pred2 = L.forward_case(name, seed)
            h1, h2 = data["optical"]["homography"], data["thermal"]["homography"]
            if threshold_gap(ref_h, h1, h2, Bf, Hf, Wf, crit.config["descriptor_loss_threshold"]) < 1e-3:
                continue
            gp, gn = L.margin_gaps(pred["desc"], pred2["desc"], crit.config["positive_margin"], crit.config["negative_margin"])
            torch.manual_seed(seed)
            n1, n2 = torch.rand((Bf, 64, Hf, Wf)), torch.rand((Bf, 64, Hf, Wf))
            if min(gp, gn) >= 1e-5 and noise_ok(data["optical"]["keypoints"], n1) and noise_ok(data["thermal"]["keypoints"], n2):
                break
        else:
            raise RuntimeError(f"fwd/{name}: no seed satisfies the conditions")
        for p in (pred, pred2):
            for k in p:
                p[k] = p[k].clone().requires_grad_(True)
        torch.manual_seed(seed)
        loss, comp = quiet(crit, {"data": data, "pred": pred, "pred2": pred2})
        loss.backward()
        g[f"fwd/{name}/seed"] = np.int64(seed)
        g[f"fwd/{name}/loss"] = loss.detach().numpy()
        g[f"fwd/{name}/h1"], g[f"fwd/{name}/h2"] = h1.numpy(), h2.numpy()
        g[f"noise/{seed}/0"], g[f"noise/{seed}/1"] = n1.numpy(), n2.numpy()
        g[f"fwd/{name}/g_logits1"], g[f"fwd/{name}/g_logits2"] = (p["logits"].grad[:, ::L.LOGIT_STRIDE].numpy() for p in (pred, pred2))
        g[f"fwd/{name}/g_desc1"], g[f"fwd/{name}/g_desc2"] = (p["desc"].grad[:, ::L.FWD_DESC_STRIDE].numpy() for p in (pred, pred2))
        for k, v in comp.items():
            g[f"fwd/{name}/c_{k}"] = np.float64(float(v))
        print(f"fwd/{name}: seed {seed}, loss {float(loss):.6g}, " + ", ".join(f"{k} {float(v):.4g}" for k, v in comp.items()))
    savez_deterministic(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(g)} arrays)")


if __name__ == "__main__":
    main()
