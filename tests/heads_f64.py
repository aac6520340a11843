"""Float64 restatement of the XPoint heads in training mode (reference XPoint.py:112-138, 348-371) with torch autograd on the CPU, and the
case tables of the head-training tests.  Pinned against the real reference by tests/test_cpu_head_training.py (tests/golden/g30_head_training.npz,
written by tools/make_golden_heads.py); the GPU tests compare the HIP heads with this restatement.

Inputs come from the hash RNG of xpoint_amd.synth: the head weights are the synthetic state dicts', the encoder tensor and the two cotangents are
hash uniforms named by case and seed.  The loss of a case is  sum logits * R1 + sum desc * R2.

The gradient jumps where a trunk pre-activation is 0, so every end-to-end case must satisfy  min |pre-activation| >= RELU_FLOOR * max |pre-activation|
(the floor DESIGN.md section 11 uses for the three-product dot): `case_seed` returns the first of the first eight seeds that does, and the tests assert the
floor before anything is compared.  No element is left out of a comparison."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from xpoint_amd import synth

RELU_FLOOR = 2e-6
DET, DSC = "detector_head_convolutions.", "descriptor_head_convolutions."
SHAPES = collections.OrderedDict((("1x2x2", (1, 2, 2)), ("3x9x7", (3, 9, 7)), ("2x8x16", (2, 8, 16))))
CONFIGS = ("vmamba", "conv")          # Ci 48, D 256 (XPoint-EXP1) / Ci 128, D 64 (multipoint params)
CASES = [f"{c}/{s}" for c in CONFIGS for s in SHAPES]
# what the golden file keeps of the large tensors: [::stride] along the leading dimensions
GOLDEN_STRIDES = {"1.weight": (16, 5), "4.weight": (8, 1), "desc": (1, 4)}


def model_config(kind):
    return synth.xpoint_exp1_config(height=64, width=64) if kind == "vmamba" else synth.multipoint_config()


@functools.lru_cache(maxsize=None)
def head_state(kind):
    """The heads' slice of the synthetic state dict of the configuration, float32 torch tensors keyed by the reference's names."""
    cfg = model_config(kind)
    sd = synth.make_state_dict(cfg) if kind == "vmamba" else synth.make_conv_xpoint_state_dict(cfg)
    out = collections.OrderedDict()
    for k, v in sd.items():
        if k.startswith(DET) or k.startswith(DSC):
            out[k] = torch.from_numpy(np.array(v, copy=True))
    return out


def case_inputs(case, seed):
    """(enc (B, Ci, Hc, Wc), R1 (B, 65, Hc, Wc), R2 (B, D, Hc, Wc)) float32 CPU tensors."""
    kind, shape = case.split("/")
    B, Hc, Wc = SHAPES[shape]
    sd = head_state(kind)
    Ci, D = sd[DET + "1.weight"].shape[1], sd[DSC + "4.weight"].shape[0]
    t = lambda what, c: torch.from_numpy(synth.uniform(f"g30/{case}/{what}/{seed}", (B, c, Hc, Wc), -1.0, 1.0))
    return t("enc", Ci), t("r1", 65), t("r2", D)


def heads_f64(sd, enc, r1=None, r2=None, training=True, dtype=torch.float64):
    """The heads on the CPU in `dtype`.  Returns a dict: logits, desc, pre (the two trunks' pre-activations), and with cotangents the
    gradient of sum logits r1 + sum desc r2 per parameter name ('grad/<name>'); in training mode also the updated running statistics
    ('<name>' of every buffer)."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(k.endswith(".weight") or k.endswith(".bias")) if v.is_floating_point() else v.clone()
         for k, v in sd.items()}
    x = enc.to(dtype)
    res, pre = {}, []

    def bn(z, pfx):
        return F.batch_norm(z, p[pfx + "running_mean"], p[pfx + "running_var"], p[pfx + "weight"], p[pfx + "bias"], training, 0.1, 1e-5)

    def head(pfx):
        a = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), p[pfx + "1.weight"], p[pfx + "1.bias"])
        pre.append(a.detach())
        return bn(F.conv2d(bn(F.relu(a), pfx + "3."), p[pfx + "4.weight"], p[pfx + "4.bias"]), pfx + "5.")

    with torch.enable_grad():
        logits = head(DET)
        desc = F.normalize(head(DSC), p=2, dim=1)
        if r1 is not None:
            loss = (logits * r1.to(dtype)).sum() + (desc * r2.to(dtype)).sum()
            names = [k for k in p if torch.is_tensor(p[k]) and p[k].requires_grad]
            for k, g in zip(names, torch.autograd.grad(loss, [p[k] for k in names])):
                res["grad/" + k] = g
    res["logits"], res["desc"], res["pre"] = logits.detach(), desc.detach(), torch.cat(pre, 1)
    if training:
        for k in p:
            if "running_" in k:
                res[k] = p[k].detach()
            elif k.endswith("num_batches_tracked"):
                res[k] = p[k] + 1
    return res


def relu_margin(pre):
    """min |pre-activation| / max |pre-activation| of a case."""
    a = pre.abs()
    return float(a.min() / a.max())


@functools.lru_cache(maxsize=None)
def case_seed(case):
    """The first of the first eight seeds whose float64 pre-activations meet the floor."""
    kind = case.split("/")[0]
    for seed in range(8):
        enc, _, _ = case_inputs(case, seed)
        if relu_margin(heads_f64(head_state(kind), enc)["pre"]) >= RELU_FLOOR:
            return seed
    raise RuntimeError(f"{case}: none of the first eight seeds meets the ReLU floor")


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(seed, inputs, float64 results) of a case, computed once and shared by the tests (treat as read-only)."""
    seed = case_seed(case)
    enc, r1, r2 = case_inputs(case, seed)
    return seed, (enc, r1, r2), heads_f64(head_state(case.split("/")[0]), enc, r1, r2)


def tensor_scale(res, name):
    """The scale a comparison of tensor `name` of the result dict `res` is measured on: its largest magnitude — except for the gradients of
    `3.bias` and `4.bias`, which are ZERO in exact arithmetic (the BatchNorm behind the 1x1 layer removes any per-channel constant, so what
    either side holds is rounding noise of a sum whose terms cancel).  Those are measured on the scale of the sibling sum over the same terms:
    d(3.bias) = sum_r dh against d(3.weight) = sum_r dh xhat, d(4.bias) = sum_r dz against d(4.weight) = sum_r dz h, with xhat and h O(1)."""
    if name.startswith("grad/") and (name.endswith("3.bias") or name.endswith("4.bias")):
        name = name[:-len("bias")] + "weight"
    return float(torch.as_tensor(np.asarray(res[name])).double().abs().max())


def golden_view(name, t):
    """The part of tensor `name` the golden file stores."""
    for suffix, (s0, s1) in GOLDEN_STRIDES.items():
        if name.endswith(suffix):
            return t[::s0, ::s1]
    return t
