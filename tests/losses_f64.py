"""float64 restatement of the two fused training losses with ANALYTIC backward (no autograd), shared by tests/test_cpu_losses.py and
tests/test_gpu_losses.py.  The dense descriptor loss is chunked over j (cells of image 2), so it never holds more than a strip of the
pair matrix.  The correspondence decision uses the float32 coordinates it is handed, in float32, like the kernel and the reference; all
other arithmetic is float64."""
import torch


def case_inputs(name, B, D, Hc, Wc, normalise=True, scale=1.0, noisy_warp=0.0):
    """Descriptors from the hash RNG (regenerated on both sides of a fixture): d1, d2 (B, D, Hc, Wc) float32.  noisy_warp > 0 makes d2 =
    d1 + noise * noisy_warp (so that positives are not saturated)."""
    from xpoint_amd import synth
    d1 = torch.from_numpy(synth.uniform(name + "/d1", (B, D, Hc, Wc), -1.0, 1.0))
    d2 = torch.from_numpy(synth.uniform(name + "/d2", (B, D, Hc, Wc), -1.0, 1.0))
    if noisy_warp > 0:
        d2 = d1 + noisy_warp * d2
    if normalise:
        d1 = torch.nn.functional.normalize(d1, dim=1)
        d2 = torch.nn.functional.normalize(d2, dim=1)
    return (d1 * scale).contiguous(), (d2 * scale).contiguous()


def centres(B, Hc, Wc):
    y = (torch.arange(Hc, dtype=torch.float32) * 8.0 + 4.0).repeat_interleave(Wc)
    x = (torch.arange(Wc, dtype=torch.float32) * 8.0 + 4.0).repeat(Hc)
    return torch.stack((y, x), dim=-1)[None].repeat(B, 1, 1).contiguous()


def descriptor_loss64(d1, d2, w1, w2, v1, v2, thr, mp, mn, lam, grad=1.0, chunk=256, want_grads=True):
    """d1, d2 (B, D, Hc, Wc); w1, w2 (B, HW, 2) float32 or None; v1, v2 (B, HW) or None.  Returns dict(loss, pos, neg, sums (B, 3), norm (B),
    g1, g2) in float64; g = d(grad * loss)/dd."""
    B, D, Hc, Wc = d1.shape
    HW = Hc * Wc
    dev = d1.device
    a1 = d1.detach().double().reshape(B, D, HW)
    a2 = d2.detach().double().reshape(B, D, HW)
    w1 = centres(B, Hc, Wc).to(dev) if w1 is None else w1.float()
    w2 = centres(B, Hc, Wc).to(dev) if w2 is None else w2.float()
    v1 = torch.ones(B, HW, dtype=torch.float64, device=dev) if v1 is None else v1.double()
    v2 = torch.ones(B, HW, dtype=torch.float64, device=dev) if v2 is None else v2.double()
    norm = v2.sum(1) * v1.sum(1)
    cb = float(grad) / (B * norm)
    sums = torch.zeros(B, 3, dtype=torch.float64, device=dev)
    g1 = torch.zeros_like(a1)
    g2 = torch.zeros_like(a2)
    thr32 = torch.tensor(thr, dtype=torch.float32, device=dev)
    for j0 in range(0, HW, chunk):
        j1 = min(HW, j0 + chunk)
        dy = w1[:, None, :, 0] - w2[:, j0:j1, None, 0]
        dx = w1[:, None, :, 1] - w2[:, j0:j1, None, 1]
        s = ((dy * dy + dx * dx).sqrt() <= thr32).double()                       # (B, jc, HW), float32 decision
        dot = torch.einsum('bkj,bki->bji', a2[:, :, j0:j1], a1)
        v = v2[:, j0:j1, None] * v1[:, None, :]
        pos = lam * s * (mp - dot).clamp(min=0) * v
        neg = (1 - s) * (dot - mn).clamp(min=0) * v
        sums[:, 1] += pos.sum((1, 2))
        sums[:, 2] += neg.sum((1, 2))
        if want_grads:
            g = cb[:, None, None] * v * (-lam * s * (dot < mp).double() + (1 - s) * (dot > mn).double())
            g1 += torch.einsum('bkj,bji->bki', a2[:, :, j0:j1], g)
            g2[:, :, j0:j1] = torch.einsum('bki,bji->bkj', a1, g)
    sums[:, 0] = sums[:, 1] + sums[:, 2]
    per = sums / norm[:, None]
    return {"loss": per[:, 0].mean(), "pos": per[:, 1].mean(), "neg": per[:, 2].mean(), "sums": sums, "norm": norm,
            "g1": g1.reshape(B, D, Hc, Wc), "g2": g2.reshape(B, D, Hc, Wc)}


def margin_gaps(d1, d2, mp, mn, chunk=256):
    """smallest |dot - mp| and |dot - mn| over all pairs (float64): the gradient jumps there"""
    B, D, Hc, Wc = d1.shape
    a1 = d1.double().reshape(B, D, -1)
    a2 = d2.double().reshape(B, D, -1)
    gp = gn = float("inf")
    for j0 in range(0, a2.shape[2], chunk):
        dot = torch.einsum('bkj,bki->bji', a2[:, :, j0:j0 + chunk], a1)
        gp = min(gp, float((dot - mp).abs().min()))
        gn = min(gn, float((dot - mn).abs().min()))
    return gp, gn


def threshold_gap(w1, w2, thr):
    """smallest | |w1_i - w2_j| - thr | over all pairs of all samples, in float32 like the correspondence decision: a pair closer to the
    threshold than the arithmetic of the two sides resolves may correspond on one side only"""
    w1, w2 = w1.float(), w2.float()
    dy = w1[:, None, :, 0] - w2[:, :, None, 0]
    dx = w1[:, None, :, 1] - w2[:, :, None, 1]
    return float(((dy * dy + dx * dx).sqrt() - torch.tensor(thr, dtype=torch.float32, device=w1.device)).abs().min())


def geometry(B, Hc, Wc, seed):
    """float32 coordinates and 0/1 cell masks handed to both sides (host tensors): cell centres moved by a smooth field of a few pixels"""
    c = centres(B, Hc, Wc)
    gen = torch.Generator().manual_seed(seed)
    w1 = c + 3.0 * torch.rand(B, 1, 2, generator=gen) + 0.01 * c.flip(-1)
    w2 = c - 2.0 * torch.rand(B, 1, 2, generator=gen) + 0.02 * c
    v1 = (torch.rand(B, Hc * Wc, generator=gen) > 0.2).float()
    v2 = (torch.rand(B, Hc * Wc, generator=gen) > 0.1).float()
    return w1, w2, v1, v2


def hard_labels(keypoint_map, noise):
    """(B, Hc, Wc) int64: argmax over [3 label + noise, 2.0], first maximum; float32 arithmetic like the reference"""
    B, H, W = keypoint_map.shape
    Hc, Wc = H // 8, W // 8
    lab = keypoint_map.float().reshape(B, Hc, 8, Wc, 8).permute(0, 2, 4, 1, 3).reshape(B, 64, Hc, Wc)
    s = 3.0 * lab + noise.float()
    s = torch.cat((s, 2.0 * torch.ones(B, 1, Hc, Wc, dtype=torch.float32, device=s.device)), dim=1)
    return torch.argmax(s, dim=1)


def block_valid(valid_mask, B, Hc, Wc, device):
    if valid_mask is None:
        return torch.ones(B, Hc, Wc, dtype=torch.float64, device=device)
    return valid_mask.double().reshape(B, Hc, 8, Wc, 8).permute(0, 1, 3, 2, 4).reshape(B, Hc, Wc, 64).prod(-1)


def detector_loss64(logits, keypoint_map, valid_mask, noise, kind, wdust=1.0, alpha=0.25, gamma=2.0, grad=1.0):
    """Returns dict(loss, total (B), nvalid (B), counts (5,) = correct, TP, FP, FN, TN, detector_loss, dlogits), float64."""
    B, C, Hc, Wc = logits.shape
    x = logits.detach().double()
    label = hard_labels(keypoint_map, noise)
    valid = block_valid(valid_mask, B, Hc, Wc, x.device)
    logp = torch.log_softmax(x, dim=1)
    p = logp.exp()
    onehot = torch.zeros_like(x).scatter_(1, label[:, None], 1.0)
    # ce = log(1 + sum_{c != label} exp(x_c - x_label)): the same number as -logp[label], but it keeps its digits where the label's
    # logit dominates (there 1 + 1e-23 rounds to 1 even in float64, and q = 0 makes q^(gamma - 1) infinite for gamma < 1)
    xl = x.gather(1, label[:, None])
    ce = torch.log1p(((x - xl).exp() * (1 - onehot)).sum(1))
    if kind == 0:
        wy = torch.where(label == 64, torch.tensor(float(wdust), dtype=torch.float64, device=x.device), torch.tensor(1.0, dtype=torch.float64, device=x.device))
        lv, dce = wy * ce, wy
    else:
        pt = torch.exp(-ce)
        q = -torch.expm1(-ce)
        lv = alpha * q ** gamma * ce
        dce = alpha * (gamma * q ** (gamma - 1) * pt * ce + q ** gamma)
    total = (lv * valid).sum((1, 2))
    nvalid = valid.sum((1, 2))
    den = nvalid.clamp(min=1.0)
    loss = (total / den).mean()
    coef = float(grad) / (B * den)
    dlogits = (coef[:, None, None] * valid * dce)[:, None] * (p - onehot)
    lm = label.double() * valid
    pred = torch.argmax(torch.softmax(logits.detach().float(), dim=1), dim=1).double()
    counts = torch.stack([(pred == lm).sum(), ((pred <= 63) & (lm <= 63)).sum(), ((pred <= 63) & (lm == 64)).sum(),
                          ((pred == 64) & (lm <= 63)).sum(), ((pred == 64) & (lm == 64)).sum()]).double()
    return {"loss": loss, "total": total, "nvalid": nvalid, "counts": counts, "detector_loss": (lv * valid).mean(), "dlogits": dlogits,
            "labels": label}


# ---- the cases of tests/golden/g27_losses.npz (tools/make_golden_losses.py); inputs are regenerated on both sides ----
# name: (B, D, Hc, Wc, normalise, scale, noisy_warp, threshold, homography kind, masks, use_mask, gradient stride (D, Hc, Wc) or None = no gradients)
DESC_CASES = {
    "unit_none":      (2, 256, 8, 12, True, 1.0, 0.5, 8.0, "none", False, True, (8, 1, 1)),
    "raw_translate":  (2, 256, 8, 12, False, 0.3, 0.0, 4.0, "translate", True, True, (8, 1, 1)),
    "raw_identity":   (2, 256, 8, 12, False, 0.3, 0.6, 8.0, "identity", True, True, (8, 1, 1)),
    "raw_projective": (2, 256, 8, 12, False, 0.3, 0.6, 8.0, "projective", True, True, (8, 1, 1)),
    "unit_large":     (2, 256, 32, 32, True, 1.0, 0.6, 8.0, "translate", True, True, (8, 2, 2)),
    "d64_projective": (1, 64, 30, 40, True, 1.0, 0.7, 4.0, "projective", False, False, None),       # losses only, see the tool
    "d64_small":      (1, 64, 10, 14, True, 1.0, 0.7, 4.0, "projective", True, True, (2, 1, 1)),
    "unit_nomask":    (2, 256, 8, 12, True, 1.0, 0.8, 4.0, "translate", True, False, (8, 1, 1)),
}


def case_masks(B, Hc, Wc):
    """(B, 1, 8Hc, 8Wc) bool masks with invalid regions on both sides (a frame and a rectangle, different per image and sample)"""
    H, W = Hc * 8, Wc * 8
    m1 = torch.ones(B, 1, H, W, dtype=torch.bool)
    m2 = torch.ones(B, 1, H, W, dtype=torch.bool)
    for b in range(B):
        m1[b, :, :5 + 3 * b, :] = False
        m1[b, :, H // 2:H // 2 + 9, W // 3:W // 3 + 11 + b] = False
        m2[b, :, :, W - 7 - 2 * b:] = False
        m2[b, :, H // 4:H // 4 + 3, :W // 2] = False
    return m1, m2


def case_homographies(kind, name, seed, B, Hc, Wc):
    """(h1, h2) float32 (B, 3, 3) or (None, None).  translate: multiples of 8 px (exact geometry, pairs exactly at the threshold)."""
    from xpoint_amd import synth
    if kind == "none":
        return None, None
    eye = torch.eye(3).repeat(B, 1, 1)
    if kind == "identity":
        return eye.clone(), eye.clone()
    if kind == "translate":
        h1, h2 = eye.clone(), eye.clone()
        for b in range(B):
            h1[b, 0, 2], h1[b, 1, 2] = 8.0 * (b + 1), -8.0
            h2[b, 0, 2], h2[b, 1, 2] = -16.0, 8.0 * b
        return h1, h2
    r = torch.from_numpy(synth.uniform(f"{name}/hom/{seed}", (2, B, 8), -1.0, 1.0))
    hs = []
    for k in range(2):
        h = eye.clone()
        h[:, 0, 0] += 0.08 * r[k, :, 0]; h[:, 0, 1] = 0.06 * r[k, :, 1]; h[:, 0, 2] = 9.0 * r[k, :, 2]
        h[:, 1, 0] = 0.06 * r[k, :, 3]; h[:, 1, 1] += 0.08 * r[k, :, 4]; h[:, 1, 2] = 9.0 * r[k, :, 5]
        h[:, 2, 0] = 1.5e-4 * r[k, :, 6]; h[:, 2, 1] = 1.5e-4 * r[k, :, 7]
        hs.append(h)
    return hs[0], hs[1]


def desc_case(name, seed):
    B, D, Hc, Wc, normalise, scale, noisy, thr, hkind, masks, use_mask, stride = DESC_CASES[name]
    d1, d2 = case_inputs(f"g27/{name}/{seed}", B, D, Hc, Wc, normalise, scale, noisy)
    h1, h2 = case_homographies(hkind, f"g27/{name}", seed, B, Hc, Wc)
    m1, m2 = case_masks(B, Hc, Wc) if masks else (None, None)
    cfg = {"descriptor_loss_threshold": thr, "descriptor_loss_use_mask": use_mask}
    return d1, d2, h1, h2, m1, m2, cfg, stride


# name: (B, Hc, Wc, loss function, dustbin weight, masks)
DET_CASES = {
    "ce_w1":      (2, 11, 12, "cross_entropy", 1.0, True),
    "ce_w05":     (2, 11, 12, "cross_entropy", 0.5, True),
    "focal":      (2, 11, 12, "focal_loss", 1.0, True),
    "focal_open": (2, 11, 12, "focal_loss", 1.0, False),
}


def det_inputs(tag, B, Hc, Wc, masks):
    """logits (B, 65, Hc, Wc) float32, keypoint map (B, H, W) bool (several keypoints in some cells, none in most), mask (B, 1, H, W) or None;
    the hash RNG names are tag + /logits, /kp, /cells"""
    from xpoint_amd import synth
    logits = torch.from_numpy(synth.uniform(f"{tag}/logits", (B, 65, Hc, Wc), -4.0, 4.0))
    u = torch.from_numpy(synth.uniform(f"{tag}/kp", (B, Hc * 8, Wc * 8), 0.0, 1.0))
    cells = torch.from_numpy(synth.uniform(f"{tag}/cells", (B, Hc, Wc), 0.0, 1.0))
    dense = (cells < 0.12).repeat_interleave(8, 1).repeat_interleave(8, 2)           # a few cells with several keypoints
    kp = (u < 0.004) | (dense & (u < 0.06))
    # make the logits agree with the labels in part of the image so that TP / TN are not empty
    logits[:, 64, : Hc // 2] += 5.0
    m = case_masks(B, Hc, Wc)[0] if masks else None
    return logits, kp, m


def det_case(name):
    """the fixture's case `name`: det_inputs at its shape, + loss function and dustbin weight"""
    B, Hc, Wc, fn, w, masks = DET_CASES[name]
    return det_inputs(f"g27/det/{name}", B, Hc, Wc, masks) + (fn, w)


def det_config(fn, w):
    return {"detector_loss_function": fn, "detector_handle_multiple_keypoints": "hard_assignment", "detector_dustbin_loss_weight": w}


# full forward(loss_input_dict) cases: cmt.yaml's loss section and the class defaults + hard_assignment
CMT_LOSS = {"detector_loss": True, "descriptor_loss": True, "descriptor_loss_threshold": 4.0, "descriptor_loss_use_mask": True,
            "sparse_descriptor_loss": False, "sparse_descriptor_loss_num_cell_divisor": 64, "positive_margin": 1.0, "negative_margin": 0.2,
            "lambda_d": 250, "lambda": 1.0, "use_encoder_similarity": False, "homography_regression_loss": {"check": False, "gamma": 1.0},
            "detector_loss_function": "cross_entropy", "detector_handle_multiple_keypoints": "hard_assignment",
            "detector_dustbin_loss_weight": 1, "detector_focal_loss": {"use": False, "alpha": 0.25, "gamma": 2.0}}
FWD_SHAPE = (2, 256, 11, 12)
LOGIT_STRIDE = 4          # channel stride of the stored logits gradients
FWD_DESC_STRIDE = 16      # channel stride of the stored descriptor gradients of the forward cases
FORWARD_CASES = {"cmt": CMT_LOSS, "defaults": {"detector_handle_multiple_keypoints": "hard_assignment"}}


def forward_case(name, seed):
    """loss_input_dict pieces at B = 2, D = 256, 11 x 12 cells: data (optical, thermal: keypoints, valid_mask, homography), pred, pred2"""
    B, D, Hc, Wc = FWD_SHAPE
    d1, d2 = case_inputs(f"g27/fwd/{name}/{seed}", B, D, Hc, Wc, True, 1.0, 0.6)
    h1, h2 = case_homographies("projective", f"g27/fwd/{name}", seed, B, Hc, Wc)
    m1, m2 = case_masks(B, Hc, Wc)
    l1, k1, _, _, _ = det_case("ce_w1")
    l2, k2, _, _, _ = det_case("focal")
    data = {"optical": {"keypoints": k1, "valid_mask": m1, "homography": h1}, "thermal": {"keypoints": k2, "valid_mask": m2, "homography": h2}}
    return data, {"logits": l1, "desc": d1}, {"logits": l2, "desc": d2}


# ---- the edge cases of tests/test_gpu_losses_edges.py; tests/test_cpu_losses.py asserts their preconditions without a GPU ----
# (B, D, Hc, Wc) rows run through test_gpu_losses._check_vs_64, which names its inputs gpu64/B_D_Hc_Wc and uses geometry(..., 7),
# threshold 8, margins 1.0 / 0.2: every multiple of 16 with a path of its own (dead k of the convert, the dead half of a k-major
# 32-block, the k < D guard; KS = 12 at 144, 176, 192), and HW = 1, 5, 32, 33, 128, 129, 133, 256, 385
EDGE_ROWS = [(2, 16, 8, 12), (2, 32, 8, 12), (2, 48, 8, 12), (1, 80, 8, 12), (1, 96, 8, 12), (1, 144, 8, 12), (2, 192, 8, 12), (1, 208, 8, 12),
             (1, 240, 8, 12), (2, 64, 1, 1), (1, 64, 1, 5), (1, 256, 4, 8), (1, 64, 3, 11), (1, 128, 8, 16), (1, 64, 3, 43), (1, 176, 7, 19),
             (2, 192, 16, 16), (1, 64, 5, 77)]
EDGE_NEED_ROW = (1, 48, 3, 43)                  # one gradient only, D = 48 at HW = 129
MARGIN_FLOOR = 2e-6       # x scale^2: four times the 2^-21 that the three-product split-fp16 dot of two unit vectors is good to
THRESHOLD_FLOOR = 1e-4    # px: what xpoint_amd/losses.py documents for its inverse
SMALL, MIXED = 2.0 ** -10 * 1.37, 2.0 ** -7 * 1.1


def row_key(shape):
    return "row/" + "x".join(map(str, shape))


def _edge_case(shape, name=None, scales=None, geom="warp", thr=8.0, masks="01"):
    B, D, Hc, Wc = shape
    return {"shape": shape, "name": name or f"gpu64/{B}_{D}_{Hc}_{Wc}", "scales": scales or (1.0,) * B, "geom": geom, "thr": thr, "masks": masks}


# key: shape, the input name string (= the seed; a case that misses a floor gets another one, never a looser floor), the factor on each
# sample's unit descriptors (0 = an all-zero sample), "warp" = geometry(..., 7) or "centres" = None for w and v (the kernel's own
# centres; threshold 12, as the centres lie exactly 8 px apart), "01" masks of geometry() or "quarter" masks with values in {0, .25, .5, 1}
EDGE_DESC_CASES = {row_key(s): _edge_case(s) for s in EDGE_ROWS + [EDGE_NEED_ROW]}
EDGE_DESC_CASES.update({
    "centres/2x64x1x1": _edge_case((2, 64, 1, 1), geom="centres", thr=12.0),
    "centres/1x64x1x5": _edge_case((1, 64, 1, 5), geom="centres", thr=12.0),
})
for _D in (64, 192):
    EDGE_DESC_CASES.update({
        f"small/{_D}": _edge_case((2, _D, 8, 12), f"edge/small/{_D}/0", (SMALL, SMALL)),
        # at these scales a near-orthogonal pair (|dot| of the unit vectors ~ 1e-4 .. 1e-9) sits at a margin: D = 192 missed the floor with
        # the names /0 .. /4 (x37) and /0 (x3e4) and moved on to the next name
        f"x37/{_D}": _edge_case((2, _D, 8, 12), f"edge/x37/{_D}/{0 if _D == 64 else 5}", (37.0, 37.0)),
        f"x3e4/{_D}": _edge_case((2, _D, 8, 12), f"edge/x3e4/{_D}/{0 if _D == 64 else 1}", (3.0e4, 3.0e4)),
        f"mixed/{_D}": _edge_case((2, _D, 8, 12), f"edge/mixed/{_D}/0", (1.0, MIXED)),
        f"zero/{_D}": _edge_case((2, _D, 8, 12), f"edge/zero/{_D}/0", (1.0, 0.0)),
        f"quarter/{_D}": _edge_case((2, _D, 8, 12), f"edge/quarter/{_D}/0", masks="quarter"),
    })


def edge_desc_inputs(key):
    """host tensors of one case: d1, d2 (unit descriptors times the sample's factor), w1, w2, v1, v2 (None for "centres"), threshold"""
    c = EDGE_DESC_CASES[key]
    B, D, Hc, Wc = c["shape"]
    d1, d2 = case_inputs(c["name"], B, D, Hc, Wc, True, 1.0, 0.6)
    f = torch.tensor(c["scales"], dtype=torch.float32).reshape(B, 1, 1, 1)
    d1, d2 = (d1 * f).contiguous(), (d2 * f).contiguous()
    if c["geom"] == "centres":
        return d1, d2, None, None, None, None, c["thr"]
    w1, w2, v1, v2 = geometry(B, Hc, Wc, 7)
    if c["masks"] == "quarter":
        gen = torch.Generator().manual_seed(11)
        v1, v2 = (torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (B, Hc * Wc), generator=gen)] for _ in range(2))
    return d1, d2, w1, w2, v1, v2, c["thr"]


def edge_desc_gaps(key, mp=1.0, mn=0.2):
    """(smallest margin gap / scale^2 over the samples, threshold gap in px) of one case; an all-zero sample counts with scale 1 (the
    kernel's S = 1 branch; its dots are 0, so its gaps are the margins themselves)"""
    c = EDGE_DESC_CASES[key]
    B, D, Hc, Wc = c["shape"]
    d1, d2, w1, w2, _, _, thr = edge_desc_inputs(key)
    worst = float("inf")
    for b in range(B):
        sc = c["scales"][b] or 1.0
        worst = min(worst, min(margin_gaps(d1[b:b + 1], d2[b:b + 1], mp, mn)) / (sc * sc))
    if w1 is None:
        w1 = w2 = centres(B, Hc, Wc)
    return worst, threshold_gap(w1, w2, thr)


def assert_edge_preconditions(key):
    """a case is a fair test only if no pair sits closer to a jump of the gradient than the kernel's arithmetic can resolve"""
    gap, tgap = edge_desc_gaps(key)
    assert gap >= MARGIN_FLOOR, (key, "margin gap / scale^2", gap)
    assert tgap >= THRESHOLD_FLOOR, (key, "threshold gap", tgap)
    return gap, tgap


# ---- detector edge cases: (B, Hc, Wc) of the shape runs, and the saturated / tied tensors at (2, 16, 17) ----
EDGE_DET_SHAPES = [(1, 1, 1), (3, 16, 17), (2, 9, 57), (5, 4, 4)]
EDGE_DET_FOCAL = [(0.25, 2.0), (0.25, 0.0), (0.5, 1.0), (0.25, 0.5), (1.0, 5.0)]


def det_noise(B, Hc, Wc, seed):
    return torch.rand(B, 64, Hc, Wc, generator=torch.Generator().manual_seed(seed))


def det_saturated():
    """(2, 16, 17): the uniform [-4, 4] draw of det_inputs with four rows of 64 consecutive cells (a whole wave each) overwritten in both
    samples: cells 0..63 the label's logit +60 (ce ~ 0, pt -> 1, q -> 0), 64..127 the logit after the label's +60 (ce ~ 60, pt -> 0),
    128..191 all 65 logits equal (the prediction is class 0), 192..255 equal maxima at classes 7 and 64 (the prediction is 7); cells
    256..271 keep the draw.  Returns logits, keypoint map, mask, noise, labels."""
    B, Hc, Wc = 2, 16, 17
    logits, kp, m = det_inputs("edge/det/saturated", B, Hc, Wc, True)
    noise = det_noise(B, Hc, Wc, 5)
    label = hard_labels(kp, noise).reshape(B, -1)
    x = logits.reshape(B, 65, -1)
    n = torch.arange(64)
    for b in range(B):
        x[b, label[b, n], n] = 60.0
        x[b, (label[b, 64 + n] + 1) % 65, 64 + n] = 60.0
        x[b, :, 128:192] = 1.5
        x[b, 7, 192:256] = 9.0
        x[b, 64, 192:256] = 9.0
    return x.reshape(B, 65, Hc, Wc).contiguous(), kp, m, noise, label.reshape(B, Hc, Wc)


def det_label_ties():
    """(2, 16, 17) keypoint map and noise for the label's ties: noise 0 everywhere, so several keypoints of a cell tie at 3.0 and the
    first in channel order wins, and a cell without one has 0 < 2: label 64.  Sample 1: cell (2, 3) noise exactly 2.0 in channel 5 and no
    keypoint (2.0 > 2.0 is false: label 5, as argmax over [s, 2.0] gives), cell (2, 4) the float32 below 2.0 there (label 64)."""
    B, Hc, Wc = 2, 16, 17
    _, kp, _ = det_inputs("edge/det/ties", B, Hc, Wc, False)
    kp[0, 8:16, 8:16] = False
    kp[0, 8 + 2, 8 + 5] = kp[0, 8 + 2, 8 + 7] = kp[0, 8 + 6, 8 + 1] = True        # cell (1, 1) of sample 0: channels 21, 23, 49 -> 21
    kp[1, 16:24, 24:40] = False
    noise = torch.zeros(B, 64, Hc, Wc)
    noise[1, 5, 2, 3] = 2.0
    noise[1, 5, 2, 4] = 1.9999999
    return kp, noise
