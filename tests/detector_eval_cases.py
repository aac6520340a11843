"""Inputs of the detector-evaluation fixture tests/golden/g28_detector_eval.npz (tools/make_golden_detector_eval.py writes it, the CPU and
GPU tests regenerate the inputs from the stored seed).  Everything comes from xpoint_amd.synth's hash RNG: exact float32, no libm.

tp/fp cases (compute_tp_fp_dist), a few thousand pixels each:
  name -> (H, W, distance_thresh, labels, candidates)
  labels:     'clusters' — groups of 3-4 labels closer together than the radius (one prediction sees several labels, several predictions
                           claim one), plus the four corners and points on every border;
              'borders'  — corners and border points only;  'few' — three labels;  'none' — zero labels
  candidates: 'dense' — about half of the pixels above zero_threshold, a tenth of the pixels straddling it (u * 2e-4);
              'all'   — every pixel a candidate (more predictions than needed to exhaust the labels);
              'one'   — exactly one candidate, next to a label;  'zero' — none
"""
import numpy as np
import torch

from xpoint_amd import synth

ZERO_THRESHOLD = 1e-4

TP_FP_CASES = {
    "clusters_24x40_t2": (24, 40, 2.0, "clusters", "dense"),
    "clusters_33x47_t2p5": (33, 47, 2.5, "clusters", "dense"),
    "clusters_33x47_t1": (33, 47, 1.0, "clusters", "dense"),
    "borders_24x40_t2": (24, 40, 2.0, "borders", "dense"),
    "exhaust_33x47_t2": (33, 47, 2.0, "few", "all"),
    "zero_labels_24x40_t2": (24, 40, 2.0, "none", "dense"),
    "one_candidate_24x40_t2": (24, 40, 2.0, "clusters", "one"),
    "zero_candidates_33x47_t2p5": (33, 47, 2.5, "clusters", "zero"),
}


def _labels(tag, H, W, kind):
    kp = np.zeros((H, W), bool)
    if kind == "none":
        return kp
    if kind == "few":
        ys = synth._hash_int(tag + "/few_y", 3, 2, H - 3); xs = synth._hash_int(tag + "/few_x", 3, 2, W - 3)
        kp[ys, xs] = True
        return kp
    kp[[0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = True                       # the corners
    nb = 6
    kp[0, synth._hash_int(tag + "/top", nb, 1, W - 2)] = True                       # every border
    kp[H - 1, synth._hash_int(tag + "/bottom", nb, 1, W - 2)] = True
    kp[synth._hash_int(tag + "/left", nb, 1, H - 2), 0] = True
    kp[synth._hash_int(tag + "/right", nb, 1, H - 2), W - 1] = True
    if kind == "clusters":
        nc = 10
        cy = synth._hash_int(tag + "/cy", nc, 1, H - 4); cx = synth._hash_int(tag + "/cx", nc, 1, W - 4)
        oy = synth._hash_int(tag + "/oy", nc * 4, 0, 1).reshape(nc, 4); ox = synth._hash_int(tag + "/ox", nc * 4, 0, 2).reshape(nc, 4)
        for c in range(nc):
            kp[cy[c] + oy[c], cx[c] + ox[c]] = True
    return kp


def _prob(tag, H, W, kind, kp, keep=0.5):
    u = synth.uniform(tag + "/u", (H, W), 0.0, 1.0)
    if kind == "zero":
        return (u * np.float32(0.5e-4)).astype(np.float32)              # all at or below zero_threshold
    if kind == "all":
        return np.maximum(u, np.float32(2e-4))
    if kind == "one":
        p = np.zeros((H, W), np.float32)
        y, x = np.argwhere(kp)[len(np.argwhere(kp)) // 2]
        p[min(y + 1, H - 1), max(x - 1, 0)] = np.float32(0.625)
        return p
    sel = synth.uniform(tag + "/sel", (H, W), 0.0, 1.0)
    p = np.where(sel < keep, u, np.float32(0.0)).astype(np.float32)
    low = sel > 0.9                                                      # a tenth of the pixels straddle the threshold
    p[low] = (u[low] * np.float32(2e-4)).astype(np.float32)
    return p


def tp_fp_case(name, seed):
    """-> prob (H, W) float32, keypoint map (H, W) bool, distance_thresh"""
    H, W, thr, lab, cand = TP_FP_CASES[name]
    tag = f"g28/{seed}/{name}"
    kp = _labels(tag, H, W, lab)
    return _prob(tag, H, W, cand, kp), kp, thr


# ---- compute_detector_metrics: three batches of two 24 x 40 images, a fake single-image net that returns the stored probabilities ----
DET_SHAPE = (3, 2, 24, 40)          # batches, batch size, H, W
DET_CONFIGS = {"nms0": {"nms": 0, "detection_threshold": 0.015}, "nms4": {"nms": 4, "detection_threshold": 0.015}}


def detector_batches(seed):
    """-> list of data dicts {'image', 'valid_mask' (B,1,H,W), 'keypoints' (B,H,W) bool} and the list of prob tensors (B,1,H,W)"""
    nb, B, H, W = DET_SHAPE
    data, probs = [], []
    for k in range(nb):
        p = np.zeros((B, 1, H, W), np.float32); kp = np.zeros((B, H, W), bool); m = np.ones((B, 1, H, W), np.float32)
        for b in range(B):
            tag = f"g28/{seed}/det/{k}/{b}"
            kp[b] = _labels(tag, H, W, "clusters" if (k + b) % 3 else "borders")
            p[b, 0] = _prob(tag, H, W, "dense", kp[b], keep=0.3)
            if (k + b) % 2:
                m[b, 0, 3:9, 5 * (k + 1):5 * (k + 1) + 12] = 0.0            # a rectangle of invalid pixels, over labels and predictions
        data.append({"image": torch.zeros(B, 1, H, W), "valid_mask": torch.from_numpy(m), "keypoints": torch.from_numpy(kp)})
        probs.append(torch.from_numpy(p))
    return data, probs


class FakeSingleNet:
    """net(data) -> {'prob': the next stored batch} (moved to the device of the data)."""

    def __init__(self, probs):
        self.probs, self.k = probs, 0

    def __call__(self, data):
        p = self.probs[self.k % len(self.probs)].to(data["image"].device)
        self.k += 1
        return {"prob": p.clone()}


# ---- compute_repeatability_multispectral: two batches of two 24 x 40 pairs, non-identity homographies, masks, empty samples ----
REP_SHAPE = (2, 2, 24, 40)
REP_CONFIG = {"prediction": {"detection_threshold": 0.015, "nms": 4, "topk": 0, "cpu_nms": True}}
REP_DISTANCE_THRESH = 3


def _homography(tag):
    u = synth.uniform(tag, (8,), -1.0, 1.0).astype(np.float64)
    h = np.array([[1.0 + 0.04 * u[0], 0.05 * u[1], 2.5 * u[2]],
                  [0.05 * u[3], 1.0 + 0.04 * u[4], 2.5 * u[5]],
                  [4e-4 * u[6], 4e-4 * u[7], 1.0]])
    return h.astype(np.float32)


def repeatability_batches(seed):
    """-> list of pair data dicts (image, valid_mask, homography per spectrum) and the list of (prob_optical, prob_thermal) batches.
    Pair 1 has no optical keypoint, pair 3 has none at all (it is skipped: no warped point)."""
    nb, B, H, W = REP_SHAPE
    data, probs = [], []
    for k in range(nb):
        d = {s: {"image": torch.zeros(B, 1, H, W)} for s in ("optical", "thermal")}
        pr = {}
        for s in ("optical", "thermal"):
            p = np.zeros((B, 1, H, W), np.float32); m = np.ones((B, 1, H, W), np.float32); hs = np.zeros((B, 3, 3), np.float32)
            for b in range(B):
                i = k * B + b
                tag = f"g28/{seed}/rep/{i}/{s}"
                u = synth.uniform(tag + "/u", (H, W), 0.02, 1.0); sel = synth.uniform(tag + "/sel", (H, W), 0.0, 1.0)
                p[b, 0] = np.where(sel < 0.12, u, u * np.float32(0.01)).astype(np.float32)          # the rest stays below the detection threshold
                if (i == 1 and s == "optical") or i == 3:
                    p[b, 0] = (u * np.float32(0.01)).astype(np.float32)
                if s == "optical":
                    m[b, 0, :, :4 + i] = 0.0                                 # invalid columns on the left
                else:
                    m[b, 0, H - 3 - i:, :] = 0.0                             # invalid rows at the bottom
                hs[b] = _homography(tag + "/h")
            d[s]["valid_mask"] = torch.from_numpy(m)
            d[s]["homography"] = torch.from_numpy(hs)
            pr[s] = torch.from_numpy(p)
        data.append(d)
        probs.append((pr["optical"], pr["thermal"]))
    return data, probs


class FakePairNet:
    """takes_pair() is True; net(data) -> ({'prob'}, {'prob'}, None) from the stored batches."""

    def __init__(self, probs):
        self.probs, self.k = probs, 0

    def takes_pair(self):
        return True

    def __call__(self, data):
        po, pt = self.probs[self.k % len(self.probs)]
        self.k += 1
        dev = data["optical"]["image"].device
        return {"prob": po.to(dev).clone()}, {"prob": pt.to(dev).clone()}, None


def all_candidate_values(seed):
    """Every probability above zero_threshold that the fixture's tp/fp and detector-metrics cases see, for the distinctness condition."""
    vals = [tp_fp_case(name, seed)[0].ravel() for name in TP_FP_CASES]
    vals += [p.numpy().ravel() for p in detector_batches(seed)[1]]
    v = np.concatenate(vals)
    return v[v > np.float32(ZERO_THRESHOLD)]
