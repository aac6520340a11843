"""Inputs and plain restatements shared by tests/test_cpu_postproc_plan.py and tests/test_gpu_postproc_paths.py.

The CPU test proves, with `xp_box_nms_plan` and the restatements below, that every input of the GPU tests takes the path it is there for; the GPU
tests then compare that path with the oracle.  Nothing here calls a kernel."""
import ctypes

import numpy as np

from xpoint_amd import synth

MIN_PROB = 0.015

# (size, iou) -> reach (largest |dy|, |dx| at which two size x size boxes on integer centres overlap with IoU > iou)
REACH_TABLE = [((8.0, 0.1), 6), ((7.5, 0.1), 6), ((4.0, 0.1), 3), ((8.0, 0.5), 2), ((16.0, 0.1), 13), ((16.0, 0.001), 15), ((15.5, 0.001), 15),
               ((1.0, 0.1), 0), ((0.5, 0.1), 0)]

# shapes of the GPU tests -> (size, iou, form, reach, bands); form 0 = tile sweeps, 1 = local maxima + finisher
SWEEP, TWO_LAUNCH = 0, 1
GPU_SHAPES = {
    "A1": [((1, 32), 8.0, 0.1, TWO_LAUNCH, 6, 1), ((1, 33), 8.0, 0.1, TWO_LAUNCH, 6, 1), ((65, 33), 8.0, 0.1, TWO_LAUNCH, 6, 1),
           ((33, 64), 8.0, 0.1, TWO_LAUNCH, 6, 1)],
    "A2": [((70, 100), s, i, TWO_LAUNCH, r, 1) for (s, i), r in REACH_TABLE],
    "A4": [((96, 256), 8.0, 0.1, TWO_LAUNCH, 6, 1)],
    "A5": [((181, 2048), 8.0, 0.1, TWO_LAUNCH, 6, 2), ((181, 2048), 16.0, 0.001, TWO_LAUNCH, 15, 2)],
    "A6": [((181, 2048), 8.0, 0.1, TWO_LAUNCH, 6, 2)],
    "B1": [((200, 24), 8.0, 0.1, SWEEP, 6, None), ((200, 24), 16.0, 0.001, SWEEP, 15, None)],
    "B2": [((40, 2080), 8.0, 0.1, SWEEP, 6, None)],
}


def plan(lib, H, W, size, iou):
    """(form, reach, bands, rows per band, list_cap) of xp_box_nms for a shape and a box, from the library."""
    out = (ctypes.c_int * 5)()
    rc = lib.xp_box_nms_plan(H, W, float(size), float(iou), out)
    assert rc == 0, lib.xp_last_error().decode()
    return tuple(out)


def overlap_table(size, iou, maxr=15):
    """ovl[dy, dx] (0 <= dy, dx <= maxr): do two size x size boxes whose centres differ by (dy, dx) overlap with IoU > iou — torchvision's
    float32 arithmetic on [c - size / 2, c + size / 2], restated in numpy float32.  Returns (ovl, reach)."""
    f = np.float32
    half = f(size) * f(0.5)
    side = (f(0) + half) - (f(0) - half)
    area = side * side
    d = np.arange(maxr + 1, dtype=np.float32)
    ext = np.maximum(np.minimum(half, d + half) - np.maximum(-half, d - half), f(0)).astype(np.float32)      # 1-d intersection per offset
    inter = (ext[:, None] * ext[None, :]).astype(np.float32)
    ovr = inter / ((area + area) - inter).astype(np.float32)
    ovl = ovr > f(iou)
    idx = np.nonzero(ovl)
    reach = int(max(idx[0].max(), idx[1].max())) if len(idx[0]) else 0
    return ovl, reach


def field(name, shape, levels, scale=1.0):
    """synth.uniform in [0, 1) quantised to `levels` values (exact ties), times `scale` (a power of two keeps the ties exact)."""
    p = synth.uniform("postproc/" + name, shape, 0.0, 1.0)
    if levels:
        p = np.floor(p * levels) / levels
    return (p * scale).astype(np.float32)


def ridge(n):
    """n strictly increasing values in [0.5, 0.9): above every value of a field scaled by 0.5, so nothing but the ridge decides the ridge."""
    r = (0.5 + 0.4 * np.arange(n, dtype=np.float64) / n).astype(np.float32)
    assert np.all(np.diff(r) > 0)
    return r


def ridge_down(p, image, col0, width=4):
    """A monotone ridge down the image (highest at the bottom): each ridge pixel waits for the one below it, through every tile and band border."""
    p[image, :, col0:col0 + width] = ridge(p.shape[1])[:, None]


def ridge_along(p, image, row0, width=4):
    p[image, row0:row0 + width, :] = ridge(p.shape[2])[None, :]


def case_a5():
    """(2, 181, 2048): 256-level field below 0.5 plus a ridge down each image, at other columns in image 1."""
    p = field("a5", (2, 181, 2048), 256, 0.5)
    ridge_down(p, 0, 300)
    ridge_down(p, 1, 1501)
    return p


def case_a6():
    """(2, 181, 2048), two constant images: after round 1 every pixel but the first keeper's window is undecided, so the short last band's
    workspace list is as long as the band has pixels."""
    return np.stack([np.full((181, 2048), 0.5, np.float32), np.full((181, 2048), 0.25, np.float32)])


def case_b1():
    """(3, 200, 24): 16-level field below 0.5 plus a ridge down columns 10-13 (crosses the three tile borders at rows 64, 128, 192)."""
    p = field("b1", (3, 200, 24), 16, 0.5)
    for b in range(3):
        ridge_down(p, b, 10)
    return p


def case_b2():
    """(1, 40, 2080): 64-level field below 0.5 plus a 4-row ridge along the image (crosses the 64 tile borders in x)."""
    p = field("b2", (1, 40, 2080), 64, 0.5)
    ridge_along(p, 0, 18)
    return p


def case_a4():
    """(3, 96, 256), every pixel a candidate: a strictly increasing row-major ramp (one round-1 keeper, the LAST pixel), a constant image (one
    round-1 keeper, the FIRST pixel; a maximal tie chain) and a 4-level field (values 1/4 .. 1)."""
    H, W = 96, 256
    n = H * W
    ramp = (0.1 + 0.8 * np.arange(n, dtype=np.float64) / n).astype(np.float32)
    assert np.all(np.diff(ramp) > 0)
    four = (np.floor(synth.uniform("postproc/a4", (H, W), 0.0, 1.0) * 4) + 1) / 4
    return np.stack([ramp.reshape(H, W), np.full((H, W), 0.5, np.float32), four.astype(np.float32)])


def undecided_after_round1(p, size, iou, min_prob=MIN_PROB, rows=None):
    """Restatement of the two-launch form's first two passes on one image: the candidates (p > min_prob), minus those with nothing AHEAD of them
    in their overlap window (higher score, or the same score earlier in row-major order: the round-1 keepers), minus those a round-1 keeper
    overlaps.  Returns (candidates, keepers, undecided) as counts; with `rows`, the undecided count of each band of `rows` rows instead."""
    ovl, R = overlap_table(size, iou)
    H, W = p.shape
    cand = p > min_prob
    pad = np.full((H + 2 * R, W + 2 * R), -np.inf, np.float32)
    pad[R:R + H, R:R + W] = np.where(cand, p, -np.inf)
    offs = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if (dy or dx) and ovl[abs(dy), abs(dx)]]
    ahead = np.zeros((H, W), bool)
    for dy, dx in offs:
        q = pad[R + dy:R + dy + H, R + dx:R + dx + W]
        ahead |= (q >= p) if (dy < 0 or (dy == 0 and dx < 0)) else (q > p)
    keep = cand & ~ahead
    kpad = np.zeros((H + 2 * R, W + 2 * R), bool)
    kpad[R:R + H, R:R + W] = keep
    hit = np.zeros((H, W), bool)
    for dy, dx in offs:
        hit |= kpad[R + dy:R + dy + H, R + dx:R + dx + W]
    und = cand & ~keep & ~hit
    if rows:
        return [int(und[y:y + rows].sum()) for y in range(0, H, rows)]
    return int(cand.sum()), int(keep.sum()), int(und.sum())
