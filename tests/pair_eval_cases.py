"""The four xp_pair_eval_* kernels (include/xpoint_hip.h, csrc/pair_eval.hip) restated in numpy, in the arithmetic the header states, and the
cases tests/test_cpu_pair_eval.py and tests/test_gpu_pair_eval.py share.

Layout, as in the library: kp (2P, cap, 2) int32 (y, x), optical images first; counts (2P); image i < P is the optical image of pair i, image
P + i its thermal image, "the other image" of i is (i + P) % 2P.  Every float64 expression is written out operation by operation (numpy does not
contract a product and a sum into one fused operation; a matrix product through BLAS may), so the kernels, built without contraction, must give
the same bits.  Filler rows: warped 0, inframe 0, near +inf, match distance +inf."""
import numpy as np

INT64_MIN_F = -9223372036854775808.0
CORNER_FILL = 999.0


def warp(h, y, x):
    """evaluation.warp_keypoints (reference homographies.py:479-497) on separate coordinate arrays: (x, y, 1) . h^T divided by the third
    coordinate; h (9,) row-major acting on (x, y, 1).  Returns (y', x') float64."""
    h = np.asarray(h, np.float64).reshape(9)
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        u = (x * h[0] + y * h[1]) + h[2]
        v = (x * h[3] + y * h[4]) + h[5]
        w = (x * h[6] + y * h[7]) + h[8]
        return v / w, u / w


def trunc_int(v):
    """float64 -> int64 -> float64 as numpy's astype(int) does it on x86: toward zero, INT64_MIN for NaN and for what does not fit."""
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.abs(v) < 9223372036854775808.0, np.trunc(v) + 0.0, INT64_MIN_F)


def _rows(counts, cap):
    return np.minimum(np.maximum(np.asarray(counts, np.int64), 0), cap)


def warp_near(kp, counts, pairs, cap, H, W, map1, map2, truncate):
    """xp_pair_eval_warp_near: (warped (2P, cap, 2) f64, inframe (2P, cap) u8, near (2P, cap) f32)."""
    n_rows = _rows(counts, cap)
    warped = np.zeros((2 * pairs, cap, 2), np.float64)
    inframe = np.zeros((2 * pairs, cap), np.uint8)
    near = np.full((2 * pairs, cap), np.inf, np.float32)
    for img in range(2 * pairs):
        n, other = int(n_rows[img]), (img + pairs) % (2 * pairs)
        if n == 0:
            continue
        wy, wx = warp(map1[img], kp[img, :n, 0], kp[img, :n, 1])
        if truncate:
            wy, wx = trunc_int(wy), trunc_int(wx)
        if map2 is not None:
            wy, wx = warp(map2[img], wy, wx)
            if truncate:
                wy, wx = trunc_int(wy), trunc_int(wx)
        warped[img, :n, 0], warped[img, :n, 1] = wy, wx
        with np.errstate(all="ignore"):
            inframe[img, :n] = (wy >= 0) & (wx >= 0) & (wy < H) & (wx < W)
            m = int(n_rows[other])
            if m:
                b = kp[other, :m].astype(np.float32).astype(np.float64)                # kp.float(): the reference's list is float32
                d0 = (wy[:, None] - b[None, :, 0]).astype(np.float32)
                d1 = (wx[:, None] - b[None, :, 1]).astype(np.float32)
                near[img, :n] = np.sqrt((d0 * d0 + d1 * d1).min(1))
    return warped, inframe, near


def match_dist(kp, counts, warped, match_q, match_t, match_count, pairs, cap):
    """xp_pair_eval_match_dist: (2, P, cap) f32, in the order of the match list."""
    out = np.full((2, pairs, cap), np.inf, np.float32)
    for p in range(pairs):
        nm = int(_rows(match_count, cap)[p])
        if nm == 0:
            continue
        q, t = match_q[p, :nm], match_t[p, :nm]
        with np.errstate(all="ignore"):
            a = (warped[p][q] - kp[pairs + p][t].astype(np.float64)).astype(np.float32)
            b = (warped[pairs + p][t] - kp[p][q].astype(np.float64)).astype(np.float32)
            out[0, p, :nm] = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])
            out[1, p, :nm] = np.sqrt(b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1])
    return out


def count(near, inframe, counts, dist, match_count, pairs, cap, thresholds, inframe_only):
    """xp_pair_eval_count: (near_cnt (2, P, T), match_cnt (2, P, T), n_inframe (2, P)) int32."""
    T = len(thresholds)
    n_rows = _rows(counts, cap)
    near_cnt = np.zeros((2, pairs, T), np.int32); match_cnt = np.zeros((2, pairs, T), np.int32); n_in = np.zeros((2, pairs), np.int32)
    for img in range(2 * pairs):
        d, p = divmod(img, pairs)
        n = int(n_rows[img])
        inside = inframe[img, :n] != 0
        n_in[d, p] = inside.sum()
        use = inside if inframe_only else np.ones(n, bool)
        nm = int(_rows(match_count, cap)[p]) if dist is not None else 0
        for k, th in enumerate(thresholds):
            near_cnt[d, p, k] = (use & (near[img, :n] <= np.float32(th))).sum()
            if nm:
                match_cnt[d, p, k] = (dist[d, p, :nm] <= np.float32(th)).sum()
    return near_cnt, match_cnt, n_in


def corner_error(H_gt, H_est, n_inliers, match_count, pairs, H, W):
    """xp_pair_eval_corner_error (reference benchmark_evaluation.py:820-825): the reference's own point list, [H, H] included."""
    py, px = np.array([0.0, H, 0.0, H]), np.array([0.0, 0.0, W, H])
    out = np.full((pairs,), CORNER_FILL, np.float64)
    for p in range(pairs):
        if int(n_inliers[p]) == 0 or int(match_count[p]) < 4:
            continue
        gy, gx = warp(H_gt[p], py, px)
        ey, ex = warp(H_est[p], py, px)
        dy, dx = ey - gy, ex - gx
        nrm = np.sqrt(dy * dy + dx * dx)
        out[p] = (((nrm[0] + nrm[1]) + nrm[2]) + nrm[3]) / 4.0
    return out


def repeatability(kp, counts, pairs, cap, H, W, map1, map2, thresholds):
    """compute_repeatability_for_sample's numbers per pair from the restated kernels: (count (P, T), n (P,)); repeatability = count / n."""
    _, inframe, near = warp_near(kp, counts, pairs, cap, H, W, map1, map2, True)
    near_cnt, _, n_in = count(near, inframe, counts, None, None, pairs, cap, thresholds, True)
    return near_cnt[0] + near_cnt[1], n_in[0] + n_in[1]


# ------------------------------------------------------------------------------------------------ shared cases
FRAME = (24, 40)
PAD = 12345           # what the rows beyond a count hold: never read as data

IDENTITY = np.eye(3)
TRANSLATION = np.array([[1.0, 0.0, 15.0], [0.0, 1.0, -10.0], [0.0, 0.0, 1.0]])             # pushes points out on the right and at the top
PROJECTIVE = np.array([[1.04, 0.03, -1.7], [-0.02, 0.97, 2.3], [4e-4, -3e-4, 1.0]])
PAIR_MAPS = [IDENTITY, TRANSLATION, PROJECTIVE]

# name -> (cap, optical counts, thermal counts, match counts): an image with 0, with 1 and with 300 keypoints (more than one 256-lane tile of
# queries and of the staged list); match counts 0, 3 (below the 4 a homography needs) and the cap itself; "edges": every image is a query
# list and a staged list one short of the 256-point tile, exactly on it and one beyond
KERNEL_CASES = {
    "ragged": (320, [300, 0, 1], [300, 7, 0], [120, 0, 0]),
    "full": (300, [300, 300, 300], [300, 257, 256], [300, 3, 0]),
    "edges": (257, [255, 256, 257], [257, 255, 256], [255, 4, 0]),
}
THRESHOLD_LISTS = {"T1": [3], "T10": [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]}


def make_kernel_case(name):
    """dict(pairs, cap, H, W, kp, counts, match_q, match_t, match_count, maps): `maps` has, per mode, the (2P, 9) tables of the launch:
    'rep' = two truncating maps per image (m, then m^-1 seen from the other side), 'desc' = one float map (m for the optical images, its
    inverse for the thermal ones)."""
    cap, n_o, n_t, n_m = KERNEL_CASES[name]
    H, W = FRAME
    P = len(n_o)
    rng = np.random.default_rng(sum(map(ord, name)))
    counts = np.array(n_o + n_t, np.int32)
    kp = np.full((2 * P, cap, 2), PAD, np.int32)
    for img in range(2 * P):
        pix = np.sort(rng.choice(H * W, int(counts[img]), replace=False))
        kp[img, :counts[img], 0], kp[img, :counts[img], 1] = pix // W, pix % W
    mq = np.full((P, cap), -7, np.int32); mt = np.full((P, cap), 2 ** 30, np.int32)
    for p in range(P):
        mq[p, :n_m[p]] = np.sort(rng.choice(n_o[p], n_m[p], replace=False)) if n_m[p] else []
        mt[p, :n_m[p]] = rng.choice(n_t[p], n_m[p], replace=False) if n_m[p] else []
    inv = [np.linalg.inv(m) for m in PAIR_MAPS]
    flat = lambda ms: np.stack([np.asarray(m, np.float64).reshape(9) for m in ms])
    shift = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, -0.25], [0.0, 0.0, 1.0]])
    maps = {"rep": (flat([shift @ m for m in PAIR_MAPS] + [shift @ m for m in inv]), flat(PAIR_MAPS + inv)),
            "desc": (flat(PAIR_MAPS + inv), None)}
    return dict(pairs=P, cap=cap, H=H, W=W, kp=kp, counts=counts, match_q=mq, match_t=mt, match_count=np.array(n_m, np.int32), maps=maps)


def single_pair(case, p):
    """Pair p of a kernel case as a batch of one."""
    P = case["pairs"]
    sel = [p, P + p]
    maps = {k: (m1[sel], None if m2 is None else m2[sel]) for k, (m1, m2) in case["maps"].items()}
    return dict(pairs=1, cap=case["cap"], H=case["H"], W=case["W"], kp=np.ascontiguousarray(case["kp"][sel]), counts=case["counts"][sel].copy(),
                match_q=case["match_q"][p:p + 1].copy(), match_t=case["match_t"][p:p + 1].copy(), match_count=case["match_count"][p:p + 1].copy(),
                maps=maps)


def make_corner_case():
    """(H_gt, H_est, n_inliers, match_count, H, W): a model, fewer than four matches, no inliers, exactly four matches."""
    gt = np.stack([m.reshape(9) for m in (IDENTITY, TRANSLATION, PROJECTIVE, PROJECTIVE)]).astype(np.float64)
    rng = np.random.default_rng(11)
    est = gt * (1.0 + 1e-3 * rng.uniform(-1, 1, gt.shape))
    est[:, 8] = 1.0
    return gt, est, np.array([10, 4, 0, 7], np.int32), np.array([300, 3, 50, 4], np.int32), 24, 40


def eval_case_keypoints(case, thr=0.015):
    """The repeatability keypoints of synth.make_eval_case: nonzero((prob > thr) * mask) per image in the ragged layout."""
    B = case["prob_optical"].shape[0]
    lists = []
    for spec in ("optical", "thermal"):
        for b in range(B):
            sel = (case[f"prob_{spec}"][b, 0] > thr).astype(np.float32) * case[f"mask_{spec}"][b, 0]
            lists.append(np.argwhere(sel != 0).astype(np.int32))
    counts = np.array([len(v) for v in lists], np.int32)
    cap = int(counts.max())
    kp = np.full((2 * B, cap, 2), PAD, np.int32)
    for i, v in enumerate(lists):
        kp[i, :len(v)] = v
    return kp, counts, cap
