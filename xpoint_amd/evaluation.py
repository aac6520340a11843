"""Evaluation-harness metrics on the MI355X path — SURVEY.md §8(f) rank 1.

Mirrors the reference's `xpoint/utils/benchmark_evaluation.py` (same function names, arguments and return
structures, including its per-sample overwrite quirks, see below) and `xpoint/utils/homographies.py:479-526`
(`warp_keypoints`, `filter_points`):

  compute_repeatability_for_sample   benchmark_evaluation.py:396-467
  compute_descriptor_for_sample      benchmark_evaluation.py:588-751   (NN-mAP inputs, M-score)
  compute_mAP / compute_desc_dict    benchmark_evaluation.py:469-558
  compute_pts_dist_for_sample        benchmark_evaluation.py:755-830   (corner error of the estimated homography;
  compute_homography_dict            benchmark_evaluation.py:560-586    the estimator is utils.find_homography, the
                                                                        device stand-in for cv2.findHomography MAGSAC:
                                                                        same contract, not bit-comparable — §8(f) rank 2)
  compute_metrics                    benchmark_evaluation.py:832-963

and the detector half of `xpoint/utils/evaluation.py` (what `predict_keypoints.py -e` runs):

  compute_tp_fp_dist                 evaluation.py:57-97    (tp / fp against keypoint labels; tp_fp_dist_batched is the device form)
  compute_detector_metrics           evaluation.py:10-55    (precision / recall over a data set)
  compute_repeatability_multispectral evaluation.py:105-204

Device work goes through the C ABI: keypoints and descriptors stay on the GPU, descriptor sampling is
`xp_sample_descriptors`, both match directions come from ONE `xp_match_mnn` call (mutual nearest neighbours are
the same pairs seen from either side), and the N x M "distance to the nearest keypoint" matrices of the reference
(`np.linalg.norm(warped[:, None] - kp[None])`, `torch.norm(dist.float(), dim=-1) <= th`) are never materialised:
`xp_points_min_dist` returns the per-row minimum, which is all the metrics use.  The per-match bookkeeping (tp lists,
sorting, precision / recall) is host numpy on a few thousand numbers, exactly as in the reference.

The batched device form of the same metrics: pair_metrics_batched (one batch: keypoints, descriptors, ONE matcher call,
the xp_pair_eval_* kernels, one batched homography estimate per RANSAC threshold, nothing read back when the list capacity is known) and
compute_metrics_batched (compute_metrics' signature and return structure; `reference_quirks` chooses between the reference's per-sample
overwrites and every sample counting).  `cli benchmark` and training.fit's validation metrics run on it.

What each reference function consists of here (every piece below is written once):
  compute_repeatability_for_sample      _repeatability_samples (keypoints, counts, warped + filtered sets, nearest distances) + the per-threshold dict
  compute_repeatability_multispectral   _batch_preamble + _repeatability_samples + its own list, print and nan mean
  compute_descriptor_for_sample         _check_matcher + _descriptor_samples (keypoints, sampled descriptors, mutual matches) + _descriptor_bookkeeping
  compute_pts_dist_for_sample           _descriptor_samples + _pts_dist_bookkeeping
  compute_metrics                       _batch_preamble, then per batch ONE _descriptor_samples for both bookkeeping halves; _MetricsAccumulator
  compute_metrics_batched               _batch_preamble + pair_metrics_batched; the same _MetricsAccumulator
  compute_desc_dict / compute_detector_metrics   _pr_envelope with div0 / _div0_one
  every 3 x 3 matrix of a sample        _sample_matrices (the per-sample functions and pair_eval_matrices: equal bits on both paths by construction)

Reference behaviour kept on purpose (the goldens in tests/golden/g13 come from the reference's own code):
  * inside a batch the repeatability dict and the `n_gt_*` counts are OVERWRITTEN per sample, so they hold the last
    sample's value (benchmark_evaluation.py:447-461, 662-663) — which is why the reference's NN-mAP can exceed 1;
  * `warp_keypoints(..., return_type=int)` truncates toward zero (`astype(int)`);
  * the repeatability keypoints use `prob > thr` times the valid mask, the descriptor metrics use `prob > thr` of the
    already masked heat map.
"""
from __future__ import annotations

import collections
import ctypes

import numpy as np
import torch

from . import _lib, utils
from ._lib import ptr


def div0(a, b):
    """reference utils.div0: a / b with 0 where b == 0."""
    with np.errstate(divide='ignore', invalid='ignore'):
        c = np.true_divide(a, b)
        c[~np.isfinite(c)] = 0
    return c


def warp_keypoints(keypoints, homography, return_type=int):
    """homographies.py:479-497.  keypoints (N,2) as (y, x); homography 3x3 acting on (x, y, 1) — the projective map of
    cv2.perspectiveTransform evaluated in float64."""
    keypoints = np.asarray(keypoints)
    if len(keypoints) == 0:
        return keypoints
    h = np.asarray(homography, dtype=np.float64)
    xy = keypoints[:, ::-1].astype(np.float64)
    hom = np.concatenate([xy, np.ones((xy.shape[0], 1))], 1) @ h.T
    out = hom[:, :2] / hom[:, 2:3]
    return out[:, ::-1].astype(return_type)


def filter_points(points, shape):
    """homographies.py:511-526."""
    points = points[points[:, 0] >= 0]
    points = points[points[:, 1] >= 0]
    points = points[points[:, 0] < shape[0]]
    points = points[points[:, 1] < shape[1]]
    return points


def _min_dist(a_np, b_dev_f32):
    """min_j |a_i - b_j| on the device; a: host array (N,2) (int or float), b: device float32 (M,2).  Returns numpy f32."""
    na, nb = int(a_np.shape[0]), int(b_dev_f32.shape[0])
    if na == 0:
        return np.zeros((0,), np.float32)
    a = torch.from_numpy(np.ascontiguousarray(a_np, dtype=np.float64)).to(b_dev_f32.device)
    out = torch.empty((na,), dtype=torch.float32, device=b_dev_f32.device)
    b = b_dev_f32.contiguous()
    _lib.call("xp_points_min_dist", ptr(a), na, ptr(b) if nb else None, nb, ptr(out), _lib.current_stream())
    return out.cpu().numpy()


def _as_list(x):
    return x if type(x) is list else [x]


def _check_matcher(config):
    m = config['prediction']['matching']
    if m['method'] != 'bfmatcher' or m.get('knn_matches', False) or not m.get('method_kwargs', {}).get('crossCheck', False):
        raise NotImplementedError("xpoint_amd.evaluation: the device matcher implements bfmatcher + crossCheck (the reference's configured mode)")


SampleMatrices = collections.namedtuple("SampleMatrices", "h_o h_t h_o_inv h_t_inv gt gt_inv")


def _sample_matrices(h_o, h_t):
    """The 3 x 3 matrices of ONE sample as float32 numpy, computed on the host as the reference does: the float32 cast, torch .inverse() of
    the float32 matrices, gt = h_t @ h_o.inverse() (optical -> thermal) and its inverse.  The only place they are computed: a batched or
    device inverse would have other bits."""
    h_o, h_t = h_o.reshape(3, 3).float().cpu(), h_t.reshape(3, 3).float().cpu()
    h_o_inv = h_o.inverse()
    gt = torch.mm(h_t, h_o_inv)
    return SampleMatrices(*(m.numpy() for m in (h_o, h_t, h_o_inv, h_t.inverse(), gt, gt.inverse())))


def _default_homographies(data):
    """Identity homographies (host, float32, (B, 3, 3)) where a batch has none, added to `data` as the reference does."""
    B = data['optical']['image'].shape[0]
    for spec in ('optical', 'thermal'):
        if 'homography' not in data[spec]:
            data[spec]['homography'] = torch.eye(3, dtype=torch.float32).repeat(B, 1, 1)


def _forward_pair(net, data):
    if not net.takes_pair():
        return net(data['optical']), net(data['thermal'])
    out_optical, out_thermal, _ = net(data)
    return out_optical, out_thermal


def _batch_preamble(net, data, device):
    """What every data-set loop does first: (data on the device, host H_optical, host H_thermal, out_optical, out_thermal)."""
    _default_homographies(data)
    H_optical, H_thermal = data['optical']['homography'], data['thermal']['homography']
    data = utils.data_to_device(data, device)
    return (data, H_optical, H_thermal) + _forward_pair(net, data)


def _repeatability_samples(out_optical, out_thermal, data, H_optical, H_thermal, detection_threshold):
    """Per sample of a batch: (n_kp_optical, n_kp_thermal, N_optical, N_thermal, d1, d2).  Keypoints are nonzero((prob > thr) * valid_mask);
    each set goes into the other frame through H.inverse() and the other H with the truncating warp_keypoints and is filtered to the image
    (N_*: what is left); d1 / d2: for every warped thermal / optical point the distance to the nearest optical / thermal keypoint (the
    reference: all-pairs norm, then np.min(axis=1)), empty when that image has no keypoint."""
    samples = []
    for (prob_o, prob_t, mask_o, mask_t, h_o, h_t) in zip(out_optical['prob'].split(1), out_thermal['prob'].split(1),
                                                          data['optical']['valid_mask'].split(1), data['thermal']['valid_mask'].split(1),
                                                          H_optical.split(1), H_thermal.split(1)):
        kp_optical_d = torch.nonzero((prob_o.squeeze() > detection_threshold).float() * mask_o.squeeze().to(prob_o.device))
        kp_thermal_d = torch.nonzero((prob_t.squeeze() > detection_threshold).float() * mask_t.squeeze().to(prob_t.device))
        image_shape = tuple(prob_o.squeeze().shape)
        m = _sample_matrices(h_o, h_t)
        warped_optical = filter_points(warp_keypoints(warp_keypoints(kp_optical_d.cpu().numpy(), m.h_o_inv), m.h_t), image_shape)
        warped_thermal = filter_points(warp_keypoints(warp_keypoints(kp_thermal_d.cpu().numpy(), m.h_t_inv), m.h_o), image_shape)
        none = np.zeros((0,), np.float32)
        d1 = _min_dist(warped_thermal, kp_optical_d.float()) if kp_optical_d.shape[0] != 0 else none
        d2 = _min_dist(warped_optical, kp_thermal_d.float()) if kp_thermal_d.shape[0] != 0 else none
        samples.append((kp_optical_d.shape[0], kp_thermal_d.shape[0], warped_optical.shape[0], warped_thermal.shape[0], d1, d2))
    return samples


def compute_repeatability_for_sample(out_optical, out_thermal, data, H_optical, H_thermal, detection_threshold, distance_thresh):
    """benchmark_evaluation.py:396-467; same returns: ({th: [repeatability]}, n_kp_optical list, n_kp_thermal list)."""
    samples = _repeatability_samples(out_optical, out_thermal, data, H_optical, H_thermal, detection_threshold)
    repeatability_member_dict = {}
    for (_, _, N_optical, N_thermal, d1, d2) in samples:
        for th in _as_list(distance_thresh):                 # overwritten per sample, as in the reference
            count = int(np.sum(d1 <= th)) + int(np.sum(d2 <= th))
            repeatability_member_dict[th] = [count / (N_thermal + N_optical)] if N_thermal + N_optical > 0 else []
    return repeatability_member_dict, [s[0] for s in samples], [s[1] for s in samples]


def compute_mAP(precision, recall):
    """benchmark_evaluation.py:469-473."""
    return np.sum(precision[1:] * (recall[1:] - recall[:-1]))


def _mutual_matches(desc_o, desc_t):
    """Both reference calls get_matches(desc_o, desc_t) and get_matches(desc_t, desc_o) (bfmatcher, crossCheck) from one
    device call: lists of (queryIdx, trainIdx, distance) ordered by queryIdx, as BFMatcher.match returns them."""
    if desc_o.shape[0] == 0 or desc_t.shape[0] == 0:
        return [], []
    res = utils.match_descriptors(desc_o[None].contiguous(), desc_t[None].contiguous(), None, "strict_mnn")
    n = int(res["match_count"][0].item())
    q = res["match_q"][0, :n].cpu().numpy(); t = res["match_t"][0, :n].cpu().numpy(); d = res["match_d"][0, :n].cpu().numpy()
    m_o = [(int(a), int(b), float(c)) for a, b, c in zip(q, t, d)]                    # query = optical (ascending q)
    order = np.argsort(t, kind="stable")
    m_t = [(int(t[i]), int(q[i]), float(d[i])) for i in order]                        # query = thermal (ascending t)
    return m_o, m_t


def _descriptor_samples(prob_optical, prob_thermal, desc_optical, desc_thermal, data, keypoint_detection_threshold):
    """Per sample of a batch, what the descriptor metrics and the corner error both start from: the descriptor keypoints nonzero(prob > thr)
    of the (already masked) heat maps (kp_o, kp_t: device, (y, x)), the descriptors sampled at them, and their mutual matches (m_o, m_t: see
    _mutual_matches) — one sampling and ONE matcher call per sample — with the sample's matrices, the heat map's shape and the image's."""
    H_o, W_o = data['optical']['image'].shape[2:]
    H_t, W_t = data['thermal']['image'].shape[2:]
    samples = []
    for (prob_o, prob_t, h_o, h_t, desc_o, desc_t) in zip(prob_optical, prob_thermal, data['optical']['homography'],
                                                          data['thermal']['homography'], desc_optical, desc_thermal):
        kp_o = torch.nonzero((prob_o.squeeze() > keypoint_detection_threshold).float())
        kp_t = torch.nonzero((prob_t.squeeze() > keypoint_detection_threshold).float())
        m_o, m_t = _mutual_matches(utils.interpolate_descriptors(kp_o, desc_o, H_o, W_o), utils.interpolate_descriptors(kp_t, desc_t, H_t, W_t))
        samples.append(dict(kp_o=kp_o, kp_t=kp_t, m_o=m_o, m_t=m_t, matrices=_sample_matrices(h_o, h_t),
                            prob_shape=tuple(prob_o.squeeze().shape), image_hw=(H_o, W_o)))
    return samples


def _descriptor_bookkeeping(samples, threshold_keypoints):
    """compute_descriptor_for_sample's dictionary from the records of _descriptor_samples."""
    per_sample = []
    for s in samples:
        matches_optical = sorted(s["m_o"], key=lambda x: x[2])
        matches_thermal = sorted(s["m_t"], key=lambda x: x[2])
        warped_optical = warp_keypoints(s["kp_o"].cpu().float().numpy(), s["matrices"].gt, float)
        warped_thermal = warp_keypoints(s["kp_t"].cpu().float().numpy(), s["matrices"].gt_inv, float)
        # rows of the reference's correct_* matrices that contain a True <=> the nearest keypoint is within th
        near_o = _min_dist(warped_optical, s["kp_t"].float())
        near_t = _min_dist(warped_thermal, s["kp_o"].float())
        po, pt = s["kp_o"].cpu().numpy().astype(np.float64), s["kp_t"].cpu().numpy().astype(np.float64)

        def pair_dist(w, other, matches):       # |warped[q] - other[t]| for the matched pairs, in the reference's f32 arithmetic
            if not matches:
                return np.zeros((0,), np.float32)
            qi = np.array([m[0] for m in matches]); ti = np.array([m[1] for m in matches])
            diff = (w[qi].astype(np.float64) - other[ti]).astype(np.float32)
            return np.sqrt(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1])
        per_sample.append(dict(mo=matches_optical, mt=matches_thermal, near_o=near_o, near_t=near_t,
                               pd_o=pair_dist(warped_optical, pt, matches_optical), pd_t=pair_dist(warped_thermal, po, matches_thermal),
                               N_optical=filter_points(warped_optical, s["prob_shape"]).shape[0],
                               N_thermal=filter_points(warped_thermal, s["prob_shape"]).shape[0]))
    descriptor_dict = {}
    for th in _as_list(threshold_keypoints):
        tp_o, tp_t, dist_o, dist_t, ms_o, ms_t, mk = [], [], [], [], [], [], []
        n_gt_o = n_gt_t = 0
        for s in per_sample:
            n_gt_o = int(np.sum(s["near_o"] <= th))          # overwritten per sample, as in the reference
            n_gt_t = int(np.sum(s["near_t"] <= th))
            c_o = (s["pd_o"] <= th); c_t = (s["pd_t"] <= th)
            tp_o += [bool(v) for v in c_o]; dist_o += [m[2] for m in s["mo"]]
            tp_t += [bool(v) for v in c_t]; dist_t += [m[2] for m in s["mt"]]
            nm_o, nm_t = int(c_o.sum()), int(c_t.sum())
            ms_o.append(float(nm_o) / s["N_optical"] if s["N_optical"] > 0 else 0.0)
            ms_t.append(float(nm_t) / s["N_thermal"] if s["N_thermal"] > 0 else 0.0)
            mk.append((nm_o + nm_t) // 2)
        descriptor_dict[th] = dict(tp_optical=tp_o, tp_thermal=tp_t, distance_optical=dist_o, distance_thermal=dist_t,
                                   m_score_optical=ms_o, m_score_thermal=ms_t, matching_kp_numbers=mk,
                                   n_gt_optical=n_gt_o, n_gt_thermal=n_gt_t)
    return descriptor_dict


def compute_descriptor_for_sample(prob_optical, prob_thermal, desc_optical, desc_thermal, data, config,
                                  keypoint_detection_threshold, threshold_keypoints):
    """benchmark_evaluation.py:588-751; same returns ({th: {tp_*, distance_*, m_score_*, matching_kp_numbers, n_gt_*}}).
    desc_* are the network's dense descriptor maps (B, D, Hc, Wc) on the device."""
    _check_matcher(config)
    return _descriptor_bookkeeping(_descriptor_samples(prob_optical, prob_thermal, desc_optical, desc_thermal, data, keypoint_detection_threshold),
                                   threshold_keypoints)


def _pts_dist_bookkeeping(samples, ransac_reporjection_thresholds):
    """compute_pts_dist_for_sample's dictionary from the records of _descriptor_samples."""
    pts = []
    for s in samples:
        if s["m_o"]:
            dev = s["kp_o"].device
            qi = torch.tensor([m[0] for m in s["m_o"]], device=dev); ti = torch.tensor([m[1] for m in s["m_o"]], device=dev)
            pts.append((s["kp_o"][qi].flip(-1).float(), s["kp_t"][ti].flip(-1).float()))       # cv2.KeyPoint(x = col, y = row)
        else:
            pts.append((torch.zeros((0, 2), device=s["kp_o"].device),) * 2)
    out = {}
    for th in _as_list(ransac_reporjection_thresholds):
        member = []
        for s, (optical_pts, thermal_pts) in zip(samples, pts):
            H_est, _ = utils.find_homography(optical_pts, thermal_pts, th) if optical_pts.shape[0] >= 4 else (None, None)
            if H_est is not None:
                H_o = s["image_hw"][0]
                corners = np.array([[0, 0], [H_o, 0], [0, s["image_hw"][1]], [H_o, H_o]])
                gt = warp_keypoints(corners, s["matrices"].gt, float)
                est = warp_keypoints(corners, H_est, float)
                member.append(np.linalg.norm(est - gt, axis=1).sum() / 4)
            else:
                member.append(999.0)
        out[th] = member
    return out


def compute_pts_dist_for_sample(prob_optical, prob_thermal, desc_optical, desc_thermal, data, config, keypoint_detection_threshold,
                                ransac_reporjection_thresholds):
    """benchmark_evaluation.py:755-830: mean distance of the four image "corners" (the reference's own point list,
    [[0,0],[H,0],[0,W],[H,H]]) warped by the ground-truth and by the estimated optical->thermal homography; 999.0 when
    no model could be estimated.  Returns {threshold: [distance per sample]}."""
    return _pts_dist_bookkeeping(_descriptor_samples(prob_optical, prob_thermal, desc_optical, desc_thermal, data, keypoint_detection_threshold),
                                 ransac_reporjection_thresholds)


def _pr_envelope(tp, n_gt, div):
    """(precision, recall) of true-positive flags sorted by rank: cumulative sums, recall = tp_cum / n_gt and precision = tp_cum / (tp_cum +
    fp_cum) under the division rule `div` (div0 or _div0_one: what a zero denominator gives), padded with [0] .. [1] and [0] .. [0], and the
    precision replaced by its envelope (the maximum over everything to the right)."""
    tp_cum, fp_cum = np.cumsum(tp), np.cumsum(np.logical_not(tp))
    recall = np.concatenate([[0], div(tp_cum, n_gt), [1]])
    precision = np.concatenate([[0], div(tp_cum, tp_cum + fp_cum), [0]])
    return np.maximum.accumulate(precision[::-1])[::-1], recall


def compute_desc_dict(descriptor_metrics_dict):
    """benchmark_evaluation.py:476-558 (host numpy on the per-match lists)."""
    results = {}
    for th, d in descriptor_metrics_dict.items():
        out = {}
        maps = {}
        for spec in ("optical", "thermal"):
            tp = np.array(d[f'tp_{spec}']); dist = np.array(d[f'distance_{spec}'])
            idx = np.argsort(dist)
            tp = tp[idx]; fp = np.logical_not(tp); dist = dist[idx]
            precision, recall = _pr_envelope(tp, d[f'n_gt_{spec}'], div0)
            maps[spec] = compute_mAP(precision, recall)
            out.update({f'tp_{spec}': tp, f'fp_{spec}': fp, f'distance_{spec}': dist, f'recall_{spec}': recall,
                        f'precision_{spec}': precision, f'nn_map_{spec}': maps[spec], f'm_score_{spec}': np.array(d[f'm_score_{spec}'])})
        out['nn_map'] = (maps['optical'] + maps['thermal']) * 0.5
        out['m_score'] = (out['m_score_optical'].mean() + out['m_score_thermal'].mean()) * 0.5
        results[th] = out
    return results


def compute_homography_dict(overall_pts_dist_dict, threshold_warp):
    """benchmark_evaluation.py:560-586."""
    results = {}
    for th_ransac, dists in overall_pts_dist_dict.items():
        pts_dist = np.array(dists)
        out = {'average_h_error': pts_dist.mean(), 'h_correctness': {}}
        for th_warp in threshold_warp:
            out['h_correctness']['epsilon_warp_th' + str(th_warp)] = (pts_dist < th_warp).sum() / len(pts_dist)
        results[th_ransac] = out
    return results


class _MetricsAccumulator:
    """The data-set loop's running lists (benchmark_evaluation.py:851-935) and its closing lines (:937-963), for compute_metrics and
    compute_metrics_batched alike."""

    def __init__(self, thresh_repeatability, thresh_keypoints, ransac_reproj_thresholds):
        self.repeatability = {th: [] for th in _as_list(thresh_repeatability)}
        self.n_kp_optical, self.n_kp_thermal = [], []
        self.descriptor = {th: {} for th in _as_list(thresh_keypoints)}
        self.pts_dist = {th: [] for th in _as_list(ransac_reproj_thresholds)}

    def add(self, repeatability, descriptor, pts_dist):
        """One batch: compute_repeatability_for_sample's triple, compute_descriptor_for_sample's dictionary (lists are concatenated, the
        n_gt_* counts summed) and (RANSAC threshold, [corner error per sample]) pairs."""
        rep, nko, nkt = repeatability
        for key, value in rep.items():
            self.repeatability[key].extend(value)
        self.n_kp_optical += nko; self.n_kp_thermal += nkt
        for key, value in descriptor.items():
            for key2, value2 in value.items():
                self.descriptor[key][key2] = self.descriptor[key].get(key2, 0 if key2.startswith("n_gt") else []) + value2
        for key, value in pts_dist:
            self.pts_dist[key] += value

    def result(self, thresh_warp):
        out_rep = {'repeatability_mean': {k: np.mean(v) for k, v in self.repeatability.items()},
                   'n_kp_optical': np.mean(self.n_kp_optical), 'n_kp_thermal': np.mean(self.n_kp_thermal)}
        out_rep['n_kp_avg'] = (out_rep['n_kp_optical'] + out_rep['n_kp_thermal']) / 2.0
        return {"repeatability": out_rep, "descriptor": compute_desc_dict(self.descriptor),
                "homography": compute_homography_dict(self.pts_dist, _as_list(thresh_warp))}


def compute_metrics(net, dataloader, device, config, keypoint_detection_threshold=0.015, thresh_repeatability=3, thresh_keypoints=2,
                    thresh_warp=2, ransac_reproj_thresholds=3):
    """benchmark_evaluation.py:832-963.  `dataloader` is any iterable of reference-style `data` dicts; returns
    {'repeatability': ..., 'descriptor': ..., 'homography': ...} (the last one from this build's estimator).  The reference samples and
    matches every sample twice (once per compute_*_for_sample call); here one _descriptor_samples per batch feeds both."""
    _check_matcher(config)
    acc = _MetricsAccumulator(thresh_repeatability, thresh_keypoints, ransac_reproj_thresholds)
    pred = config['prediction']
    for data in dataloader:
        data, H_optical, H_thermal, out_optical, out_thermal = _batch_preamble(net, data, device)
        prob_optical = out_optical['prob'] * data['optical']['valid_mask']
        prob_thermal = out_thermal['prob'] * data['thermal']['valid_mask']
        if pred['nms'] > 0:
            kw = dict(keep_top_k=pred['topk'], on_cpu=pred.get('cpu_nms', False))
            prob_thermal = utils.box_nms(prob_thermal, pred['nms'], keypoint_detection_threshold, **kw)
            prob_optical = utils.box_nms(prob_optical, pred['nms'], keypoint_detection_threshold, **kw)
            out_optical['prob'] = utils.box_nms(out_optical['prob'], pred['nms'], keypoint_detection_threshold, **kw)
            out_thermal['prob'] = utils.box_nms(out_thermal['prob'], pred['nms'], keypoint_detection_threshold, **kw)
        samples = _descriptor_samples(prob_optical, prob_thermal, out_optical['desc'], out_thermal['desc'], data, keypoint_detection_threshold)
        acc.add(compute_repeatability_for_sample(out_optical, out_thermal, data, H_optical, H_thermal, keypoint_detection_threshold,
                                                 thresh_repeatability),
                _descriptor_bookkeeping(samples, thresh_keypoints),
                _pts_dist_bookkeeping(samples, _as_list(ransac_reproj_thresholds)).items())
    return acc.result(thresh_warp)


# ------------------------------------------------------------------------------------------------
# The same metrics for a whole batch on the device (DESIGN.md "Matching evaluation"; include/xpoint_hip.h, xp_pair_eval_*).
# ------------------------------------------------------------------------------------------------
PAIR_EVAL_MAX_THRESHOLDS = 16          # thresholds per xp_pair_eval_count launch (longer lists take several launches)


def pair_eval_matrices(H_o, H_t):
    """The 3 x 3 matrices of one batch: _sample_matrices of every sample (the host computation the per-sample functions use), laid out for the
    kernels.  H_o, H_t: (B, 3, 3).  Returns float64 numpy arrays: rep_map1, rep_map2, desc_map1 (2B, 9) — per image, optical images first —
    and gt (B, 9)."""
    ms = [_sample_matrices(h_o, h_t) for h_o, h_t in zip(H_o, H_t)]
    f = lambda rows: np.stack([np.asarray(r, dtype=np.float64).reshape(9) for r in rows])
    return (f([m.h_o_inv for m in ms] + [m.h_t_inv for m in ms]), f([m.h_t for m in ms] + [m.h_o for m in ms]),      # optical -> scene -> thermal
            f([m.gt for m in ms] + [m.gt_inv for m in ms]), f([m.gt for m in ms]))


def _pe_warp_near(kp, counts, P, cap, H, W, map1, map2, truncate):
    dev = kp.device
    warped = torch.empty((2 * P, cap, 2), dtype=torch.float64, device=dev)
    inframe = torch.empty((2 * P, cap), dtype=torch.uint8, device=dev)
    near = torch.empty((2 * P, cap), dtype=torch.float32, device=dev)
    _lib.call("xp_pair_eval_warp_near", ptr(kp), ptr(counts), P, cap, int(H), int(W), ptr(map1), ptr(map2), int(bool(truncate)),
              ptr(warped), ptr(inframe), ptr(near), _lib.current_stream(dev))
    return warped, inframe, near


def _pe_match_dist(kp, counts, warped, res, P, cap):
    dist = torch.empty((2, P, cap), dtype=torch.float32, device=kp.device)
    _lib.call("xp_pair_eval_match_dist", ptr(kp), ptr(counts), ptr(warped), ptr(res["match_q"]), ptr(res["match_t"]), ptr(res["match_count"]),
              P, cap, ptr(dist), _lib.current_stream(kp.device))
    return dist


def _pe_count(near, inframe, counts, dist, match_count, P, cap, thresholds, inframe_only):
    """(near_cnt (2, P, T), match_cnt (2, P, T), n_inframe (2, P)) int32 on the device; one launch per 16 thresholds."""
    dev = near.device
    ths = [float(t) for t in thresholds]
    if not ths:
        raise ValueError("pair evaluation: the threshold list is empty")
    near_cnt, match_cnt = [], []
    n_in = torch.empty((2, P), dtype=torch.int32, device=dev)
    for k0 in range(0, len(ths), PAIR_EVAL_MAX_THRESHOLDS):
        part = ths[k0:k0 + PAIR_EVAL_MAX_THRESHOLDS]
        T = len(part)
        nc = torch.empty((2, P, T), dtype=torch.int32, device=dev)
        mc = torch.zeros((2, P, T), dtype=torch.int32, device=dev)
        _lib.call("xp_pair_eval_count", ptr(near), ptr(inframe), ptr(counts), ptr(dist), ptr(match_count), P, cap, (ctypes.c_float * T)(*part), T,
                  int(bool(inframe_only)), ptr(nc), ptr(mc), ptr(n_in), _lib.current_stream(dev))
        near_cnt.append(nc); match_cnt.append(mc)
    return torch.cat(near_cnt, 2), torch.cat(match_cnt, 2), n_in


def _pe_corner_error(H_gt, H_est, n_inliers, match_count, P, H, W):
    err = torch.empty((P,), dtype=torch.float64, device=H_gt.device)
    H_est = H_est.contiguous()
    _lib.call("xp_pair_eval_corner_error", ptr(H_gt), ptr(H_est), ptr(n_inliers), ptr(match_count), P, int(H), int(W), ptr(err),
              _lib.current_stream(H_gt.device))
    return err


def pair_metrics_batched(prob_rep_o, prob_rep_t, prob_desc_o, prob_desc_t, desc_o, desc_t, H_o, H_t, detection_threshold, thresh_repeatability,
                         thresh_keypoints, ransac_reproj_thresholds, cap=None, mask_rep_o=None, mask_rep_t=None):
    """compute_repeatability_for_sample + compute_descriptor_for_sample + compute_pts_dist_for_sample for ONE batch as device work.

    prob_rep_* (B, 1, H, W): the heat maps of the repeatability keypoints, nonzero((prob > thr) * mask_rep_*) (mask_rep_*: the valid masks, or
    None); prob_desc_* (B, 1, H, W): the (already masked) heat maps of the descriptor keypoints, nonzero(prob > thr); desc_* (B, D, Hc, Wc) the
    dense descriptor maps; H_o, H_t (B, 3, 3) the sample homographies — HOST tensors (pair_eval_matrices prepares the B x 9 numbers on the
    host, one upload per batch).  cap: the capacity of the ragged lists; when it is given (prediction.topk > 0 bounds every list) nothing is
    read back, otherwise the largest count is read once.

    Launch plan: two xp_extract_keypoints (each over the 2B stacked maps), one xp_sample_descriptors, ONE xp_match_mnn over the B pairs (compute_metrics
    makes one call per sample), xp_pair_eval_warp_near + xp_pair_eval_count for the repeatability set, warp_near +
    match_dist + count for the descriptor set, xp_gather_match_points, and per RANSAC threshold one xp_find_homography and one
    xp_pair_eval_corner_error.  The reference's match order (sorted by distance, equal distances by ascending query index for query = optical
    and by ascending target index for query = thermal) comes from torch's stable sort on the device.

    Returns device tensors (B pairs, Tr / Tk / R thresholds), directions [0] = optical image is the query, [1] = thermal:
      n_kp (2B)                      repeatability keypoints per image, optical images first
      rep_count (2, B, Tr), rep_inframe (2, B)      warped in-frame points with a keypoint of the other image within th / their number
      n_desc_kp (2B), n_gt (2, B, Tk), desc_inframe (2, B), match_ok (2, B, Tk), match_count (B)
      match_dist (2, B, cap), pair_dist (2, B, cap)  matcher distance and |warped - matched| per match, in the reference's order (+inf filler)
      corner_error (R, B) float64, H_est (R, B, 3, 3), n_inliers (R, B)
      overflow ()  bool: a list was longer than cap and is truncated (compute_metrics_batched refuses such a result)
    Homography estimates: xp_find_homography seeds its hypotheses with the PAIR INDEX, so sample p of a batch draws as pair p while the
    per-sample path always draws as pair 0: corner_error of sample 0 equals compute_pts_dist_for_sample's, the other samples get the batched
    estimator's (equally valid) estimate."""
    if not (torch.is_tensor(prob_rep_o) and prob_rep_o.is_cuda):
        raise ValueError("pair_metrics_batched: the heat maps must be GPU tensors (no CPU fallback)")
    H, W = (int(v) for v in prob_rep_o.shape[-2:])
    B = prob_rep_o.numel() // (H * W)
    dev = prob_rep_o.device
    ths_rep, ths_kp, ths_ransac = _as_list(thresh_repeatability), _as_list(thresh_keypoints), _as_list(ransac_reproj_thresholds)
    stack = lambda a, b: torch.cat([a.reshape(B, H, W).float(), b.reshape(B, H, W).float()])
    with torch.cuda.device(dev):
        mask = None
        if mask_rep_o is not None or mask_rep_t is not None:
            ones = torch.ones((B, H, W), dtype=torch.bool, device=dev)
            mask = torch.cat([ones if m is None else (m.reshape(B, H, W).to(dev) != 0) for m in (mask_rep_o, mask_rep_t)])
        kp_r, cnt_r = utils.extract_keypoints(stack(prob_rep_o, prob_rep_t), detection_threshold, mask, cap)
        kp_d, cnt_d = utils.extract_keypoints(stack(prob_desc_o, prob_desc_t), detection_threshold, None, cap)
        if cap is None:
            cap = max(1, int(torch.maximum(cnt_r.max(), cnt_d.max()).item()))                  # the one read-back of an unbounded batch
            kp_r, kp_d = kp_r[:, :cap].contiguous(), kp_d[:, :cap].contiguous()
        cap = int(cap)
        overflow = (cnt_r > cap).any() | (cnt_d > cap).any()
        cnt_r, cnt_d = cnt_r.clamp(max=cap), cnt_d.clamp(max=cap)
        tables = np.concatenate(pair_eval_matrices(H_o, H_t))
        tables = torch.from_numpy(tables).to(dev)                                               # the one upload: (7B, 9) float64
        rep1, rep2, desc1, gt = tables[:2 * B], tables[2 * B:4 * B], tables[4 * B:6 * B], tables[6 * B:]

        # repeatability: two truncating maps, counts over the in-frame points
        _, in_r, near_r = _pe_warp_near(kp_r, cnt_r, B, cap, H, W, rep1, rep2, True)
        rep_count, _, rep_inframe = _pe_count(near_r, in_r, cnt_r, None, None, B, cap, ths_rep, True)

        # descriptors: one sampling call, one matcher call, one float map per direction
        nhwc = torch.cat([desc_o, desc_t]).permute(0, 2, 3, 1).contiguous().float()
        Hc, Wc, D = (int(v) for v in nhwc.shape[1:])
        d = torch.zeros((2 * B, cap, D), dtype=torch.float32, device=dev)
        _lib.call("xp_sample_descriptors", ptr(kp_d), ptr(cnt_d), ptr(nhwc), ptr(d), 2 * B, cap, Hc, Wc, D, H, W, _lib.current_stream(dev))
        res = utils.match_descriptors(d[:B], d[B:], cnt_d, "strict_mnn")
        mcount = res["match_count"]
        warped_d, in_d, near_d = _pe_warp_near(kp_d, cnt_d, B, cap, H, W, desc1, None, False)
        pd = _pe_match_dist(kp_d, cnt_d, warped_d, res, B, cap)
        n_gt, match_ok, desc_inframe = _pe_count(near_d, in_d, cnt_d, pd, mcount, B, cap, ths_kp, False)

        # the reference's order of the two match lists
        live = torch.arange(cap, device=dev)[None, :] < mcount[:, None]
        dkey = torch.where(live, res["match_d"], torch.full_like(res["match_d"], float("inf")))
        order_o = torch.sort(dkey, dim=1, stable=True).indices
        tkey = torch.where(live, res["match_t"], torch.full_like(res["match_t"], 2 ** 31 - 1))
        by_t = torch.sort(tkey, dim=1, stable=True).indices
        order_t = by_t.gather(1, torch.sort(dkey.gather(1, by_t), dim=1, stable=True).indices)
        match_dist = torch.stack([dkey.gather(1, order_o), dkey.gather(1, order_t)])
        pair_dist = torch.stack([pd[0].gather(1, order_o), pd[1].gather(1, order_t)])

        # homography: correspondences in the match list's own order (ascending query index), as compute_pts_dist_for_sample
        src = torch.empty((B, cap, 2), dtype=torch.float32, device=dev); dst = torch.empty_like(src)
        _lib.call("xp_gather_match_points", ptr(kp_d), ptr(res["match_q"]), ptr(res["match_t"]), ptr(mcount), B, cap, ptr(src), ptr(dst),
                  _lib.current_stream(dev))
        errs, ests, inls = [], [], []
        for th in ths_ransac:
            H_est, _, n_inl = utils.find_homography_batched(src, dst, mcount, th)
            errs.append(_pe_corner_error(gt, H_est, n_inl, mcount, B, H, W)); ests.append(H_est); inls.append(n_inl)
    return dict(n_kp=cnt_r, rep_count=rep_count, rep_inframe=rep_inframe, n_desc_kp=cnt_d, n_gt=n_gt, desc_inframe=desc_inframe, match_ok=match_ok,
                match_count=mcount, match_dist=match_dist, pair_dist=pair_dist, corner_error=torch.stack(errs), H_est=torch.stack(ests),
                n_inliers=torch.stack(inls), overflow=overflow)


def download_pair_metrics(batches):
    """The results of pair_metrics_batched calls as numpy, one device -> host copy per result array for ALL batches."""
    if not batches:
        return []
    out = [{} for _ in batches]
    for key in batches[0]:
        flat = torch.cat([b[key].reshape(-1) for b in batches]).cpu().numpy()
        o = 0
        for dst, b in zip(out, batches):
            n = b[key].numel()
            dst[key] = flat[o:o + n].reshape(tuple(b[key].shape))
            o += n
    return out


def repeatability_from_batch(r, thresh_repeatability, reference_quirks=True):
    """compute_repeatability_for_sample's returns from one downloaded batch: ({th: [..]}, n_kp_optical list, n_kp_thermal list).  With
    reference_quirks the dict holds the LAST sample's entry only (the reference overwrites it per sample), else one entry per sample that
    has a warped point in frame."""
    B = r["rep_inframe"].shape[1]
    out = {}
    for k, th in enumerate(_as_list(thresh_repeatability)):
        member = []
        for b in ([B - 1] if reference_quirks else range(B)):
            n = int(r["rep_inframe"][0, b]) + int(r["rep_inframe"][1, b])
            if n > 0:
                member.append((int(r["rep_count"][1, b, k]) + int(r["rep_count"][0, b, k])) / n)
        out[th] = member
    return out, [int(v) for v in r["n_kp"][:B]], [int(v) for v in r["n_kp"][B:]]


def descriptor_from_batch(r, thresh_keypoints, reference_quirks=True):
    """compute_descriptor_for_sample's return from one downloaded batch.  With reference_quirks n_gt_* is the LAST sample's (overwritten per
    sample in the reference), else the sum over the samples."""
    B = r["match_count"].shape[0]
    out = {}
    for k, th in enumerate(_as_list(thresh_keypoints)):
        e = {}
        thf = np.float32(th)
        for di, spec in enumerate(("optical", "thermal")):
            tp, dist, ms = [], [], []
            for b in range(B):
                n = int(r["match_count"][b])
                tp += (r["pair_dist"][di, b, :n] <= thf).tolist()
                dist += r["match_dist"][di, b, :n].tolist()
                n_in = int(r["desc_inframe"][di, b])
                ms.append(float(int(r["match_ok"][di, b, k])) / n_in if n_in > 0 else 0.0)
            e[f"tp_{spec}"], e[f"distance_{spec}"], e[f"m_score_{spec}"] = tp, dist, ms
            e[f"n_gt_{spec}"] = int(r["n_gt"][di, B - 1, k]) if reference_quirks else int(r["n_gt"][di, :, k].sum())
        e["matching_kp_numbers"] = [(int(r["match_ok"][0, b, k]) + int(r["match_ok"][1, b, k])) // 2 for b in range(B)]
        out[th] = e
    return out


def compute_metrics_batched(net, dataloader, device, config, keypoint_detection_threshold=0.015, thresh_repeatability=3, thresh_keypoints=2,
                            thresh_warp=2, ransac_reproj_thresholds=3, reference_quirks=True):
    """compute_metrics with the per-sample functions replaced by pair_metrics_batched: same arguments, same return structure.  Per batch: the
    forward, ONE box_nms over the four stacked heat-map sets (the NMS decides every image on its own), one pair_metrics_batched (no read-back
    when prediction.topk > 0 bounds the lists); the per-batch results stay on the device and come back in one pass at the end
    (download_pair_metrics); precision / recall are compute_desc_dict / compute_homography_dict, unchanged.

    reference_quirks=True keeps the reference's per-sample overwrites (the repeatability entry and n_gt_* of a batch are its LAST sample's), so
    the repeatability and descriptor dictionaries equal compute_metrics'.  False uses every sample: one repeatability entry per sample and n_gt
    summed over the samples, which bounds NN-mAP by 1.
    Homography: sample p of a batch is estimated as pair p of xp_find_homography (see pair_metrics_batched); sample 0 of every batch equals
    the per-sample path, the others are the batched estimator's estimates of the same correspondences."""
    ths_rep, ths_kp = _as_list(thresh_repeatability), _as_list(thresh_keypoints)
    rts = _as_list(ransac_reproj_thresholds)
    pred = config['prediction']
    _check_matcher(config)
    batches = []
    for data in dataloader:
        data, H_optical, H_thermal, out_optical, out_thermal = _batch_preamble(net, data, device)
        B = data['optical']['image'].shape[0]
        mask_o, mask_t = data['optical']['valid_mask'], data['thermal']['valid_mask']
        maps = [out_thermal['prob'] * mask_t, out_optical['prob'] * mask_o, out_optical['prob'], out_thermal['prob']]
        cap = None
        if pred['nms'] > 0:
            stacked = utils.box_nms(torch.cat([p.reshape(B, 1, *p.shape[-2:]).float() for p in maps]), pred['nms'], keypoint_detection_threshold,
                                    keep_top_k=pred['topk'], on_cpu=pred.get('cpu_nms', False))
            maps = list(stacked.split(B))
            if pred['topk'] > 0:
                cap = int(pred['topk'])
        batches.append(pair_metrics_batched(maps[2], maps[3], maps[1], maps[0], out_optical['desc'], out_thermal['desc'], H_optical, H_thermal,
                                            keypoint_detection_threshold, ths_rep, ths_kp, rts, cap=cap, mask_rep_o=mask_o, mask_rep_t=mask_t))
    acc = _MetricsAccumulator(ths_rep, ths_kp, rts)
    for r in download_pair_metrics(batches):
        if bool(r["overflow"]):
            raise _lib.XPointHipError("compute_metrics_batched: a keypoint list is longer than its capacity (prediction.topk)")
        acc.add(repeatability_from_batch(r, ths_rep, reference_quirks), descriptor_from_batch(r, ths_kp, reference_quirks),
                [(th, [float(v) for v in r["corner_error"][i]]) for i, th in enumerate(rts)])
    return acc.result(thresh_warp)


# ------------------------------------------------------------------------------------------------
# Detector evaluation against keypoint labels: reference xpoint/utils/evaluation.py (compute_tp_fp_dist, compute_detector_metrics,
# compute_repeatability_multispectral) — the evaluation half of predict_keypoints.py -e.
# ------------------------------------------------------------------------------------------------
def _div0_one(a, b):
    """The div0 of reference evaluation.py:206-211 (and utils.py:127-132): a / b, and where that is not finite 1 if a == 0 else 0 — so a
    data set without labels has recall 1, unlike `div0` above (benchmark_evaluation.py's, 0 there)."""
    a = np.asarray(a)
    with np.errstate(divide='ignore', invalid='ignore'):
        c = np.true_divide(a, b)
        idx = ~np.isfinite(c)
        c[idx] = np.where(a[idx] == 0, 1, 0)
    return c


def tp_fp_dist_batched(prob, keypoints, zero_threshold=1e-4, distance_thresh=2.0):
    """compute_tp_fp_dist (evaluation.py:57-97) for a batch on the device: prob (B, H, W) float32, keypoints (B, H, W) label maps (bool /
    uint8 / anything whose non-zeros are labels), both on the GPU.  Returns one (tp bool[P], fp bool[P], prob float32[P] descending,
    n_gt int, dist float32[M]) per image, as device tensors (views of batch-wide buffers).

    Formulation (include/xpoint_hip.h, xp_detector_eval_*; DESIGN.md "Detector evaluation"): a candidate is a pixel with prob >
    zero_threshold; each claims the first row-major label within the radius with a u64 atomic minimum of its rank key, and is a true
    positive iff it holds its label's minimum — the reference's greedy loop, with no (predictions x labels) tensor and no loop over
    either.  Rank order: descending prob, equal probabilities by ascending row-major pixel index (this project's rule: the reference's
    order among exact ties is whatever torch.sort does).  dist holds every within-radius (prediction, label) pair, not only the true
    positives, ordered by (rank, row-major label) — the reference's dist[matches].
    Device plumbing between the four launches: one stable torch.sort of the candidate probabilities per image (a loop over the images
    of the batch) and one cumsum of the pair counts.  One
    synchronisation: the per-image counts come back in a single copy, which sizes `dist`.  Every output of image b is what the image
    gives alone."""
    if not (torch.is_tensor(prob) and prob.is_cuda and prob.dim() == 3):
        raise ValueError("tp_fp_dist_batched: prob must be a (B, H, W) tensor on the GPU (no CPU fallback)")
    if not (torch.is_tensor(keypoints) and keypoints.is_cuda and tuple(keypoints.shape) == tuple(prob.shape)):
        raise ValueError("tp_fp_dist_batched: keypoints must be a (B, H, W) label map on the device of prob")
    B, H, W = (int(v) for v in prob.shape)
    if B == 0:
        return []
    p = prob.contiguous().float()
    kp = keypoints.contiguous()
    lab = kp.view(torch.uint8) if kp.dtype == torch.bool else (kp if kp.dtype == torch.uint8 else (kp != 0).view(torch.uint8))
    HW = H * W
    dev = p.device
    with torch.cuda.device(dev):
        st = _lib.current_stream(dev)
        cand = torch.empty((B, HW), dtype=torch.float32, device=dev)
        winner = torch.empty((B, HW), dtype=torch.int64, device=dev)
        first = torch.empty((B, HW), dtype=torch.int32, device=dev)
        within = torch.empty((B, HW), dtype=torch.int32, device=dev)
        counts = torch.empty((2, B), dtype=torch.int32, device=dev)
        _lib.call("xp_detector_eval_claim", ptr(p), ptr(lab), B, H, W, float(zero_threshold), float(distance_thresh),
                  ptr(cand), ptr(winner), ptr(first), ptr(within), ptr(counts[0]),
                  ptr(counts[1]), st)
        tp_pix = torch.empty((B, HW), dtype=torch.uint8, device=dev)
        _lib.call("xp_detector_eval_resolve", ptr(cand), ptr(winner), ptr(first), B, H, W, ptr(tp_pix), st)
        del winner, first
        # the rank order = the order of the u64 keys: descending probability, equal ones by ascending pixel index (the sort is stable and
        # its input is in pixel order); non-candidates are 0 in `cand` and come last.  One image at a time: a 1-D sort's temporaries
        # are those of one image, and they are gone before the next.
        prob_s = torch.empty((B, HW), dtype=torch.float32, device=dev)
        rank_pix = torch.empty((B, HW), dtype=torch.int64, device=dev)
        for b in range(B):
            torch.sort(cand[b], descending=True, stable=True, out=(prob_s[b], rank_pix[b]))
        del cand
        tp_s = torch.empty((B, HW), dtype=torch.bool, device=dev)
        cnt_s = torch.empty((B, HW), dtype=torch.int32, device=dev)
        _lib.call("xp_detector_eval_gather", ptr(rank_pix), ptr(tp_pix), ptr(within), ptr(counts[0]), B, H, W,
                  ptr(tp_s), ptr(cnt_s), st)
        del tp_pix, within
        incl = torch.cumsum(cnt_s.view(-1), 0, dtype=torch.int64)
        host = torch.cat([counts.view(-1).to(torch.int64), incl.view(B, HW)[:, -1]]).cpu().tolist()         # the one synchronisation
        n_cand, n_gt, ends = host[:B], host[B:2 * B], [0] + host[2 * B:]
        dist = torch.empty((ends[-1],), dtype=torch.float32, device=dev)
        _lib.call("xp_detector_eval_fill_dist", ptr(rank_pix), ptr(lab), ptr(incl), ptr(cnt_s), B, H, W,
                  float(distance_thresh), ptr(dist) if ends[-1] else None, ends[-1], st)
    out = []
    for b in range(B):
        tp = tp_s[b, :n_cand[b]]
        out.append((tp, ~tp, prob_s[b, :n_cand[b]], n_gt[b], dist[ends[b]:ends[b + 1]]))
    return out


def _as_device_tensor(x, device, dtype=None):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=device, dtype=dtype) if dtype is not None else t.to(device)


def compute_tp_fp_dist(prob, keypoints, zero_threshold=1e-4, distance_thresh=2.0):
    """evaluation.py:57-97, same returns: (tp bool[P], fp bool[P], prob float32[P] descending, n_gt int, dist float32[M]) as numpy.
    prob (H, W): tensor (any device) or array; keypoints: a label map of the same shape, or — any other shape — a point list (N, 2) of
    (y, x), turned into a map by utils.generate_keypoint_map as in the reference.  Runs on the GPU (tp_fp_dist_batched with B = 1; the
    device of prob if it has one, else the current one); equal probabilities rank by ascending pixel index."""
    if not torch.cuda.is_available():
        raise _lib.XPointHipError("xpoint_amd.evaluation.compute_tp_fp_dist runs on the GPU only (no CPU fallback)")
    device = prob.device if torch.is_tensor(prob) and prob.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if tuple(prob.shape) != tuple(keypoints.shape):
        pts = keypoints.cpu().numpy() if torch.is_tensor(keypoints) else np.asarray(keypoints)
        keypoints = utils.generate_keypoint_map(pts, tuple(prob.shape))
    p = _as_device_tensor(prob, device, torch.float32)
    k = _as_device_tensor(keypoints, device)
    tp, fp, pr, n_gt, dist = tp_fp_dist_batched(p[None], k[None], zero_threshold, distance_thresh)[0]
    return tp.cpu().numpy(), fp.cpu().numpy(), pr.cpu().numpy(), n_gt, dist.cpu().numpy()


def compute_detector_metrics(net, dataloader, device, config):
    """evaluation.py:10-55: precision / recall of a single-image detector against the keypoint labels of a data set.  `dataloader`:
    any iterable of single-image data dicts {'image' (B,1,H,W), 'valid_mask', 'keypoints' (B,H,W) label maps, ...}; `net(data)` returns
    {'prob' (B,1,H,W)}; config: the prediction section ('nms', 'detection_threshold').  Returns (precision, recall, prob, dist).
    Per batch: out['prob'] * valid_mask, box_nms(pred, nms, detection_threshold) when nms > 0 (no keep_top_k, as the reference), then
    ONE tp_fp_dist_batched call.  Across images the results are concatenated in order and sorted by descending prob with ties in
    concatenation order (the reference: np.argsort(prob)[::-1], unspecified among ties); prob and dist come back as float64 (the reference
    goes through .tolist()).  Cumulative sums and the precision envelope are host numpy, like the rest of this module."""
    tp, prob, dist, n_gt = [], [], [], 0
    for data in dataloader:
        data = utils.data_to_device(data, device)
        out = net(data)
        pred = out['prob'] * data['valid_mask']
        if config['nms'] > 0:
            pred = utils.box_nms(pred, config['nms'], config['detection_threshold'])
        res = tp_fp_dist_batched(pred[:, 0], data['keypoints'].reshape(pred[:, 0].shape))
        n = [len(r[0]) for r in res]
        m = [len(r[4]) for r in res]
        # three copies for the whole batch (the per-image results are views of batch-wide buffers, in image order)
        tp.append(torch.cat([r[0] for r in res]).cpu().numpy()); prob.append(torch.cat([r[2] for r in res]).cpu().numpy().astype(np.float64))
        dist.append(torch.cat([r[4] for r in res]).cpu().numpy().astype(np.float64))
        n_gt += sum(r[3] for r in res)
        assert len(tp[-1]) == sum(n) and len(dist[-1]) == sum(m)
    tp = np.concatenate(tp) if tp else np.zeros((0,), bool)
    prob = np.concatenate(prob) if prob else np.zeros((0,), np.float64)
    dist = np.concatenate(dist) if dist else np.zeros((0,), np.float64)
    sort_idx = np.argsort(-prob, kind="stable")
    precision, recall = _pr_envelope(tp[sort_idx], n_gt, _div0_one)
    return precision, recall, prob[sort_idx], dist


def compute_repeatability_multispectral(net, dataloader, device, config, distance_thresh=3, verbose=False):
    """evaluation.py:105-204: (mean repeatability, list per sample, n_kp_optical list, n_kp_thermal list).  Reads config['prediction']
    (detection_threshold, nms, topk, cpu_nms); homographies default to identity; keypoints = nonzero((prob > thr) * valid_mask) of the
    (optionally box_nms'ed, UNMASKED) heat map; each set is warped into the other frame with the truncating warp_keypoints through
    H.inverse() (float32, torch) and then the other H, and filtered to the image; the "distance to the nearest keypoint" of the reference's
    all-pairs norm goes through xp_points_min_dist.  Kept from the reference: a sample without any warped point is skipped (no list entry),
    and the mean of an empty list is numpy's nan (with its warning)."""
    repeatability, n_kp_optical, n_kp_thermal = [], [], []
    pred = config['prediction']
    for data in dataloader:
        detection_threshold = pred['detection_threshold']
        data, H_optical, H_thermal, out_optical, out_thermal = _batch_preamble(net, data, device)
        if pred['nms'] > 0:
            kw = dict(keep_top_k=pred['topk'], on_cpu=pred.get('cpu_nms', False))
            out_optical['prob'] = utils.box_nms(out_optical['prob'], pred['nms'], detection_threshold, **kw)
            out_thermal['prob'] = utils.box_nms(out_thermal['prob'], pred['nms'], detection_threshold, **kw)
        for (nko, nkt, N_optical, N_thermal, d1, d2) in _repeatability_samples(out_optical, out_thermal, data, H_optical, H_thermal,
                                                                               detection_threshold):
            n_kp_optical.append(nko)
            n_kp_thermal.append(nkt)
            count1, count2 = int(np.sum(d1 <= distance_thresh)), int(np.sum(d2 <= distance_thresh))
            if N_thermal + N_optical > 0:
                repeatability.append((count1 + count2) / (N_thermal + N_optical))
                if verbose:
                    print(f"repeatability {repeatability[-1]:.4f} ({count1} + {count2}) / ({N_thermal} + {N_optical})")
    return np.mean(repeatability), repeatability, n_kp_optical, n_kp_thermal


# ------------------------------------------------------------------------------------------------
# Timing harness: reference benchmark_evaluation.py:16-142 (`desc_process_and_display_sample`) — the callable benchmark.py:149-172
# drives to print "Two forward passes / Box nms / interpolate" rates.  Same signature, same loop, same `time_dict_seconds` keys.
# ------------------------------------------------------------------------------------------------
class _EventSpan:
    """One timed span on the current HIP stream: hipEvents around the enqueued work (the reference brackets with
    torch.cuda.synchronize() + time.time(), which on a GPU also counts the host's launch latency of an idle queue)."""

    def __init__(self):
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e1 = torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        self.e0.record()
        return self

    def __exit__(self, *exc):
        self.e1.record()
        return False

    def seconds(self):
        self.e1.synchronize()
        return self.e0.elapsed_time(self.e1) * 1e-3


def desc_process_and_display_sample(net, dataset, device, config, args):
    """reference benchmark_evaluation.py:16-227.  For every index in args.index: sample -> device -> forward (both spectra) ->
    box_nms(prob * valid_mask) -> per pair nonzero + interpolate_descriptors; returns
        time_dict_seconds = {"two_forward": [...], "nms": [...], "interpolate": [...]}      (one entry per sample / per pair)
    measured with HIP events on the stream the kernels run on.  With args.plot the reference goes on to match, estimate the homography
    (cv2 MAGSAC), mask the matches by the ground-truth homography and WRITE A PNG (cv2.drawMatches / imwrite, :129-218); cv2 is not
    part of this path, so the same quantities — keypoints, matches, H_est, the ground-truth matches mask — are computed on the device and
    written next to where the PNG would go, as `<same stem>.npz`."""
    import os
    time_dict_seconds = {"two_forward": [], "nms": [], "interpolate": []}
    pred = config['prediction']
    thr = pred['detection_threshold']
    for index in args.index:
        data = dataset[index]
        data = utils.data_to_device(data, device)
        data = utils.data_unsqueeze(data, 0)
        with _EventSpan() as t_fwd:
            out_optical, out_thermal = _forward_pair(net, data)
        time_dict_seconds["two_forward"].append(t_fwd.seconds())
        with _EventSpan() as t_nms:
            if pred['nms'] > 0:
                out_optical['prob'] = utils.box_nms(out_optical['prob'] * data['optical']['valid_mask'], pred['nms'], thr,
                                                    keep_top_k=pred['topk'], on_cpu=pred['cpu_nms'])
                out_thermal['prob'] = utils.box_nms(out_thermal['prob'] * data['thermal']['valid_mask'], pred['nms'], thr,
                                                    keep_top_k=pred['topk'], on_cpu=pred['cpu_nms'])
        time_dict_seconds["nms"].append(t_nms.seconds())
        n = data['optical']['image'].shape[0]
        _default_homographies(data)                         # reference :88-92
        H, W = data['optical']['image'].shape[2:]
        for i in range(n):
            prob_optical, prob_thermal = out_optical['prob'][i], out_thermal['prob'][i]
            pred_optical = torch.nonzero((prob_optical.squeeze() > thr).float())
            pred_thermal = torch.nonzero((prob_thermal.squeeze() > thr).float())
            with _EventSpan() as t_int:
                if out_optical['desc'][i].shape[1:] == prob_optical.shape[1:]:
                    # classic descriptors, directly take values (reference :117-120)
                    do, dt = out_optical['desc'][i], out_thermal['desc'][i]
                    desc_optical_sampled = do[:, pred_optical[:, 0], pred_optical[:, 1]].transpose(0, 1)
                    desc_thermal_sampled = dt[:, pred_thermal[:, 0], pred_thermal[:, 1]].transpose(0, 1)
                elif 'desc_nhwc' in out_optical:
                    desc_optical_sampled = utils.interpolate_descriptors_nhwc(pred_optical, out_optical['desc_nhwc'][i], H, W)
                    desc_thermal_sampled = utils.interpolate_descriptors_nhwc(pred_thermal, out_thermal['desc_nhwc'][i], H, W)
                else:
                    desc_optical_sampled = utils.interpolate_descriptors(pred_optical, out_optical['desc'][i], H, W)
                    desc_thermal_sampled = utils.interpolate_descriptors(pred_thermal, out_thermal['desc'][i], H, W)
            time_dict_seconds["interpolate"].append(t_int.seconds())
            if getattr(args, "plot", False):
                matches = utils.get_matches(desc_optical_sampled, desc_thermal_sampled, pred['matching']['method'], pred['matching']['knn_matches'],
                                            **pred['matching']['method_kwargs'])
                kpo, kpt = pred_optical.cpu().numpy().astype(np.float32), pred_thermal.cpu().numpy().astype(np.float32)
                optical_pts = np.float32([kpo[m.queryIdx][::-1] for m in matches]).reshape(-1, 1, 2)       # cv2.KeyPoint(c[1], c[0]).pt = (x, y)
                thermal_pts = np.float32([kpt[m.trainIdx][::-1] for m in matches]).reshape(-1, 1, 2)
                if optical_pts.shape[0] < 4 or thermal_pts.shape[0] < 4:
                    H_est = np.eye(3, 3)
                else:
                    H_est, _ = utils.find_homography(optical_pts, thermal_pts, float(pred['reprojection_threshold']), 10000)
                # correct matches mask (reference :189-193): matches whose ground-truth reprojection error is below the threshold
                H_gt = np.matmul(data['thermal']['homography'][i].cpu().numpy(), np.linalg.inv(data['optical']['homography'][i].cpu().numpy()))
                if len(matches):
                    warped_optical = warp_keypoints(optical_pts.squeeze(1)[:, ::-1], H_gt)[:, ::-1]
                    diff = np.linalg.norm(thermal_pts.squeeze(1) - warped_optical, axis=1)
                    matchesMask = (diff < pred['reprojection_threshold'])
                else:
                    matchesMask = np.zeros((0,), bool)
                save_dir = os.path.join(args.output_dir, 'images', 'supp', 'i' + str(index))
                os.makedirs(save_dir, exist_ok=True)
                stem = "{}_{}_i{}_s{}".format(os.path.join(save_dir, args.model_dir.split("/")[-1]), args.version, index, args.seed)
                np.savez(stem + ".npz", kp_optical=kpo, kp_thermal=kpt, matches=np.array([[m.queryIdx, m.trainIdx] for m in matches], np.int32).reshape(-1, 2),
                         H_est=np.eye(3) if H_est is None else H_est, matches_mask=matchesMask)
    return time_dict_seconds
