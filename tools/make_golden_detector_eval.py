"""Generate tests/golden/g28_detector_eval.npz by running the REAL reference detector evaluation (xpoint.utils.evaluation:
compute_tp_fp_dist, compute_detector_metrics, compute_repeatability_multispectral, imported from the reference tree with the harness shims
of oracle/refharness, which this tool imports and does not modify) on the CPU.  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_detector_eval.py

Inputs come from tests/detector_eval_cases.py (hash RNG of xpoint_amd.synth), so the tests regenerate them; the file holds the seed and the
reference's outputs only:
  seed
  tpfp/<case>/{tp, fp, prob, n_gt, dist, order}     compute_tp_fp_dist; order = row-major pixel index of every prediction in rank order,
                                                    read off the returned probabilities (they are pairwise distinct)
  det/<nms0|nms4>/{precision, recall, prob, dist}   compute_detector_metrics with a fake single-image net over three batches of two images
                                                    (nms4 goes through the reference's box_nms on the harness's greedy NMS)
  rep/{mean, list, n_kp_optical, n_kp_thermal}      compute_repeatability_multispectral with a fake pair net, non-identity homographies,
                                                    masks and empty samples
Conditions asserted (the ONE seed of all inputs is re-drawn until the first holds): every probability above zero_threshold is distinct
from every other one, within an image and across the whole set, so that no result depends on a sort's order among ties; no
prediction-label distance lies within 1e-4 of a case's threshold (distances are square roots of integers: automatic for 1.0, 2.0, 2.5,
asserted anyway).  One thread; fixed zip timestamps: a re-run is byte-identical.
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
from tests import detector_eval_cases as C  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g28_detector_eval.npz")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*a, **k)


def distinct(seed):
    v = C.all_candidate_values(seed)
    return len(np.unique(v)) == len(v)


def threshold_gap(thr):
    """smallest | sqrt(dy^2 + dx^2) - thr | over the integer offsets a window can hold"""
    r = int(np.floor(thr)) + 2
    d = np.sqrt(np.add.outer(np.arange(-r, r + 1) ** 2, np.arange(-r, r + 1) ** 2).astype(np.float32))
    return float(np.abs(d - np.float32(thr)).min())


def main():
    torch.set_num_threads(1)
    stubs.install()
    from xpoint.utils import evaluation as ref_eval
    for seed in range(4096):
        if distinct(seed):
            break
    else:
        raise RuntimeError("no seed gives pairwise distinct probabilities")
    g = {"seed": np.int64(seed)}
    for name in C.TP_FP_CASES:
        prob, kp, thr = C.tp_fp_case(name, seed)
        gap = threshold_gap(thr)
        assert gap == 0.0 or gap > 1e-4, (name, gap)          # on the threshold exactly (integer distance) or clear of it
        tp, fp, pr, n_gt, dist = ref_eval.compute_tp_fp_dist(torch.from_numpy(prob), torch.from_numpy(kp), C.ZERO_THRESHOLD, thr)
        flat = prob.ravel()
        lookup = {float(v): i for i, v in enumerate(flat) if v > np.float32(C.ZERO_THRESHOLD)}
        order = np.array([lookup[float(v)] for v in pr], np.int64)
        assert len(set(order.tolist())) == len(order) == len(lookup)
        g[f"tpfp/{name}/tp"], g[f"tpfp/{name}/fp"] = np.asarray(tp, bool), np.asarray(fp, bool)
        g[f"tpfp/{name}/prob"] = np.asarray(pr, np.float32).reshape(-1)
        g[f"tpfp/{name}/n_gt"] = np.int64(n_gt)
        g[f"tpfp/{name}/dist"] = np.asarray(dist, np.float32).reshape(-1)
        g[f"tpfp/{name}/order"] = order
        print(f"tpfp/{name}: {len(order)} predictions, {int(n_gt)} labels, {int(np.sum(tp))} tp, {len(g[f'tpfp/{name}/dist'])} pairs within {thr}")
    for tag, cfg in C.DET_CONFIGS.items():
        data, probs = C.detector_batches(seed)
        precision, recall, pr, dist = quiet(ref_eval.compute_detector_metrics, C.FakeSingleNet(probs), data, torch.device("cpu"), copy.deepcopy(cfg))
        g[f"det/{tag}/precision"], g[f"det/{tag}/recall"] = np.asarray(precision, np.float64), np.asarray(recall, np.float64)
        g[f"det/{tag}/prob"], g[f"det/{tag}/dist"] = np.asarray(pr, np.float64), np.asarray(dist, np.float64)
        print(f"det/{tag}: {len(pr)} predictions, mAP {ref_eval.compute_mAP(precision, recall):.6f}, {len(dist)} pairs")
    data, probs = C.repeatability_batches(seed)
    mean, lst, nko, nkt = quiet(ref_eval.compute_repeatability_multispectral, C.FakePairNet(probs), data, torch.device("cpu"),
                                copy.deepcopy(C.REP_CONFIG), distance_thresh=C.REP_DISTANCE_THRESH)
    g["rep/mean"], g["rep/list"] = np.float64(mean), np.asarray(lst, np.float64)
    g["rep/n_kp_optical"], g["rep/n_kp_thermal"] = np.asarray(nko, np.int64), np.asarray(nkt, np.int64)
    print(f"rep: mean {mean:.6f} over {len(lst)} of {len(nko)} samples, keypoints {nko} / {nkt}")
    savez_deterministic(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(g)} arrays, seed {seed})")


if __name__ == "__main__":
    main()
