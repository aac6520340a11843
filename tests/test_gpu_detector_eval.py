"""Detector evaluation on the device (xp_detector_eval_* through xpoint_amd.evaluation) against the REAL reference's outputs
(tests/golden/g28_detector_eval.npz, inputs regenerated from the stored seed) and this project's own guarantees: batch invariance, the
tie rule, no (predictions x labels) tensor, and the `keypoints -e` command line."""
import os

import numpy as np
import pytest
import torch

from tests import detector_eval_cases as C
from tests.test_cpu_detector_eval import tp_fp_rule
from xpoint_amd import evaluation, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(C.TP_FP_CASES))
def test_tp_fp_dist_equals_the_reference(gpu_lib, golden, name):
    g = golden("g28_detector_eval.npz")
    prob, kp, thr = C.tp_fp_case(name, int(g["seed"]))
    tp, fp, pr, n_gt, dist = evaluation.compute_tp_fp_dist(torch.from_numpy(prob), torch.from_numpy(kp), C.ZERO_THRESHOLD, thr)
    assert tp.dtype == bool and fp.dtype == bool and pr.dtype == np.float32 and dist.dtype == np.float32
    assert np.array_equal(tp, g[f"tpfp/{name}/tp"]) and np.array_equal(fp, g[f"tpfp/{name}/fp"])
    assert n_gt == int(g[f"tpfp/{name}/n_gt"])
    assert np.array_equal(_bits(pr), _bits(g[f"tpfp/{name}/prob"]))
    # the rank order, read off the (pairwise distinct) probabilities as the fixture's was
    lookup = {float(v): i for i, v in enumerate(prob.ravel()) if v > np.float32(C.ZERO_THRESHOLD)}
    assert np.array_equal(np.array([lookup[float(v)] for v in pr], np.int64), g[f"tpfp/{name}/order"])
    assert np.array_equal(_bits(dist), _bits(g[f"tpfp/{name}/dist"]))
    # a point list instead of a map, and device inputs, give the same
    again = evaluation.compute_tp_fp_dist(torch.from_numpy(prob).to(DEV), np.argwhere(kp), C.ZERO_THRESHOLD, thr)
    if kp.any():
        assert all(np.array_equal(a, b) for a, b in zip((tp, fp, pr, dist), (again[0], again[1], again[2], again[4]))) and again[3] == n_gt


@pytest.mark.parametrize("tag", list(C.DET_CONFIGS))
def test_compute_detector_metrics_equals_the_reference(gpu_lib, golden, tag):
    g = golden("g28_detector_eval.npz")
    data, probs = C.detector_batches(int(g["seed"]))
    precision, recall, prob, dist = evaluation.compute_detector_metrics(C.FakeSingleNet(probs), data, DEV, dict(C.DET_CONFIGS[tag]))
    assert np.array_equal(precision, g[f"det/{tag}/precision"]) and np.array_equal(recall, g[f"det/{tag}/recall"])
    assert np.array_equal(prob, g[f"det/{tag}/prob"])
    # the reference concatenates per image in order: the same pairs in the same order
    assert np.array_equal(dist, g[f"det/{tag}/dist"])
    assert evaluation.compute_mAP(precision, recall) > 0.05


def test_compute_repeatability_multispectral_equals_the_reference(gpu_lib, golden):
    g = golden("g28_detector_eval.npz")
    data, probs = C.repeatability_batches(int(g["seed"]))
    mean, lst, n_o, n_t = evaluation.compute_repeatability_multispectral(C.FakePairNet(probs), data, DEV, C.REP_CONFIG,
                                                                         distance_thresh=C.REP_DISTANCE_THRESH)
    assert lst == g["rep/list"].tolist() and mean == float(g["rep/mean"])
    assert n_o == g["rep/n_kp_optical"].tolist() and n_t == g["rep/n_kp_thermal"].tolist()
    # homographies default to identity: every keypoint of a pair without masks or NMS repeats itself
    d = {s: {"image": torch.zeros(1, 1, 24, 40), "valid_mask": torch.ones(1, 1, 24, 40)} for s in ("optical", "thermal")}
    p = probs[0][0][:1]
    cfg = {"prediction": {"detection_threshold": 0.015, "nms": 0, "topk": 0, "cpu_nms": False}}
    mean, lst, n_o, n_t = evaluation.compute_repeatability_multispectral(C.FakePairNet([(p, p)]), [d], DEV, cfg, distance_thresh=0)
    assert lst == [1.0] and n_o == n_t == [int((p > 0.015).sum())]


def test_batch_invariance(gpu_lib, golden):
    seed = int(golden("g28_detector_eval.npz")["seed"])
    names = ("clusters_24x40_t2", "borders_24x40_t2", "zero_labels_24x40_t2")
    cases = [C.tp_fp_case(n, seed) for n in names]
    prob = torch.from_numpy(np.stack([c[0] for c in cases])).to(DEV)
    kp = torch.from_numpy(np.stack([c[1] for c in cases])).to(DEV)
    batch = evaluation.tp_fp_dist_batched(prob, kp, C.ZERO_THRESHOLD, 2.0)
    assert len(batch) == 3
    for b in range(3):
        alone = evaluation.tp_fp_dist_batched(prob[b:b + 1], kp[b:b + 1], C.ZERO_THRESHOLD, 2.0)[0]
        for got, want in zip(batch[b], alone):
            assert got == want if isinstance(want, int) else torch.equal(got, want)
    assert len(batch[1][0]) > 0 and len(batch[1][4]) > 0


def test_equal_probabilities_rank_by_pixel_index_and_repeat(gpu_lib):
    H, W = 9, 13
    prob = np.zeros((H, W), np.float32); kp = np.zeros((H, W), bool)
    kp[4, 6] = True
    prob[4, 7] = prob[4, 5] = 0.5                      # two equal probabilities, both one pixel from the only label
    prob[1, 1] = prob[8, 12] = prob[0, 12] = 0.25      # further ties, no label near
    want = tp_fp_rule(prob, kp)
    assert want[5][:2].tolist() == [4 * W + 5, 4 * W + 7] and want[0][:2].tolist() == [True, False]
    p, k = torch.from_numpy(prob).to(DEV)[None], torch.from_numpy(kp).to(DEV)[None]
    first = None
    for _ in range(5):
        tp, fp, pr, n_gt, dist = evaluation.tp_fp_dist_batched(p, k)[0]
        assert tp.tolist() == want[0].tolist() and fp.tolist() == want[1].tolist()          # the lower pixel index wins
        assert np.array_equal(pr.cpu().numpy(), want[2]) and n_gt == 1 and dist.tolist() == [1.0, 1.0]
        if first is None:
            first = (tp, fp, pr, dist)
        assert all(torch.equal(a, b) for a, b in zip(first, (tp, fp, pr, dist)))


def test_no_predictions_by_labels_tensor_at_480x640(gpu_lib):
    """nms 0: every pixel above 1e-4 is a prediction.  The peak device memory of the call stays below 64 bytes per pixel per image; a
    (predictions x labels) tensor alone would take 4 * 500 bytes per pixel."""
    B, H, W = 2, 480, 640
    prob = torch.from_numpy(synth.uniform("g28/mem/prob", (B, H, W), 0.001, 1.0)).to(DEV)
    kp = torch.from_numpy(synth.uniform("g28/mem/kp", (B, H, W), 0.0, 1.0) < 500.0 / (H * W)).to(DEV)
    assert 400 < int(kp[0].sum()) < 600
    evaluation.tp_fp_dist_batched(prob[:1, :32, :32].contiguous(), kp[:1, :32, :32].contiguous())        # library and allocator warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = evaluation.tp_fp_dist_batched(prob, kp)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak device memory of the call: {peak / (B * H * W):.1f} bytes per pixel per image")
    assert peak < 64 * B * H * W, peak / (B * H * W)
    for b in range(B):
        tp, fp, pr, n_gt, dist = res[b]
        assert len(tp) == H * W and n_gt == int(kp[b].sum()) and 0 < int(tp.sum()) <= n_gt and len(dist) >= int(tp.sum())
        assert bool((pr[:-1] >= pr[1:]).all())
    # the host rule on image 0 (vectorised numpy over the window, no loop over predictions)
    want = tp_fp_rule(prob[0].cpu().numpy(), kp[0].cpu().numpy())
    assert np.array_equal(res[0][0].cpu().numpy(), want[0]) and np.array_equal(res[0][2].cpu().numpy(), want[2])
    assert np.array_equal(_bits(res[0][4].cpu().numpy()), _bits(want[4]))


def _cli_setup(tmp_path, with_labels):
    import yaml
    from PIL import Image
    H, W, n = 64, 96, 3
    for spec in ("optical", "thermal"):
        os.makedirs(tmp_path / "data" / spec)
        for i in range(n):
            img = synth.make_image(60 + i, spec, H, W)[0]
            Image.fromarray((img * 255).astype(np.uint8)).save(tmp_path / "data" / spec / f"p{i}.png")
    mcfg = synth.xpoint_exp1_config(H, W, vssm={"EMBED_DIM": 32})
    os.makedirs(tmp_path / "model")
    yaml.safe_dump({"model": mcfg}, open(tmp_path / "model" / "params.yaml", "w"))
    torch.save(synth.make_torch_state_dict(mcfg), tmp_path / "model" / "latest.model")
    ds = {"type": "ImagePairDataset", "foldername": str(tmp_path / "data"), "height": H, "width": W}
    if with_labels:             # the layout `cli export` writes, one list per spectrum
        lab = {}
        for i in range(n):
            for spec in ("optical", "thermal"):
                ys = synth._hash_int(f"g28/cli/{i}/{spec}/y", 40, 0, H - 1); xs = synth._hash_int(f"g28/cli/{i}/{spec}/x", 40, 0, W - 1)
                lab[f"p{i}.png/keypoints_{spec}"] = np.stack([ys, xs], 1)
        np.savez(tmp_path / "labels.npz", **lab)
        ds["keypoints_filename"] = str(tmp_path / "labels.npz")
    yaml.safe_dump({"dataset": ds, "prediction": {"detection_threshold": 0.015, "nms": 4, "cpu_nms": True, "topk": 0, "reprojection_threshold": 3,
                                                  "allow_gpu": True, "batchsize": 2, "num_worker": 0}}, open(tmp_path / "cfg.yaml", "w"))
    return ["keypoints", "-y", str(tmp_path / "cfg.yaml"), "-m", str(tmp_path / "model"), "-v", "latest"]


def test_cli_keypoints_evaluation(gpu_lib, tmp_path, capsys):
    from xpoint_amd import cli
    argv = _cli_setup(tmp_path, with_labels=True)
    out = cli.main(argv + ["-e", "-t", "3", "-o", str(tmp_path / "out.npz")])
    printed = capsys.readouterr().out
    assert "Repeatability: " in printed and "Number of optical keypoints: " in printed and "Number of thermal keypoints: " in printed
    rep_keys = {"repeatability_mean", "repeatability", "n_kp_optical", "n_kp_thermal", "distance_threshold"}
    det_keys = {f"detector_{s}_{k}" for s in ("optical", "thermal") for k in ("precision", "recall", "prob", "dist", "mAP", "mean_dist")}
    assert set(out) == rep_keys | det_keys | {"0/kp_optical", "0/kp_thermal"}
    assert len(out["n_kp_optical"]) == 3 and out["distance_threshold"] == 3 and 1 <= len(out["repeatability"]) <= 3
    # identity homographies, one shared encoder: the repeatability is that of two different images, a number in [0, 1]
    assert 0.0 <= out["repeatability_mean"] <= 1.0
    for s in ("optical", "thermal"):
        assert 0.0 <= out[f"detector_{s}_mAP"] <= 1.0 and len(out[f"detector_{s}_prob"]) > 0
        assert len(out[f"detector_{s}_precision"]) == len(out[f"detector_{s}_prob"]) + 2
    saved = np.load(tmp_path / "out.npz")
    assert rep_keys <= set(saved.files) and float(saved["repeatability_mean"]) == out["repeatability_mean"]


def test_cli_keypoints_without_evaluation_is_unchanged(gpu_lib, tmp_path):
    from xpoint_amd import cli
    argv = _cli_setup(tmp_path, with_labels=False)
    out = cli.main(argv + ["-i", "1"])
    assert set(out) == {"1/kp_optical", "1/kp_thermal"}
    out = cli.main(argv + ["-e"])                  # no label file: the repeatability alone
    assert set(out) == {"repeatability_mean", "repeatability", "n_kp_optical", "n_kp_thermal", "distance_threshold", "0/kp_optical", "0/kp_thermal"}
