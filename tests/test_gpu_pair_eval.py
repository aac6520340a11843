"""GPU: the batched matching evaluation (DESIGN.md "Matching evaluation").  The four xp_pair_eval_* kernels against their numpy restatement
(tests/pair_eval_cases.py) bit for bit; pair_metrics_batched / compute_metrics_batched against the per-sample functions (exact) and the REAL
reference's numbers (tests/golden/g13_eval_metrics.npz, at tests/test_gpu_evaluation.py's bars); the synthetic model end to end; `cli benchmark`;
`fit` with training.validation.compute_metrics."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import pair_eval_cases as pc
from xpoint_amd import synth

pytestmark = pytest.mark.gpu

CONFIG = {"prediction": {"matching": {"method": "bfmatcher", "knn_matches": False, "method_kwargs": {"crossCheck": True}}}}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_kernels(case, mode, thresholds):
    """warp_near (+ match_dist on the float map) + count on a kernel case: dict of numpy results."""
    from xpoint_amd import evaluation as ev
    P, cap, H, W = case["pairs"], case["cap"], case["H"], case["W"]
    kp, counts = _dev(case["kp"]), _dev(case["counts"])
    m1, m2 = (_dev(m) for m in case["maps"][mode])
    warped, inframe, near = ev._pe_warp_near(kp, counts, P, cap, H, W, m1, m2, mode == "rep")
    out = dict(warped=warped, inframe=inframe, near=near)
    dist = mcount = None
    if mode == "desc":
        res = {"match_q": _dev(case["match_q"]), "match_t": _dev(case["match_t"]), "match_count": _dev(case["match_count"])}
        dist, mcount = ev._pe_match_dist(kp, counts, warped, res, P, cap), res["match_count"]
        out["dist"] = dist
    for name, ths in thresholds.items():
        out[f"near_cnt/{name}"], out[f"match_cnt/{name}"], out[f"n_in/{name}"] = ev._pe_count(near, inframe, counts, dist, mcount, P, cap, ths, mode == "rep")
    return {k: v.cpu().numpy() for k, v in out.items()}


def _restate(case, mode, thresholds):
    P, cap, H, W = case["pairs"], case["cap"], case["H"], case["W"]
    m1, m2 = case["maps"][mode]
    warped, inframe, near = pc.warp_near(case["kp"], case["counts"], P, cap, H, W, m1, m2, mode == "rep")
    out = dict(warped=warped, inframe=inframe, near=near)
    dist = mcount = None
    if mode == "desc":
        dist, mcount = pc.match_dist(case["kp"], case["counts"], warped, case["match_q"], case["match_t"], case["match_count"], P, cap), case["match_count"]
        out["dist"] = dist
    for name, ths in thresholds.items():
        out[f"near_cnt/{name}"], out[f"match_cnt/{name}"], out[f"n_in/{name}"] = pc.count(near, inframe, case["counts"], dist, mcount, P, cap, ths,
                                                                                          mode == "rep")
    return out


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("mode", ["rep", "desc"])
@pytest.mark.parametrize("name", sorted(pc.KERNEL_CASES))
def test_kernels_equal_the_restatement(gpu_lib, name, mode):
    case = pc.make_kernel_case(name)
    got, ref = _run_kernels(case, mode, pc.THRESHOLD_LISTS), _restate(case, mode, pc.THRESHOLD_LISTS)
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (name, mode, k)
    # filler rows hold the filler
    P, cap = case["pairs"], case["cap"]
    for img in range(2 * P):
        n = int(case["counts"][img])
        assert not got["warped"][img, n:].any() and not got["inframe"][img, n:].any() and np.isposinf(got["near"][img, n:]).all()
    if mode == "desc":
        for p in range(P):
            assert np.isposinf(got["dist"][:, p, int(case["match_count"][p]):]).all()
    # two calls are identical
    again = _run_kernels(case, mode, pc.THRESHOLD_LISTS)
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), (name, mode, k)
    # pair p of the batch is the pair alone, bit for bit
    for p in range(P):
        alone = _run_kernels(pc.single_pair(case, p), mode, pc.THRESHOLD_LISTS)
        for k in got:
            if k.startswith(("near_cnt", "match_cnt", "n_in")) or k == "dist":
                assert np.array_equal(_bits(got[k][:, p]), _bits(alone[k][:, 0])), (name, mode, k, p)
            else:
                assert np.array_equal(_bits(got[k][[p, P + p]]), _bits(alone[k])), (name, mode, k, p)


def test_corner_error_equals_the_restatement(gpu_lib):
    from xpoint_amd import evaluation as ev
    gt, est, n_inl, mc, H, W = pc.make_corner_case()
    ref = pc.corner_error(gt, est, n_inl, mc, 4, H, W)
    args = (_dev(gt), _dev(est), _dev(n_inl), _dev(mc), 4, H, W)
    got = ev._pe_corner_error(*args).cpu().numpy()
    assert np.array_equal(got, ref) and got[1] == 999.0 and got[2] == 999.0
    assert np.array_equal(_bits(got), _bits(ev._pe_corner_error(*args).cpu().numpy()))
    for p in range(4):
        one = ev._pe_corner_error(_dev(gt[p:p + 1]), _dev(est[p:p + 1]), _dev(n_inl[p:p + 1]), _dev(mc[p:p + 1]), 1, H, W).cpu().numpy()
        assert _bits(one)[0] == _bits(got)[p]


def test_argument_checks(gpu_lib):
    from xpoint_amd import _lib, evaluation as ev
    case = pc.make_kernel_case("ragged")
    kp, counts = _dev(case["kp"]), _dev(case["counts"])
    m1 = _dev(case["maps"]["desc"][0])
    _, inframe, near = ev._pe_warp_near(kp, counts, 3, case["cap"], 24, 40, m1, None, False)
    with pytest.raises(ValueError):
        ev._pe_count(near, inframe, counts, None, None, 3, case["cap"], [], False)
    got = ev._pe_count(near, inframe, counts, None, None, 3, case["cap"], list(range(1, 20)), False)[0]          # 19 thresholds: two launches
    assert got.shape == (2, 3, 19) and (got[..., 1:] >= got[..., :-1]).all()
    with pytest.raises(_lib.XPointHipError, match="pairs"):
        ev._pe_warp_near(kp, counts, 0, case["cap"], 24, 40, m1, None, False)


# ------------------------------------------------------------------------------------------------ against the per-sample path and the reference
def _case(seed):
    c = synth.make_eval_case(seed)
    t = {k: torch.from_numpy(v).cuda() for k, v in c.items()}
    data = {"optical": {"image": torch.zeros(t["prob_optical"].shape), "valid_mask": t["mask_optical"], "homography": t["H_optical"]},
            "thermal": {"image": torch.zeros(t["prob_thermal"].shape), "valid_mask": t["mask_thermal"], "homography": t["H_thermal"]}}
    return c, t, data


def _batched(t, c, cap, ransac=(3,)):
    from xpoint_amd import evaluation as ev
    po, pt = t["prob_optical"] * t["mask_optical"], t["prob_thermal"] * t["mask_thermal"]
    r = ev.pair_metrics_batched(t["prob_optical"], t["prob_thermal"], po, pt, t["desc_optical"], t["desc_thermal"], torch.from_numpy(c["H_optical"]),
                                torch.from_numpy(c["H_thermal"]), 0.015, [1, 3, 5], [2, 4], list(ransac), cap=cap, mask_rep_o=t["mask_optical"],
                                mask_rep_t=t["mask_thermal"])
    return r, ev.download_pair_metrics([r])[0]


@pytest.fixture(scope="module")
def per_sample():
    """The per-sample functions on make_eval_case(0 / 1), computed once."""
    from xpoint_amd import evaluation as ev
    out = {}
    for seed in (0, 1):
        c, t, data = _case(seed)
        po, pt = t["prob_optical"] * t["mask_optical"], t["prob_thermal"] * t["mask_thermal"]
        out[seed] = dict(rep=ev.compute_repeatability_for_sample({"prob": t["prob_optical"]}, {"prob": t["prob_thermal"]}, data, t["H_optical"],
                                                                 t["H_thermal"], 0.015, [1, 3, 5]),
                         desc=ev.compute_descriptor_for_sample(po, pt, t["desc_optical"], t["desc_thermal"], data, CONFIG, 0.015, [2, 4]),
                         pts=ev.compute_pts_dist_for_sample(po, pt, t["desc_optical"], t["desc_thermal"], data, CONFIG, 0.015, [3]))
    return out


@pytest.mark.parametrize("cap", [None, 384])
@pytest.mark.parametrize("seed", [0, 1])
def test_pair_metrics_equal_the_per_sample_path_and_the_reference(gpu_lib, golden, per_sample, seed, cap):
    from xpoint_amd import evaluation as ev
    g = golden("g13_eval_metrics.npz")
    c, t, _ = _case(seed)
    _, r = _batched(t, c, cap)
    assert not bool(r["overflow"])
    rep, nko, nkt = ev.repeatability_from_batch(r, [1, 3, 5], True)
    ref_rep, ref_nko, ref_nkt = per_sample[seed]["rep"]
    assert rep == ref_rep and nko == ref_nko and nkt == ref_nkt
    assert nko == g[f"s{seed}/rep/n_kp_optical"].tolist() and nkt == g[f"s{seed}/rep/n_kp_thermal"].tolist()
    for th in (1, 3, 5):
        assert np.allclose(np.array(rep[th]), g[f"s{seed}/rep/{th}"], rtol=0, atol=1e-12), (th, rep[th])
    dd, ref_dd = ev.descriptor_from_batch(r, [2, 4], True), per_sample[seed]["desc"]
    for th in (2, 4):
        assert set(dd[th]) == set(ref_dd[th])
        for k in ref_dd[th]:
            assert dd[th][k] == ref_dd[th][k], (th, k)                            # counts, tp lists, M-scores AND the distance lists: ==
        for k in ("n_gt_optical", "n_gt_thermal"):
            assert dd[th][k] == int(g[f"s{seed}/desc/{th}/{k}"]), (th, k)
        for k in ("tp_optical", "tp_thermal", "matching_kp_numbers"):
            assert [float(v) for v in dd[th][k]] == g[f"s{seed}/desc/{th}/{k}"].tolist(), (th, k)
        for k in ("distance_optical", "distance_thermal", "m_score_optical", "m_score_thermal"):
            assert np.allclose(np.array(dd[th][k], np.float64), g[f"s{seed}/desc/{th}/{k}"], rtol=0, atol=1e-5), (th, k)
    res = ev.compute_desc_dict(dd)
    for th in (2, 4):
        for k in ("nn_map_optical", "nn_map_thermal", "nn_map", "m_score"):
            assert abs(float(res[th][k]) - float(g[f"s{seed}/res/{th}/{k}"])) < 1e-5, (th, k)


@pytest.mark.parametrize("seed", [0, 1])
def test_corner_error_of_a_batch(gpu_lib, per_sample, seed):
    """Sample 0 draws its hypotheses as pair 0, as the per-sample path always does: the same estimate, hence the same error.  The other samples:
    the restatement applied to what find_homography_batched returns for the per-sample path's own correspondences (bit for bit).

    The bar for sample 0: the per-sample path warps the four points with a BLAS matrix product, which may fuse multiply and add, the kernel
    evaluates the written order; each warped coordinate (magnitude below 2^8 on this frame) then differs by at most a few units of 2^-52 * 2^8
    = 5.7e-14, and the difference of two warped points, the norm and the mean of four keep that order: 1e-11 leaves a factor above 20."""
    from xpoint_amd import evaluation as ev, utils
    c, t, _ = _case(seed)
    _, r = _batched(t, c, None)
    B, _, H, W = c["prob_optical"].shape
    print("corner error, sample 0: batched", repr(float(r["corner_error"][0, 0])), "per sample", repr(float(per_sample[seed]["pts"][3][0])))
    assert r["corner_error"].shape == (1, B) and abs(r["corner_error"][0, 0] - per_sample[seed]["pts"][3][0]) <= 1e-11
    assert per_sample[seed]["pts"][3][0] < 999.0
    po, pt = t["prob_optical"] * t["mask_optical"], t["prob_thermal"] * t["mask_thermal"]
    cap = r["match_dist"].shape[2]
    src = torch.zeros((B, cap, 2)).cuda(); dst = torch.zeros((B, cap, 2)).cuda()
    n = []
    for b in range(B):
        ko, kt = torch.nonzero(po[b, 0] > 0.015), torch.nonzero(pt[b, 0] > 0.015)
        m_o, _ = ev._mutual_matches(utils.interpolate_descriptors(ko, t["desc_optical"][b], H, W), utils.interpolate_descriptors(kt, t["desc_thermal"][b], H, W))
        n.append(len(m_o))
        src[b, :n[b]] = ko[[m[0] for m in m_o]].flip(-1).float(); dst[b, :n[b]] = kt[[m[1] for m in m_o]].flip(-1).float()
    assert n == r["match_count"].tolist() and min(n) >= 4
    H_est, _, n_inl = utils.find_homography_batched(src, dst, torch.tensor(n, dtype=torch.int32).cuda(), 3)
    assert np.array_equal(H_est.cpu().numpy(), r["H_est"][0]) and np.array_equal(n_inl.cpu().numpy(), r["n_inliers"][0])
    gt = ev.pair_eval_matrices(torch.from_numpy(c["H_optical"]), torch.from_numpy(c["H_thermal"]))[3]
    ref = pc.corner_error(gt, r["H_est"][0].reshape(B, 9), r["n_inliers"][0], r["match_count"], B, H, W)
    assert np.array_equal(r["corner_error"][0], ref) and (ref < 999.0).all()


def _same_tree(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _same_tree(a[k], b[k], f"{path}/{k}")
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), path


class _FixedNet:
    """A 'network' that returns the heat maps and descriptor maps of make_eval_case: compute_metrics' loop without a forward."""

    def __init__(self, tensors):
        self.t = tensors

    def takes_pair(self):
        return True

    def __call__(self, data):
        return ({"prob": self.t["prob_optical"].clone(), "desc": self.t["desc_optical"]},
                {"prob": self.t["prob_thermal"].clone(), "desc": self.t["desc_thermal"]}, None)


class _EvalCaseNet(_FixedNet):
    """make_eval_case(0), then (1), in turn: the outputs for the batches of _eval_case_loader."""

    def __init__(self):
        self.i = 0
        self.cases = [_case(s) for s in (0, 1)]

    def __call__(self, data):
        self.t = self.cases[self.i % 2][1]
        self.i += 1
        return super().__call__(data)


def _eval_case_loader():
    for s in (0, 1):
        c = synth.make_eval_case(s)
        yield {spec: {"image": torch.zeros(c[f"prob_{spec}"].shape), "valid_mask": torch.from_numpy(c[f"mask_{spec}"]),
                      "homography": torch.from_numpy(c[f"H_{spec}"])} for spec in ("optical", "thermal")}


def test_compute_metrics_is_the_three_per_sample_functions_with_one_match_per_sample(gpu_lib, per_sample, monkeypatch):
    """compute_metrics over the two eval-case batches (no NMS) against dictionaries assembled by hand from separate calls of
    compute_repeatability_for_sample, compute_descriptor_for_sample and compute_pts_dist_for_sample (the `per_sample` fixture): equal, the
    homography part included (the per-sample path estimates every sample as pair 0, so every entry is the same draw).  During the call the
    matcher is entered once per sample: the descriptor metrics and the corner error share one sampling and one match."""
    from xpoint_amd import evaluation as ev, utils
    config = {"prediction": dict(CONFIG["prediction"], nms=0, topk=0)}
    calls = []
    matcher = utils.match_descriptors

    def counted(*args, **kwargs):
        calls.append(1)
        return matcher(*args, **kwargs)
    monkeypatch.setattr(utils, "match_descriptors", counted)
    got = ev.compute_metrics(_EvalCaseNet(), _eval_case_loader(), "cuda", config, 0.015, [1, 3, 5], [2, 4], [1, 2, 3], [3])
    monkeypatch.undo()
    n_samples = sum(synth.make_eval_case(s)["prob_optical"].shape[0] for s in (0, 1))
    assert n_samples >= 4 and len(calls) == n_samples

    nko = per_sample[0]["rep"][1] + per_sample[1]["rep"][1]
    nkt = per_sample[0]["rep"][2] + per_sample[1]["rep"][2]
    rep = {"repeatability_mean": {th: np.mean(per_sample[0]["rep"][0][th] + per_sample[1]["rep"][0][th]) for th in (1, 3, 5)},
           "n_kp_optical": np.mean(nko), "n_kp_thermal": np.mean(nkt)}
    rep["n_kp_avg"] = (rep["n_kp_optical"] + rep["n_kp_thermal"]) / 2.0
    _same_tree(got["repeatability"], rep, "repeatability")
    merged = {th: {k: per_sample[0]["desc"][th][k] + per_sample[1]["desc"][th][k] for k in per_sample[0]["desc"][th]} for th in (2, 4)}
    assert all(isinstance(merged[th][k], int) for th in (2, 4) for k in ("n_gt_optical", "n_gt_thermal"))
    _same_tree(got["descriptor"], ev.compute_desc_dict(merged), "descriptor")
    pts = per_sample[0]["pts"][3] + per_sample[1]["pts"][3]
    assert len(pts) == n_samples
    _same_tree(got["homography"], ev.compute_homography_dict({3: pts}, [1, 2, 3]), "homography")


def test_compute_metrics_batched_equals_compute_metrics_on_the_eval_cases(gpu_lib):
    """Two batches (make_eval_case 0 and 1, non-trivial homographies and masks), no NMS: with reference_quirks the repeatability and descriptor
    dictionaries are compute_metrics' own, and the homography error agrees on the first sample of every batch."""
    from xpoint_amd import evaluation as ev
    config = {"prediction": dict(CONFIG["prediction"], nms=0, topk=0)}
    Net, loader = _EvalCaseNet, _eval_case_loader
    ref = ev.compute_metrics(Net(), loader(), "cuda", config, 0.015, [1, 3, 5], [2, 4], [1, 2, 3], [3])
    got = ev.compute_metrics_batched(Net(), loader(), "cuda", config, 0.015, [1, 3, 5], [2, 4], [1, 2, 3], [3])
    _same_tree(got["repeatability"], ref["repeatability"], "repeatability")
    _same_tree(got["descriptor"], ref["descriptor"], "descriptor")
    assert list(got["homography"]) == [3] and list(got["homography"][3]["h_correctness"]) == list(ref["homography"][3]["h_correctness"])
    assert np.isfinite(got["homography"][3]["average_h_error"]) and got["homography"][3]["average_h_error"] < 999.0
    free = ev.compute_metrics_batched(Net(), loader(), "cuda", config, 0.015, [1, 3, 5], [2, 4], [1, 2, 3], [3], reference_quirks=False)
    assert all(free["descriptor"][th]["nn_map"] <= 1.0 + 1e-12 for th in (2, 4))
    assert free["repeatability"]["n_kp_avg"] == ref["repeatability"]["n_kp_avg"]


# ------------------------------------------------------------------------------------------------ end to end
def test_synthetic_model_end_to_end(gpu_lib):
    """tests/test_gpu_evaluation.py::test_compute_metrics_runs_end_to_end's set-up with two batches of 2: the batched path equals compute_metrics
    (NMS on, lists unbounded and bounded by topk); without the reference's overwrites NN-mAP <= 1 and the repeatability is 1."""
    from xpoint_amd import evaluation as ev, models
    H, W = 64, 96
    cfg = synth.xpoint_exp1_config(H, W)
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg), strict=True)
    net = net.to("cuda").eval()

    def loader():
        for s in (0, 1):
            d = synth.to_torch(synth.make_pair_batch(s, 2, H, W))
            d["thermal"]["image"] = d["optical"]["image"].clone()
            yield d
    for topk in (0, 200):
        config = {"prediction": dict(CONFIG["prediction"], nms=4, topk=topk, cpu_nms=False)}
        with torch.no_grad():
            ref = ev.compute_metrics(net, loader(), "cuda", config, 0.015, [1, 3], [2], [2], [3])
            got = ev.compute_metrics_batched(net, loader(), "cuda", config, 0.015, [1, 3], [2], [2], [3])
        _same_tree(got["repeatability"], ref["repeatability"], "repeatability")
        _same_tree(got["descriptor"], ref["descriptor"], "descriptor")
        assert got["repeatability"]["repeatability_mean"][1] == 1.0 and abs(got["descriptor"][2]["m_score"] - 1.0) < 1e-9
        assert got["homography"][3]["average_h_error"] < 1e-6 and got["homography"][3]["h_correctness"]["epsilon_warp_th2"] == 1.0
    with torch.no_grad():
        free = ev.compute_metrics_batched(net, loader(), "cuda", config, 0.015, [1, 3], [2], [2], [3], reference_quirks=False)
    assert free["descriptor"][2]["nn_map"] <= 1.0 and free["descriptor"][2]["nn_map"] > 0.99
    assert free["repeatability"]["repeatability_mean"][1] == 1.0 and free["repeatability"]["repeatability_mean"][3] == 1.0


def test_truncated_lists_are_flagged(gpu_lib):
    """A capacity below the longest list truncates it: the result says so (compute_metrics_batched refuses such a batch)."""
    c, t, _ = _case(0)
    r, host = _batched(t, c, 64)
    assert bool(host["overflow"]) and int(host["n_kp"].max()) == 64


# ------------------------------------------------------------------------------------------------ command line and training
def _folder(root, n, tag, H=64, W=96):
    from PIL import Image
    lab = {}
    for i in range(n):
        for spec in ("optical", "thermal"):
            os.makedirs(root / spec, exist_ok=True)
            img = synth.make_image(80 + i, spec, H, W)[0]
            Image.fromarray((img * 255).astype(np.uint8)).save(root / spec / f"p{i}.png")
            ys = synth._hash_int(f"pe/{tag}/{i}/{spec}/y", 40, 0, H - 1); xs = synth._hash_int(f"pe/{tag}/{i}/{spec}/x", 40, 0, W - 1)
            lab[f"p{i}.png/keypoints_{spec}"] = np.stack([ys, xs], 1)
    np.savez(root / "labels.npz", **lab)
    return str(root), str(root / "labels.npz")


def test_cli_benchmark_writes_the_reference_json(gpu_lib, tmp_path, capsys):
    import yaml
    from xpoint_amd import cli
    H, W = 64, 96
    folder, _ = _folder(tmp_path / "data", 4, "cli")
    mcfg = synth.xpoint_exp1_config(H, W, vssm={"EMBED_DIM": 32})
    os.makedirs(tmp_path / "model")
    yaml.safe_dump({"model": mcfg}, open(tmp_path / "model" / "params.yaml", "w"))
    torch.save(synth.make_torch_state_dict(mcfg), tmp_path / "model" / "latest.model")
    yaml.safe_dump({"dataset": {"type": "ImagePairDataset", "foldername": folder, "height": H, "width": W},
                    "prediction": {"detection_threshold": 0.015, "nms": 4, "cpu_nms": True, "topk": 0, "reprojection_threshold": 3, "allow_gpu": True,
                                   "batchsize": 2, "num_worker": 0}}, open(tmp_path / "cfg.yaml", "w"))
    res = cli.main(["benchmark", "-y", str(tmp_path / "cfg.yaml"), "-m", str(tmp_path / "model"), "-v", "latest", "-o", str(tmp_path / "out" / "b.json")])
    printed = capsys.readouterr().out
    for line in ("Repeatability: ", "Number of optical keypoints: ", "th kp : 1, NN-mAP: ", "th kp : 10, M-Score: ", "Homography correctness: "):
        assert line in printed, line
    back = json.load(open(tmp_path / "out" / "b.json"))
    assert back == res
    assert {"repeatability", "descriptor", "homography", "model_dir", "model_version", "height-width", "dataset", "nms", "detection_th",
            "threshold_keypoints_for_descriptor", "threshold_homography_epsilon", "threshold_repeatability_distance_th",
            "ransac_reproj_thresholds"} == set(back)
    ths = [str(t) for t in range(1, 11)]
    assert list(back["repeatability"]["repeatability_mean"]) == ths and list(back["descriptor"]) == [f"th_kp_{t}" for t in ths]
    assert all(set(v) == {"nn_map", "m_score"} and 0.0 <= v["m_score"] <= 1.0 for v in back["descriptor"].values())
    assert list(back["homography"]) == ["2"] and list(back["homography"]["2"]["h_correctness"]) == [f"epsilon_warp_th{t}" for t in ths]
    rep = [back["repeatability"]["repeatability_mean"][t] for t in ths]
    assert all(0.0 <= a <= b <= 1.0 for a, b in zip(rep, rep[1:])) and back["repeatability"]["n_kp_optical"] > 0
    assert back["height-width"] == "64,96" and back["nms"] == 4 and back["detection_th"] == 0.015 and back["dataset"] == folder


def test_fit_validation_metrics(gpu_lib, tmp_path):
    """Two epochs on tests/test_gpu_fit.py's small fixture with a validation folder: with training.validation.compute_metrics the history and the
    learning curve gain the metrics; without the key none of that appears, and everything else the two runs write is equal (the metrics pass
    moves neither weights nor generators)."""
    from tests.training_cases import AUG_CFG_HM, LOSS_CFG
    from xpoint_amd import training
    H, W = 64, 96
    folder, labels = _folder(tmp_path / "data", 4, "train")
    val_folder, val_labels = _folder(tmp_path / "val", 4, "val")
    mcfg = synth.xpoint_exp1_config(H, W, vssm={"EMBED_DIM": 32, "DEPTHS": [1, 1, 1, 1]})
    mcfg["mixed_precision"] = False
    start = tmp_path / "start.model"
    torch.save(synth.make_torch_state_dict(mcfg), start)
    val = {"compute_validation_loss": True, "every_nth_epoch": 1, "foldername": val_folder, "keypoints": val_labels}
    cfg = {"model": mcfg, "loss": dict(LOSS_CFG, type="XPointLoss"),
           "dataset": {"type": "ImagePairDataset", "foldername": folder, "keypoints_filename": labels, "height": H, "width": W,
                       "augmentation": copy.deepcopy(AUG_CFG_HM)},
           "prediction": {"detection_threshold": 0.015, "nms": 4, "topk": 0},
           "training": {"output_directory": str(tmp_path / "plain"), "n_epochs": 2, "learningrate": 1e-4, "weight_decay": 5e-4, "batchsize": 2,
                        "save_every_n_epoch": 1, "mixed_precision": False, "use_writer": True, "log_every": 1,
                        "scheduler": {"use_scheduler": True, "type": "ExponentialLR", "gamma": 0.5}, "validation": val}}
    plain = training.fit(copy.deepcopy(cfg), weight_file=str(start), seed=3)
    with_m = copy.deepcopy(cfg)
    with_m["training"]["output_directory"] = str(tmp_path / "metrics")
    with_m["training"]["validation"] = dict(val, compute_metrics=True, metric_thresholds=[1, 3])
    hist = training.fit(with_m, weight_file=str(start), seed=3)

    assert set(plain) == {"epoch", "loss", "components", "validation_loss", "validation_components", "learning_rate", "skipped_steps"}
    vm = hist.pop("validation_metrics")
    assert hist == plain
    assert len(vm) == 2
    for m in vm:
        assert set(m) == {"repeatability", "nn_map", "m_score", "h_correctness", "average_h_error", "n_kp_optical", "n_kp_thermal"}
        for name in ("repeatability", "nn_map", "m_score", "h_correctness"):
            assert list(m[name]) == [1, 3] and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in m[name].values()), (name, m[name])
        assert np.isfinite(m["average_h_error"]) and m["n_kp_optical"] > 0
        assert m["repeatability"][1] <= m["repeatability"][3]

    def records(out):
        return [json.loads(line) for line in open(os.path.join(out, "learningcurve.jsonl"))]
    added = {f"validation/{n}_{th}" for n in ("repeatability", "nn_map", "m_score", "h_correctness") for th in (1, 3)}
    ra, rb = records(tmp_path / "plain"), records(tmp_path / "metrics")
    assert len(ra) == len(rb)
    for a, b in zip(ra, rb):
        assert not any(k.startswith("validation/") for k in a["scalars"])
        if b["tag"] == "epoch":
            assert added <= set(b["scalars"])
            assert b["scalars"]["validation/m_score_3"] == vm[b["step"] - 1]["m_score"][3]
            b = dict(b, scalars={k: v for k, v in b["scalars"].items() if k not in added})
        assert a == b
    for name in ("e1.model", "e2.model", "latest.model"):
        x, y = torch.load(tmp_path / "plain" / name, map_location="cpu"), torch.load(tmp_path / "metrics" / name, map_location="cpu")
        assert list(x) == list(y) and all(torch.equal(x[k], y[k]) for k in x), name
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "metrics"))
