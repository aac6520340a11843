"""Detector evaluation, the part that needs no GPU: the tp/fp rule restated in numpy against the reference's own outputs
(tests/golden/g28_detector_eval.npz), the label files of the dataset, and the C ABI's declarations and argument checks."""
import ctypes
import os

import numpy as np
import pytest

from tests import detector_eval_cases as C
from xpoint_amd import _lib

SYMBOLS = ("xp_detector_eval_claim", "xp_detector_eval_resolve", "xp_detector_eval_gather", "xp_detector_eval_fill_dist")


def tp_fp_rule(prob, kp, zero_threshold=1e-4, distance_thresh=2.0):
    """The rule of xpoint_amd.evaluation.tp_fp_dist_batched in plain numpy, one image: -> (tp, fp, prob sorted, n_gt, dist, order).
    Candidates prob > zero_threshold, ranked by descending prob and, among equals, ascending row-major pixel index; each claims the first
    row-major label within the radius; the best-ranked claimant of a label is the true positive; dist lists every within-radius pair by
    (rank, row-major label)."""
    H, W = prob.shape
    flat = prob.ravel()
    cand = np.flatnonzero(flat > np.float32(zero_threshold))
    order = cand[np.lexsort((cand, -flat[cand].astype(np.float64)))]
    ys, xs = order // W, order % W
    r = int(np.floor(distance_thresh))
    first = np.full(len(order), -1, np.int64)
    pair_rank, pair_dist = [], []
    for dy in range(-r, r + 1):                     # (dy, dx) ascending = the labels of one prediction in row-major order
        for dx in range(-r, r + 1):
            d = np.sqrt(np.float32(dy * dy + dx * dx))
            if not d <= np.float32(distance_thresh):
                continue
            yy, xx = ys + dy, xs + dx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            ok[ok] = kp[yy[ok], xx[ok]]
            idx = np.flatnonzero(ok)
            new = idx[first[idx] < 0]
            first[new] = yy[new] * W + xx[new]
            pair_rank.append(idx); pair_dist.append(np.full(len(idx), d, np.float32))
    tp = np.zeros(len(order), bool)
    claim = np.flatnonzero(first >= 0)              # ascending rank: the first occurrence of a label is its best-ranked claimant
    _, pos = np.unique(first[claim], return_index=True)
    tp[claim[pos]] = True
    pair_rank = np.concatenate(pair_rank) if pair_rank else np.zeros((0,), np.int64)
    pair_dist = np.concatenate(pair_dist) if pair_dist else np.zeros((0,), np.float32)
    dist = pair_dist[np.argsort(pair_rank, kind="stable")]
    return tp, ~tp, flat[order], int(kp.sum()), dist, order


@pytest.mark.parametrize("name", list(C.TP_FP_CASES))
def test_numpy_rule_equals_the_reference(golden, name):
    g = golden("g28_detector_eval.npz")
    prob, kp, thr = C.tp_fp_case(name, int(g["seed"]))
    tp, fp, pr, n_gt, dist, order = tp_fp_rule(prob, kp, C.ZERO_THRESHOLD, thr)
    assert np.array_equal(tp, g[f"tpfp/{name}/tp"]) and np.array_equal(fp, g[f"tpfp/{name}/fp"])
    assert np.array_equal(order, g[f"tpfp/{name}/order"])
    assert np.array_equal(pr, g[f"tpfp/{name}/prob"])
    assert n_gt == int(g[f"tpfp/{name}/n_gt"]) and len(dist) == len(g[f"tpfp/{name}/dist"])
    assert np.allclose(dist, g[f"tpfp/{name}/dist"], rtol=0, atol=1e-6)


def test_fixture_covers_the_cases_it_is_meant_to(golden):
    g = golden("g28_detector_eval.npz")
    seed = int(g["seed"])
    v = C.all_candidate_values(seed)
    assert len(np.unique(v)) == len(v)                                       # no result depends on a sort's order among ties
    n = {name: (len(g[f"tpfp/{name}/tp"]), int(g[f"tpfp/{name}/n_gt"]), int(g[f"tpfp/{name}/tp"].sum())) for name in C.TP_FP_CASES}
    assert n["zero_labels_24x40_t2"][1] == 0 and n["zero_labels_24x40_t2"][0] > 0
    assert n["one_candidate_24x40_t2"][0] == 1 and n["zero_candidates_33x47_t2p5"][0] == 0
    p, k, t = n["exhaust_33x47_t2"]
    assert t == k and len(g["tpfp/exhaust_33x47_t2/dist"]) > k               # every label taken, further predictions within the radius
    prob, kp, thr = C.tp_fp_case("clusters_24x40_t2", seed)
    tp, _, _, _, dist, order = tp_fp_rule(prob, kp, C.ZERO_THRESHOLD, thr)
    assert len(dist) > int((g["tpfp/clusters_24x40_t2/tp"]).sum()) * 2       # predictions see several labels / share labels
    assert kp[0, 0] and kp[-1, -1] and kp[0].sum() > 2 and kp[:, 0].sum() > 2
    assert len(g["rep/list"]) < len(g["rep/n_kp_optical"]) and 0 in g["rep/n_kp_optical"]


def test_rule_tie_break_is_the_lower_pixel_index():
    prob = np.zeros((5, 7), np.float32); kp = np.zeros((5, 7), bool)
    kp[2, 3] = True
    prob[2, 4] = prob[2, 2] = 0.5            # both one pixel from the label
    tp, fp, pr, n_gt, dist, order = tp_fp_rule(prob, kp)
    assert order.tolist() == [2 * 7 + 2, 2 * 7 + 4] and tp.tolist() == [True, False] and dist.tolist() == [1.0, 1.0]


def _folder(tmp_path, names, H, W):
    from PIL import Image
    rng = np.random.default_rng(5)
    for spec in ("optical", "thermal"):
        os.makedirs(tmp_path / "data" / spec)
        for n in names:
            Image.fromarray(rng.integers(0, 256, (H, W), dtype=np.uint8)).save(tmp_path / "data" / spec / n)
    return str(tmp_path / "data")


def test_dataset_reads_exported_label_files(tmp_path):
    import random
    from xpoint_amd.datasets import ImagePairDataset
    H, W = 80, 112
    names = ["a.png", "b.png"]
    folder = _folder(tmp_path, names, H, W)
    pts = {"a.png": np.array([[0, 0], [10, 20], [79, 111], [40, 50], [33, 34]]), "b.png": np.zeros((0, 2), np.int64)}
    pts_t = {"a.png": np.array([[5, 6], [70, 100]]), "b.png": np.array([[1, 2]])}
    np.savez(tmp_path / "one.npz", **{f"{n}/keypoints": pts[n] for n in names})
    np.savez(tmp_path / "two.npz", **{f"{n}/keypoints_optical": pts[n] for n in names}, **{f"{n}/keypoints_thermal": pts_t[n] for n in names})
    # no crop: the maps are the points as they are, one list serves both spectra
    ds = ImagePairDataset({"foldername": folder, "keypoints_filename": str(tmp_path / "one.npz")})
    s = ds[0]
    for spec in ("optical", "thermal"):
        m = s[spec]["keypoints"]
        assert m.dtype.is_floating_point is False and tuple(m.shape) == (H, W) and str(m.dtype) == "torch.bool"
        assert sorted(map(tuple, np.argwhere(m.numpy()).tolist())) == sorted(map(tuple, pts["a.png"].tolist()))
    assert int(ds[1]["optical"]["keypoints"].sum()) == 0
    # a crop: shifted by its origin, the points outside dropped; one list per spectrum
    ds = ImagePairDataset({"foldername": folder, "keypoints_filename": str(tmp_path / "two.npz"), "height": 64, "width": 96})
    random.seed(11)
    i_h, i_w = random.randint(0, H - 64), random.randint(0, W - 96)
    random.seed(11)
    s = ds[0]
    for spec, src in (("optical", pts["a.png"]), ("thermal", pts_t["a.png"])):
        want = src - np.array([[i_h, i_w]])
        want = want[(want[:, 0] >= 0) & (want[:, 0] < 64) & (want[:, 1] >= 0) & (want[:, 1] < 96)]
        got = np.argwhere(s[spec]["keypoints"].numpy())
        assert tuple(s[spec]["keypoints"].shape) == (64, 96) == tuple(s[spec]["image"].shape[1:])
        assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist())), spec
    assert (i_h, i_w) != (0, 0) and int(s["optical"]["keypoints"].sum()) < len(pts["a.png"])         # the crop moved and dropped points
    # a sample without labels in the file is an error at construction, as in the reference
    np.savez(tmp_path / "short.npz", **{"a.png/keypoints": pts["a.png"]})
    with pytest.raises(IndexError, match="b.png"):
        ImagePairDataset({"foldername": folder, "keypoints_filename": str(tmp_path / "short.npz")})


def test_dataset_still_rejects_what_it_does_not_read(tmp_path):
    from xpoint_amd.datasets import ImagePairDataset
    folder = _folder(tmp_path, ["a.png"], 64, 64)
    with pytest.raises(NotImplementedError, match="h5py"):
        ImagePairDataset({"foldername": folder, "keypoints_filename": str(tmp_path / "labels.hdf5")})
    with pytest.raises(NotImplementedError):
        ImagePairDataset({"foldername": folder, "single_image": True})
    with pytest.raises(NotImplementedError):
        ImagePairDataset({"filename": str(tmp_path / "x.hdf5")})
    assert "keypoints" not in ImagePairDataset({"foldername": folder})[0]["optical"]


def test_detector_eval_symbols_declared_and_exported():
    lib = _lib.load()
    declared = _lib.exported_symbols()
    for n in SYMBOLS:
        assert n in declared and n in _lib._SIGNATURES and hasattr(lib, n), n


def test_detector_eval_argument_errors_name_the_argument():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))           # never dereferenced: every call below fails its checks before any launch

    def err(rc):
        assert rc != 0
        return lib.xp_last_error().decode()
    assert "distance_thresh" in err(lib.xp_detector_eval_claim(p, p, 1, 4, 4, 1e-4, 9.0, p, p, p, p, p, p, None))
    assert "distance_thresh" in err(lib.xp_detector_eval_claim(p, p, 1, 4, 4, 1e-4, -0.5, p, p, p, p, p, p, None))
    assert "distance_thresh" in err(lib.xp_detector_eval_claim(p, p, 1, 4, 4, 1e-4, float("nan"), p, p, p, p, p, p, None))
    assert "distance_thresh" in err(lib.xp_detector_eval_fill_dist(p, p, p, p, 1, 4, 4, 9.0, p, 1, None))
    assert "zero_threshold" in err(lib.xp_detector_eval_claim(p, p, 1, 4, 4, -1.0, 2.0, p, p, p, p, p, p, None))
    assert "H * W" in err(lib.xp_detector_eval_claim(p, p, 1, 1 << 17, 1 << 17, 1e-4, 2.0, p, p, p, p, p, p, None))
    assert "batch" in err(lib.xp_detector_eval_claim(p, p, 0, 4, 4, 1e-4, 2.0, p, p, p, p, p, p, None))
    names = ("prob", "labels", "cand_prob", "winner", "first_label", "n_within", "n_cand", "n_gt")
    for i, name in enumerate(names):
        a = [p] * 8
        a[i] = None
        msg = err(lib.xp_detector_eval_claim(a[0], a[1], 1, 4, 4, 1e-4, 2.0, *a[2:], None))
        assert "null pointer" in msg and msg.rstrip().endswith(name), msg
    assert "tp_pix" in err(lib.xp_detector_eval_resolve(p, p, p, 1, 4, 4, None, None))
    assert "rank_pix" in err(lib.xp_detector_eval_gather(None, p, p, p, 1, 4, 4, p, p, None))
    assert "n_cand" in err(lib.xp_detector_eval_gather(p, p, p, None, 1, 4, 4, p, p, None))
    assert "incl" in err(lib.xp_detector_eval_fill_dist(p, p, None, p, 1, 4, 4, 2.0, p, 1, None))
    assert "dist_len" in err(lib.xp_detector_eval_fill_dist(p, p, p, p, 1, 4, 4, 2.0, p, -1, None))


def test_host_helpers():
    from xpoint_amd import evaluation, utils
    m = utils.generate_keypoint_map(np.array([[1.9, 2.2], [0, 0]]), (3, 4))
    assert m.dtype == bool and np.argwhere(m).tolist() == [[0, 0], [1, 2]]
    assert utils.generate_keypoint_map(np.zeros((0, 2)), (3, 4)).sum() == 0
    assert evaluation._div0_one(np.array([0, 1]), 0).tolist() == [1.0, 0.0]          # the reference evaluation.py div0: 0 / 0 -> 1
    with pytest.raises(ValueError, match="GPU"):
        evaluation.tp_fp_dist_batched(np.zeros((1, 4, 4), np.float32), np.zeros((1, 4, 4), bool))
