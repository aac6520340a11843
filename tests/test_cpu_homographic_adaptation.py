"""CPU (-m "not gpu"): the host side of homographic adaptation (xpoint_amd/homographies.py, cli export) against the REAL reference's
recorded draws (tests/golden/g24_homographic_adaptation.npz, tools/make_golden_ha.py): the RNG call order of sample_homography, the
config merge, the errors, and the CLI's argument handling.  No GPU is touched."""
import json

import numpy as np
import pytest
import torch

from xpoint_amd import homographies as ha
from xpoint_amd import utils


def test_sample_homography_reproduces_the_reference_draws(golden):
    """Seeded as in the fixture, the restatement draws every recorded matrix (pins the shuffle-first order and the full n_scales / n_angles draws)."""
    g = golden("g24_homographic_adaptation.npz")
    cases = sorted({k.split("/")[0] for k in g.files if "/" in k})
    assert len(cases) == 12
    for case in cases:
        cfg = json.loads(str(g[f"{case}/config"]))
        ref = g[f"{case}/homographies"]
        assert ref.shape == (cfg["ha"]["num"] - 1, 3, 3)
        merged = utils.dict_update(json.loads(json.dumps(ha.homography_adaptation_default_config)), cfg["ha"])
        np.random.seed(cfg["seed"])
        H, W = cfg["model"]["H"], cfg["model"]["W"]
        got = np.stack([utils.sample_homography(np.array([H, W]), **merged["homographies"]) for _ in range(len(ref))])
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max(), err_msg=case)


def test_get_perspective_transform_maps_the_corners():
    src = np.array([[0, 0], [0, 63], [95, 63], [95, 0]], np.float32)
    dst = np.array([[3.5, 2.0], [1.0, 60.0], [90.0, 66.0], [97.0, -4.0]], np.float32)
    M = ha.get_perspective_transform(src, dst)
    assert M.dtype == np.float64 and M[2, 2] == 1.0
    p = np.concatenate([src.astype(np.float64), np.ones((4, 1))], 1) @ M.T
    np.testing.assert_allclose(p[:, :2] / p[:, 2:], dst, atol=1e-9)
    np.testing.assert_array_equal(ha.get_perspective_transform(src, src), np.eye(3))


def test_kernel_grid_formula_is_torch_linspace():
    """xp_ha_warp's destination grid (two-sided, fused multiply-add) equals torch.linspace(-1, 1, n) bit for bit."""
    for n in list(range(2, 300)) + [479, 480, 640, 1024, 1081]:
        step = np.float32(2.0) / np.float32(n - 1)
        i = np.arange(n)
        lin = np.where(i < n // 2, np.float64(step) * i - 1.0, 1.0 - np.float64(step) * (n - 1 - i)).astype(np.float32)
        assert np.array_equal(lin, torch.linspace(-1, 1, n).numpy()), n


def test_config_merge_and_errors():
    data = {"optical": {"image": torch.zeros(1, 1, 8, 8)}, "thermal": {"image": torch.zeros(1, 1, 8, 8)}}
    c = ha._config({"num": 3, "homographies": {"max_angle": 1.0}}, True)
    assert c["num"] == 3 and c["aggregation"] == "prod" and c["homographies"]["max_angle"] == 1.0
    assert c["homographies"]["patch_ratio"] == 0.9 and c["erosion_radius"] == 5 and c["min_count"] == 2
    assert ha.homography_adaptation_default_config["homographies"]["max_angle"] == np.pi      # defaults are not written into
    for bad, msg in (({"num": 0}, "num must be larger than 0"), ({"filter_size": 2}, "uneven"),
                     ({"aggregation": "window", "window_size": 3, "filter_size": 3}, "Window aggregation"),
                     ({"aggregation": "max"}, "Unknown aggregation: max")):
        with pytest.raises(ValueError, match=msg):
            utils.homographic_adaptation_multispectral(data, None, bad)
    with pytest.raises(ValueError, match="num must be larger than 0"):
        utils.homographic_adaptation(data["optical"], None, {"num": 0})
    with pytest.raises(ValueError, match="uneven"):
        utils.homographic_adaptation(data["optical"], None, {"filter_size": 4})
    with pytest.raises(KeyError):
        utils.homographic_adaptation_multispectral(data, None, {"aggregation": "window"})         # the reference's missing window_size
    with pytest.raises(RuntimeError, match="GPU only"):
        utils.homographic_adaptation_multispectral(data, None, {"num": 1})
    with pytest.raises(ValueError, match="expected num - 1 = 2"):
        ha._homographies({"num": 3}, (8, 8), [np.eye(3)])


def test_cli_export_arguments(tmp_path, capsys):
    from xpoint_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["--help"])
    h = capsys.readouterr().out
    assert "export" in h and "--chunk" in h and "HDF5" in h and "labels.npz" in h
    (tmp_path / "params.yaml").write_text("model:\n  type: XPoint\n")
    cfg = tmp_path / "export.yaml"
    cfg.write_text("dataset:\n  type: ImagePairDataset\n  filename: training.hdf5\nprediction:\n  nms: 8\n")
    with pytest.raises(SystemExit, match="folder datasets"):
        cli.main(["export", "-y", str(cfg), "-m", str(tmp_path), "-o", str(tmp_path / "labels.npz")])
    with pytest.raises(SystemExit, match="--output"):
        cli.main(["export", "-y", str(cfg), "-m", str(tmp_path)])
