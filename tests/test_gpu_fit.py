"""GPU: the training run xpoint_amd.training.fit and `cli train` on a folder dataset of four synthetic 64 x 96 pairs with a
labels .npz (built as tests/test_gpu_detector_eval.py::_cli_setup builds its data): EMBED_DIM 32, DEPTHS [1, 1, 1, 1], homography head off, batch 2,
photometric and homographic augmentation on.  The files a run writes, the bit-exact resume from e<N>.model + e<N>.optim, the schedule, validation in
eval mode, and the command line with `cli align` on its result."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests.training_cases import AUG_CFG_HM, LOSS_CFG
from xpoint_amd import synth

pytestmark = pytest.mark.gpu

H, W, N = 64, 96, 4
EPOCH_SCALARS = {"loss", "learning_rate", "skipped_steps", "loss/descriptor_loss", "loss/positive_dist", "loss/negative_dist"} | {
    f"loss/{k}{s}" for s in "12" for k in ("correct_ratio", "incorrect_ratio", "TP_ratio", "FP_ratio", "FN_ratio", "TN_ratio", "detector_loss",
                                           "detector_normalized_loss")}


def _folder(root, tag):
    from PIL import Image
    lab = {}
    for i in range(N):
        for spec in ("optical", "thermal"):
            os.makedirs(root / spec, exist_ok=True)
            img = synth.make_image(70 + i, spec, H, W)[0]
            Image.fromarray((img * 255).astype(np.uint8)).save(root / spec / f"p{i}.png")
            ys = synth._hash_int(f"fit/{tag}/{i}/{spec}/y", 40, 0, H - 1); xs = synth._hash_int(f"fit/{tag}/{i}/{spec}/x", 40, 0, W - 1)
            lab[f"p{i}.png/keypoints_{spec}"] = np.stack([ys, xs], 1)
    np.savez(root / "labels.npz", **lab)
    return str(root), str(root / "labels.npz")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The dataset, the start weights and the base configuration; the straight two-epoch run, made once and shared."""
    from xpoint_amd import training
    root = tmp_path_factory.mktemp("fit")
    folder, labels = _folder(root / "data", "train")
    val_folder, val_labels = _folder(root / "val", "val")
    mcfg = synth.xpoint_exp1_config(H, W, vssm={"EMBED_DIM": 32, "DEPTHS": [1, 1, 1, 1]})
    mcfg["mixed_precision"] = False
    start = root / "start.model"
    torch.save(synth.make_torch_state_dict(mcfg), start)
    cfg = {"model": mcfg, "loss": dict(LOSS_CFG, type="XPointLoss"),
           "dataset": {"type": "ImagePairDataset", "foldername": folder, "keypoints_filename": labels, "height": H, "width": W,
                       "augmentation": copy.deepcopy(AUG_CFG_HM)},
           "training": {"output_directory": str(root / "straight"), "n_epochs": 2, "learningrate": 1e-4, "weight_decay": 5e-4, "batchsize": 2,
                        "save_every_n_epoch": 1, "mixed_precision": False, "use_writer": True, "allow_gpu": True, "num_worker": 4, "log_every": 1,
                        "scheduler": {"use_scheduler": True, "type": "ExponentialLR", "gamma": 0.5},
                        "validation": {"compute_validation_loss": False, "every_nth_epoch": 1}}}
    history = training.fit(copy.deepcopy(cfg), weight_file=str(start), seed=3)
    return {"root": root, "cfg": cfg, "start": str(start), "history": history, "val": (val_folder, val_labels)}


def _cfg(setup, out, **training_over):
    cfg = copy.deepcopy(setup["cfg"])
    cfg["training"].update(training_over, output_directory=str(setup["root"] / out))
    return cfg


def _same(a, b):
    a, b = torch.load(a, map_location="cpu"), torch.load(b, map_location="cpu")
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def _records(out):
    return [json.loads(line) for line in open(os.path.join(out, "learningcurve.jsonl"))]


def test_two_epochs_write_the_reference_files(gpu_lib, setup):
    import yaml
    from xpoint_amd import models
    out = setup["root"] / "straight"
    assert {"params.yaml", "e1.model", "e1.optim", "e2.model", "e2.optim", "latest.model", "learningcurve.jsonl"} <= set(os.listdir(out))
    assert set(yaml.safe_load(open(out / "params.yaml"))) == {"model", "loss", "training", "dataset"}
    h = setup["history"]
    assert h["epoch"] == [1, 2] and all(np.isfinite(h["loss"])) and h["skipped_steps"] == [0, 0] and h["validation_loss"] == [None, None]
    assert all(np.isfinite(list(c.values())).all() for c in h["components"])
    assert h["learning_rate"] == [1e-4, 5e-5]                               # ExponentialLR, gamma 0.5, stepped per epoch
    rec = _records(out)
    epochs = [r for r in rec if r["tag"] == "epoch"]
    assert [r["step"] for r in epochs] == [1, 2] and all(set(r["scalars"]) == EPOCH_SCALARS for r in epochs)
    assert [r["scalars"]["learning_rate"] for r in epochs] == [1e-4, 5e-5] and epochs[0]["scalars"]["loss"] == h["loss"][0]
    batches = [r for r in rec if r["tag"] == "batch"]
    assert [r["step"] for r in batches] == [1, 2, 3, 4]                      # log_every 1, two batches of 2 per epoch
    assert all({"batch_loss", "batch_loss/descriptor_loss", "batch_loss/detector_loss1"} <= set(r["scalars"]) for r in batches)
    assert abs(sum(r["scalars"]["batch_loss"] for r in batches[:2]) / 2 - h["loss"][0]) <= 1e-5 * abs(h["loss"][0])
    net = models.XPoint(setup["cfg"]["model"])
    r = net.load_state_dict(torch.load(out / "latest.model", map_location="cpu"), strict=True)
    assert list(r.missing_keys) == [] and list(r.unexpected_keys) == []
    first, last = torch.load(setup["start"]), torch.load(out / "latest.model", map_location="cpu")
    assert list(first) == list(last)
    changed = [k for k in first if not torch.equal(first[k], last[k])]
    assert any(k.startswith("encoder.") for k in changed) and any(k.startswith("detector_head") for k in changed)
    assert _same(out / "e2.model", out / "latest.model") and not _same(out / "e1.model", out / "e2.model")


def test_resume_is_bit_exact(gpu_lib, setup):
    from xpoint_amd import training
    training.fit(_cfg(setup, "one", n_epochs=1), weight_file=setup["start"], seed=3)
    one = setup["root"] / "one"
    assert _same(one / "e1.model", setup["root"] / "straight" / "e1.model")
    h = training.fit(_cfg(setup, "one", n_epochs=2), weight_file=str(one / "e1.model"), seed=3)
    assert h["epoch"] == [2] and h["learning_rate"] == [5e-5] and h["loss"] == setup["history"]["loss"][1:]
    assert _same(one / "latest.model", setup["root"] / "straight" / "latest.model")
    # the reference's restart: the same weights, a fresh optimiser
    training.fit(_cfg(setup, "fresh", n_epochs=2), weight_file=str(one / "e1.model"), seed=3, resume_optimizer=False)
    assert not _same(setup["root"] / "fresh" / "latest.model", setup["root"] / "straight" / "latest.model")


def test_validation_runs_in_eval_mode(gpu_lib, setup):
    from xpoint_amd import training
    folder, labels = setup["val"]
    val = {"compute_validation_loss": True, "every_nth_epoch": 1, "foldername": folder, "keypoints": labels}
    h = training.fit(_cfg(setup, "val", n_epochs=1, validation=val), weight_file=setup["start"], seed=3)
    assert np.isfinite(h["validation_loss"][0]) and "descriptor_loss" in h["validation_components"][0]
    epoch = [r for r in _records(setup["root"] / "val") if r["tag"] == "epoch"][0]["scalars"]
    assert epoch["validation_loss"] == h["validation_loss"][0] and "validation_loss/detector_loss1" in epoch
    # validation moved nothing: every tensor, the BatchNorm running statistics and batch counts included, is the run's without validation
    assert _same(setup["root"] / "val" / "e1.model", setup["root"] / "straight" / "e1.model")
    sd = torch.load(setup["root"] / "val" / "e1.model")
    assert int(sd["detector_head_convolutions.3.num_batches_tracked"]) == 4          # two batches x two spectra, training only


def test_cli_train_then_align(gpu_lib, setup, capsys):
    import yaml
    from xpoint_amd import cli
    cfg = _cfg(setup, "cli")
    path = setup["root"] / "train.yaml"
    yaml.safe_dump(cfg, open(path, "w"))
    h = cli.main(["train", "-y", str(path), "-w", setup["start"], "-s", "3"])
    assert h["loss"] == setup["history"]["loss"]
    out = setup["root"] / "cli"
    assert _same(out / "latest.model", setup["root"] / "straight" / "latest.model")
    pcfg = {"dataset": {k: v for k, v in cfg["dataset"].items() if k != "augmentation"},
            "prediction": {"detection_threshold": 0.015, "nms": 4, "cpu_nms": True, "topk": 0, "reprojection_threshold": 3, "allow_gpu": True,
                           "batchsize": 2, "num_worker": 0}}
    yaml.safe_dump(pcfg, open(setup["root"] / "align.yaml", "w"))
    capsys.readouterr()
    res = cli.main(["align", "-y", str(setup["root"] / "align.yaml"), "-m", str(out), "-v", "latest"])
    assert "0/kp_optical" in res and "keypoints" in capsys.readouterr().out
