"""CPU: the float64 restatement of the two training losses (tests/losses_f64.py: analytic backward, chunked) pinned by autograd on tiny
shapes away from the kinks and by the real reference's results (tests/golden/g27_losses.npz) at the precision an f32 reference allows
against f64 (1e-5 of each tensor's scale: f32 sums of up to 1e6 terms); the host side of xpoint_amd.losses (imports without a GPU, config
merge, the reference's errors) and the new C-ABI exports."""
import copy

import numpy as np
import pytest
import torch

from tests import losses_f64 as L

TOL = 1e-5


def _close(got, ref, what, tol=TOL):
    got, ref = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, sc = float((got - ref).abs().max()), float(ref.abs().max())
    assert err <= tol * max(sc, 1e-30), (what, err, sc)


def _eager64(d1, d2, w1, w2, v1, v2, thr, mp, mn, lam):
    """the reference's formulation with the whole pair tensor, float64, autograd"""
    B, D, Hc, Wc = d1.shape
    a1, a2 = d1.reshape(B, D, -1), d2.reshape(B, D, -1)
    dist = (w1[:, None, :, :] - w2[:, :, None, :]).float().norm(dim=-1)
    s = (dist <= thr).double()
    dot = torch.matmul(a2.permute(0, 2, 1), a1)
    v = v2[:, :, None] * v1[:, None, :]
    loss = (lam * s * (mp - dot).clamp(min=0) + (1 - s) * (dot - mn).clamp(min=0)) * v
    return (loss.sum((1, 2)) / v.sum((1, 2))).mean()


def test_descriptor_restatement_matches_autograd():
    B, D, Hc, Wc = 2, 16, 3, 4
    gen = torch.Generator().manual_seed(1)
    d1 = torch.randn(B, D, Hc, Wc, generator=gen, dtype=torch.float64) * 0.3
    d2 = torch.randn(B, D, Hc, Wc, generator=gen, dtype=torch.float64) * 0.3
    w1 = L.centres(B, Hc, Wc) + 1.5
    w2 = L.centres(B, Hc, Wc) * 1.02
    v1 = (torch.rand(B, Hc * Wc, generator=gen) > 0.2).double()
    v2 = (torch.rand(B, Hc * Wc, generator=gen) > 0.2).double()
    gp, gn = L.margin_gaps(d1, d2, 1.0, 0.2)
    assert min(gp, gn) > 1e-4                               # away from the kinks
    a1, a2 = d1.clone().requires_grad_(True), d2.clone().requires_grad_(True)
    ref = _eager64(a1, a2, w1, w2, v1, v2, 8.0, 1.0, 0.2, 250.0)
    (2.5 * ref).backward()
    got = L.descriptor_loss64(d1, d2, w1, w2, v1, v2, 8.0, 1.0, 0.2, 250.0, grad=2.5, chunk=5)
    _close(got["loss"], ref.detach(), "loss", 1e-12)
    _close(got["g1"], a1.grad, "g1", 1e-12)
    _close(got["g2"], a2.grad, "g2", 1e-12)
    assert torch.autograd.gradcheck(lambda x, y: _eager64(x, y, w1, w2, v1, v2, 8.0, 1.0, 0.2, 250.0), (a1, a2), eps=1e-7, atol=1e-6)


@pytest.mark.parametrize("kind", [0, 1])
def test_detector_restatement_matches_autograd(kind):
    logits, kp, m, _, _ = L.det_case("ce_w05")
    noise = torch.rand(2, 64, 11, 12, generator=torch.Generator().manual_seed(2))
    x = logits.double().requires_grad_(True)
    label = L.hard_labels(kp, noise)
    valid = L.block_valid(m, 2, 11, 12, x.device)
    if kind == 0:
        lv = torch.nn.functional.cross_entropy(x, label, weight=torch.tensor([1.0] * 64 + [0.5], dtype=torch.float64), reduction="none")
    else:
        ce = torch.nn.functional.cross_entropy(x, label, reduction="none")
        lv = 0.25 * (1 - torch.exp(-ce)) ** 2.0 * ce
    lv = lv * valid
    ref = (lv.sum((1, 2)) / valid.sum((1, 2)).clamp(min=1.0)).mean()
    (1.7 * ref).backward()
    got = L.detector_loss64(logits, kp, m, noise, kind, 0.5, 0.25, 2.0, grad=1.7)
    _close(got["loss"], ref.detach(), "loss", 1e-12)
    _close(got["dlogits"], x.grad, "dlogits", 1e-11)
    assert float(got["counts"][1:].sum()) == 2 * 11 * 12


def _warp64(h, B, Hc, Wc):
    """warp_points_pytorch(centres, h.inverse()) in float64, rounded to float32"""
    if h is None:
        return None
    c = L.centres(B, Hc, Wc).double()
    p = torch.cat((c.flip(-1), torch.ones(B, Hc * Wc, 1, dtype=torch.float64)), -1)
    q = torch.bmm(h.double().inverse(), p.permute(0, 2, 1)).permute(0, 2, 1)
    return (q[:, :, :2] / q[:, :, 2:]).flip(-1).float()


@pytest.mark.parametrize("name", list(L.DESC_CASES))
def test_descriptor_restatement_vs_reference(golden, name):
    g = golden("g27_losses.npz")
    d1, d2, h1, h2, m1, m2, cfg, stride = L.desc_case(name, int(g[f"desc/{name}/seed"]))
    B, D, Hc, Wc = d1.shape
    if h1 is not None:
        assert np.array_equal(h1.numpy(), g[f"desc/{name}/h1"]) and np.array_equal(h2.numpy(), g[f"desc/{name}/h2"])
    use = cfg["descriptor_loss_use_mask"]
    v1 = L.block_valid(m1[:, 0], B, Hc, Wc, "cpu").reshape(B, -1) if (use and m1 is not None) else None
    v2 = L.block_valid(m2[:, 0], B, Hc, Wc, "cpu").reshape(B, -1) if (use and m2 is not None) else None
    got = L.descriptor_loss64(d1, d2, _warp64(h1, B, Hc, Wc), _warp64(h2, B, Hc, Wc), v1, v2, cfg["descriptor_loss_threshold"], 1.0, 0.2, 250.0,
                              want_grads=stride is not None)
    for k in ("loss", "pos", "neg"):
        _close(got[k], g[f"desc/{name}/{k}"], f"{name}/{k}")
    if stride is not None:
        sd, sh, sw = stride
        _close(got["g1"][:, ::sd, ::sh, ::sw], g[f"desc/{name}/g1"], f"{name}/g1")
        _close(got["g2"][:, ::sd, ::sh, ::sw], g[f"desc/{name}/g2"], f"{name}/g2")


@pytest.mark.parametrize("name", list(L.DET_CASES))
def test_detector_restatement_vs_reference(golden, name):
    g = golden("g27_losses.npz")
    logits, kp, m, fn, w = L.det_case(name)
    noise = torch.from_numpy(g[f"noise/{int(g[f'det/{name}/seed'])}/0"])
    got = L.detector_loss64(logits, kp, None if m is None else m[:, 0], noise, 0 if fn == "cross_entropy" else 1, w)
    _close(got["loss"], g[f"det/{name}/loss"], "loss")
    _close(got["dlogits"][:, ::L.LOGIT_STRIDE], g[f"det/{name}/dlogits"], "dlogits")
    n = logits.shape[0] * logits.shape[2] * logits.shape[3]
    counts = [round(float(g[f"det/{name}/c_{k}"]) * n) for k in ("correct_ratio", "TP_ratio", "FP_ratio", "FN_ratio", "TN_ratio")]
    assert got["counts"].tolist() == counts
    _close(got["detector_loss"], g[f"det/{name}/c_detector_loss"], "detector_loss")


def test_losses_module_imports_and_merges_configs():
    from xpoint_amd import losses
    before = copy.deepcopy(losses.XPointLoss.default_config)
    crit = losses.XPointLoss({"lambda": 1.0, "detector_focal_loss": {"gamma": 3.0}})
    assert crit.config["lambda"] == 1.0 and crit.config["lambda_d"] == 250
    assert crit.config["detector_focal_loss"] == {"use": True, "alpha": 0.25, "gamma": 3.0}          # nested merge like dict_update
    assert losses.XPointLoss.default_config == before                                                # the class default is not written to
    assert losses.XPointLoss().config == before
    assert isinstance(crit.detector_loss_fn2, losses.FocalLoss) and crit.detector_loss_fn2.gamma == 3.0
    ce = losses.XPointLoss({"detector_loss_function": "cross_entropy", "detector_dustbin_loss_weight": 0.5})
    assert ce.cross_entropy_weights == [1] * 64 + [0.5] and ce.detector_loss_fn2.dustbin_weight == 0.5
    fl = losses.FocalLoss(alpha=0.5, gamma=2.0)
    x, y = torch.randn(2, 65, 3, 4), torch.randint(0, 65, (2, 3, 4))
    ce0 = torch.nn.functional.cross_entropy(x, y, reduction="none")
    assert torch.allclose(fl(x, y), 0.5 * (1 - torch.exp(-ce0)) ** 2 * ce0)


def test_losses_raise_the_reference_errors():
    from xpoint_amd import losses
    with pytest.raises(ValueError, match="Unsupported detector_loss_function"):
        losses.XPointLoss({"detector_loss_function": "bce"})
    with pytest.raises(ValueError, match="Focal Loss is not enabled"):
        losses.XPointLoss({"detector_focal_loss": {"use": False}})
    with pytest.raises(NotImplementedError, match="cross_entropy_focal_blended"):
        losses.XPointLoss({"detector_loss_function": "cross_entropy_focal_blended"})
    crit = losses.XPointLoss({"detector_handle_multiple_keypoints": "hard_assignment"})
    data = {"optical": {"keypoints": torch.zeros(1, 16, 16), "valid_mask": None}, "thermal": {"keypoints": torch.zeros(1, 16, 16), "valid_mask": None}}
    pred = {"logits": torch.zeros(1, 65, 2, 2), "desc": torch.zeros(1, 64, 2, 2)}
    with pytest.raises(ValueError, match="Both pred2 and data2"):
        crit({"data": data, "pred": pred})
    with pytest.raises(ValueError, match="Both pred2 and data2"):
        crit({"data": data["optical"], "pred": pred, "pred2": pred})
    with pytest.raises(ValueError, match="Encoder similarity"):
        losses.XPointLoss({"use_encoder_similarity": True})({"data": data["optical"], "pred": pred})
    with pytest.raises(ValueError, match="Unsupported detector_handle_multiple_keypoints"):          # the class default, as in the reference
        losses.XPointLoss().detector_loss(None, pred["logits"], torch.zeros(1, 16, 16))
    with pytest.raises(NotImplementedError, match="soft_assignment"):
        losses.XPointLoss({"detector_handle_multiple_keypoints": "soft_assignment"}).detector_loss(None, pred["logits"], torch.zeros(1, 16, 16))
    with pytest.raises(AssertionError, match="Descriptor shapes must match"):
        crit.descriptor_loss(torch.zeros(1, 64, 2, 2), torch.zeros(1, 64, 2, 3), None, None)
    with pytest.raises(AssertionError, match="Homography shapes must match"):
        crit.descriptor_loss(pred["desc"], pred["desc"], torch.eye(3)[None], torch.eye(3)[None].repeat(2, 1, 1))
    with pytest.raises(AssertionError, match="4D"):
        crit.detector_loss(crit.detector_loss_fn2, torch.zeros(65, 2, 2), torch.zeros(1, 16, 16))
    with pytest.raises(NotImplementedError, match="sparse_descriptor_loss"):
        losses.XPointLoss({"sparse_descriptor_loss": True}).descriptor_loss(pred["desc"], pred["desc"], None, None)


def test_loss_symbols_exported_and_sized():
    from xpoint_amd import _lib
    lib = _lib.load()
    names = ("xp_descriptor_loss_workspace_bytes", "xp_descriptor_loss_fwd", "xp_descriptor_loss_bwd", "xp_detector_loss_fwd", "xp_detector_loss_bwd")
    declared = _lib.exported_symbols()
    for n in names:
        assert n in declared and hasattr(lib, n), n
    # the workspace grows linearly in Hc * Wc: no (HW x HW) tensor
    w1 = int(lib.xp_descriptor_loss_workspace_bytes(8, 256, 32, 32))
    w4 = int(lib.xp_descriptor_loss_workspace_bytes(8, 256, 64, 64))
    assert 0 < w1 and w4 <= 4 * w1 + 4096
    assert int(lib.xp_descriptor_loss_workspace_bytes(8, 256, 60, 80)) < 8 * 4800 * 4800 * 4 // 4
    assert lib.xp_descriptor_loss_fwd(None, None, None, None, None, None, 1, 100, 4, 4, 8.0, 1.0, 0.2, 250.0, None, 0, None, None, None) != 0
    assert b"multiple of 16" in lib.xp_last_error()
    assert lib.xp_detector_loss_fwd(None, None, None, None, 1, 4, 4, 2, 1.0, 0.25, 2.0, None, None, None, None, None, None) != 0
    assert b"kind" in lib.xp_last_error()


@pytest.mark.parametrize("key", list(L.EDGE_DESC_CASES))
def test_edge_descriptor_case_preconditions(key):
    """every descriptor case of tests/test_gpu_losses_edges.py is a fair test: no dot within 2e-6 x scale^2 of a margin (four times the
    2^-21 of the split-fp16 dot), no distance within 1e-4 px of the threshold, every sample with a valid pair"""
    gap, tgap = L.assert_edge_preconditions(key)
    assert gap >= L.MARGIN_FLOOR == 2e-6 and tgap >= L.THRESHOLD_FLOOR == 1e-4
    d1, d2, w1, w2, v1, v2, thr = L.edge_desc_inputs(key)
    ref = L.descriptor_loss64(d1, d2, w1, w2, v1, v2, thr, 1.0, 0.2, 250.0)
    assert float(ref["norm"].min()) > 0
    for k in ("sums", "g1", "g2"):
        assert bool(torch.isfinite(ref[k]).all())
    c = L.EDGE_DESC_CASES[key]
    for b, sc in enumerate(c["scales"]):           # the factor really is the sample's scale: unit descriptors times it
        n1 = d1[b].double().norm(dim=0)
        assert float((n1 - sc).abs().max()) <= 1e-6 * max(sc, 1e-30), (key, b)


def test_edge_table_covers_every_instance_and_shape():
    rows = L.EDGE_ROWS
    assert len(rows) == len(set(rows)) == 18
    assert {16, 32, 48, 80, 96, 144, 176, 192, 208, 240} <= {s[1] for s in rows}
    assert {1, 5, 32, 33, 128, 129, 133, 256, 385} <= {s[2] * s[3] for s in rows}
    assert {(d + 63) // 64 * 4 for _, d, _, _ in rows} == {4, 8, 12, 16}                  # every KS instance
    assert (2, 192, 16, 16) in rows and (1, 192, 25, 41) not in rows
    for s in rows + [L.EDGE_NEED_ROW]:
        assert L.EDGE_DESC_CASES[L.row_key(s)]["name"] == "gpu64/" + "_".join(map(str, s))     # what _check_vs_64 names its inputs
    assert L.EDGE_NEED_ROW[1] == 48 and L.EDGE_NEED_ROW[2] * L.EDGE_NEED_ROW[3] == 129
    assert L.EDGE_DET_SHAPES == [(1, 1, 1), (3, 16, 17), (2, 9, 57), (5, 4, 4)]


def test_threshold_gap_is_the_float32_distance_to_the_threshold():
    w1 = torch.tensor([[[0.0, 0.0], [3.0, 4.0]]])
    w2 = torch.tensor([[[0.0, 0.0], [0.0, 9.5]]])
    assert L.threshold_gap(w1, w2, 8.0) == 1.5             # distances 0, 9.5, 5, sqrt(9 + 30.25) = 6.26..
    assert L.threshold_gap(w1, w2, 5.0) == 0.0
    c = L.centres(2, 1, 5)
    assert L.threshold_gap(c, c, 8.0) == 0.0 and L.threshold_gap(c, c, 12.0) == 4.0
    assert isinstance(L.threshold_gap(w1.double(), w2.double(), 8.0), float)


def test_detector_edge_inputs_hit_their_regimes():
    """the saturated tensor's regimes as float64 sees them, and the float64 restatement finite there for every focal parameter"""
    logits, kp, m, noise, label = L.det_saturated()
    assert torch.equal(label, L.hard_labels(kp, noise))
    x, lab = logits.reshape(2, 65, -1), label.reshape(2, -1)
    pred = torch.argmax(torch.softmax(logits, 1), 1).reshape(2, -1)
    assert bool((x.gather(1, lab[:, None])[:, 0, :64] == 60.0).all()) and bool((pred[:, :64] == lab[:, :64]).all())
    assert bool((pred[:, 64:128] == (lab[:, 64:128] + 1) % 65).all())
    assert bool((pred[:, 128:192] == 0).all()) and bool((pred[:, 192:256] == 7).all())
    for alpha, gamma in L.EDGE_DET_FOCAL:
        ref = L.detector_loss64(logits, kp, m, noise, 1, 1.0, alpha, gamma)
        assert all(bool(torch.isfinite(ref[k]).all()) for k in ("total", "dlogits", "loss")), (alpha, gamma)
        assert float(ref["total"].min()) > 0
    ce = L.detector_loss64(logits, kp, None, noise, 0, 1.0)
    per = -torch.log_softmax(logits.double(), 1).gather(1, label[:, None]).squeeze(1).reshape(2, -1)
    assert float(per[:, :64].max()) < 1e-15 and float(per[:, 64:128].min()) > 50.0
    assert abs(float(ce["total"].sum()) - float(per.sum())) <= 1e-12 * float(per.sum())
    kp2, noise2 = L.det_label_ties()
    ref = L.hard_labels(kp2, noise2)
    assert int(ref[0, 1, 1]) == 21 and int(ref[1, 2, 3]) == 5 and int(ref[1, 2, 4]) == 64
    assert float(noise2[1, 5, 2, 4]) < 2.0
