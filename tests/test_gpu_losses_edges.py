"""GPU: the fused training losses (csrc/desc_loss.hip, csrc/det_loss.hip) at every kernel instance, ragged shape and saturated input,
against the float64 restatement of tests/losses_f64.py on the host.  Inputs are handed to both sides.  Bar: max |got - ref| <= 1e-4 x
max |ref| of each tensor (norm: 1e-7); integer counters and labels exact.  Every descriptor case first asserts that no pair sits closer
to a jump of the gradient than the kernel's arithmetic resolves (losses_f64.assert_edge_preconditions; the same table is asserted without
a GPU in tests/test_cpu_losses.py).  Each check prints its error before it asserts (pytest -s)."""
import ctypes

import pytest
import torch

from tests import losses_f64 as L
from tests.test_gpu_losses import TOL, _check_vs_64, _close, _geometry

pytestmark = pytest.mark.gpu
IDS = lambda s: "x".join(map(str, s))      # noqa: E731


def _cuda(t):
    return None if t is None else t.cuda()


# ------------------------------------------------------------------------------------------------------------------------------------
# descriptor loss
# ------------------------------------------------------------------------------------------------------------------------------------
def _run_case(key, need=(True, True), lam=250.0):
    """one case of L.EDGE_DESC_CASES through the public operator, every sample's sums, parts, norm and gradients against float64"""
    from xpoint_amd import losses
    L.assert_edge_preconditions(key)
    d1, d2, w1, w2, v1, v2, thr = L.edge_desc_inputs(key)
    ref = L.descriptor_loss64(d1, d2, w1, w2, v1, v2, thr, 1.0, 0.2, lam)
    a1, a2 = d1.cuda().requires_grad_(need[0]), d2.cuda().requires_grad_(need[1])
    total, parts, norm = losses.descriptor_loss_sums(a1, a2, _cuda(w1), _cuda(w2), _cuda(v1), _cuda(v2), thr, 1.0, 0.2, lam)
    (total / norm).mean().backward()
    got = {"total": total.detach(), "parts": parts, "norm": norm, "g1": a1.grad, "g2": a2.grad}
    for t in got.values():
        assert t is None or bool(torch.isfinite(t).all()), key
    _close(norm, ref["norm"], f"{key}/norm", 1e-7)
    for b in range(d1.shape[0]):                       # per sample: a sample of another magnitude must not hide behind its neighbour
        _close(total[b:b + 1], ref["sums"][b:b + 1, 0], f"{key}/{b}/total")
        _close(parts[b], ref["sums"][b, 1:], f"{key}/{b}/parts")
        for a, k, n in ((a1, "g1", need[0]), (a2, "g2", need[1])):
            if n:
                _close(a.grad[b], ref[k][b], f"{key}/{b}/{k}")
            else:
                assert a.grad is None
    return got, ref


@pytest.mark.parametrize("shape", L.EDGE_ROWS, ids=IDS)
def test_descriptor_rows_vs_float64(gpu_lib, shape):
    """D = 16, 32, 48, 80, 96, 144, 176, 192, 208, 240 (KS = 4, 8, 12, 16 with dead k, a dead k-major half and the k < D guard) and
    HW = 1, 5, 32, 33, 128, 129, 133, 256, 385: forward sums, parts, norm and both gradients."""
    key = L.row_key(shape)
    B, _, Hc, Wc = shape
    w1, w2, v1, v2 = _geometry(B, Hc, Wc, 7)
    g = L.geometry(B, Hc, Wc, 7)
    assert all(torch.equal(a.cpu(), b) for a, b in zip((w1, w2, v1, v2), g))       # the table's preconditions are about THESE inputs
    assert L.EDGE_DESC_CASES[key]["name"] == "gpu64/" + "_".join(map(str, shape))
    assert float(v1.sum(1).min()) > 0 and float(v2.sum(1).min()) > 0
    L.assert_edge_preconditions(key)
    _check_vs_64(*shape)


def test_descriptor_single_gradient_d48_hw129(gpu_lib):
    L.assert_edge_preconditions(L.row_key(L.EDGE_NEED_ROW))
    _check_vs_64(*L.EDGE_NEED_ROW, need=(True, False))
    _check_vs_64(*L.EDGE_NEED_ROW, need=(False, True))


@pytest.mark.parametrize("key", ["centres/2x64x1x1", "centres/1x64x1x5"])
def test_descriptor_own_centres(gpu_lib, key):
    """w = v = None at HW = 1 and 5: the kernel's own cell centres and all-valid masks, norm = HW^2 (threshold 12: the centres lie 8 px
    apart, so 8 would put pairs exactly on the threshold and the case's threshold gap at 0)."""
    got, _ = _run_case(key)
    B, _, Hc, Wc = L.EDGE_DESC_CASES[key]["shape"]
    assert got["norm"].tolist() == [float((Hc * Wc) ** 2)] * B


def test_descriptor_partial_layout_two_strips(gpu_lib):
    """B = 2, HW = 256 (two strips), KS = 12: sample 0 inside the batch equals sample 0 alone bit for bit, so the forward partials of
    sample 1 (b * strips * waves + block) do not run into sample 0's, and neither do the gradients."""
    from xpoint_amd import losses
    shape = (2, 192, 16, 16)
    B, D, Hc, Wc = shape
    L.assert_edge_preconditions(L.row_key(shape))
    d1, d2 = (t.cuda() for t in L.case_inputs("gpu64/2_192_16_16", B, D, Hc, Wc, True, 1.0, 0.6))
    w1, w2, v1, v2 = _geometry(B, Hc, Wc, 7)

    def run(sl):
        a1, a2 = d1[sl].clone().requires_grad_(True), d2[sl].clone().requires_grad_(True)
        total, parts, norm = losses.descriptor_loss_sums(a1, a2, w1[sl], w2[sl], v1[sl], v2[sl], 8.0, 1.0, 0.2, 250.0)
        total.sum().backward()
        return total.detach(), parts, norm, a1.grad, a2.grad
    full, again, one, other = run(slice(0, 2)), run(slice(0, 2)), run(slice(0, 1)), run(slice(1, 2))
    for a, b, c, d in zip(full, again, one, other):
        assert torch.equal(a, b)
        assert torch.equal(a[:1], c)
        assert torch.equal(a[1:], d)


def _nan_window(n, pad):
    big = torch.full((pad + n + pad,), float("nan"), dtype=torch.float32, device="cuda")
    return big, ctypes.c_void_p(big.data_ptr() + 4 * pad)


def _window_intact(big, n, pad):
    return bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + n:]).all()) and bool(torch.isfinite(big[pad:pad + n]).all())


@pytest.mark.parametrize("shape", [s for s in L.EDGE_ROWS if s[0] >= 2 and s[1] % 64], ids=IDS)
def test_descriptor_outputs_stay_inside_their_window(gpu_lib, shape):
    """B >= 2 and D no multiple of 64: sums / norm of the forward and dD1 / dD2 of the backward lie in the middle of NaN-filled
    allocations (padding: 64 more k rows than the operand planes are padded by, and 1024 words); every word outside the window is still
    NaN, every word inside is finite and equals what the autograd path returns."""
    from xpoint_amd import _lib, losses
    B, D, Hc, Wc = shape
    HW = Hc * Wc
    L.assert_edge_preconditions(L.row_key(shape))
    d1, d2 = (t.cuda() for t in L.case_inputs("gpu64/" + "_".join(map(str, shape)), B, D, Hc, Wc, True, 1.0, 0.6))
    w1, w2, v1, v2 = _geometry(B, Hc, Wc, 7)
    nbytes = int(gpu_lib.xp_descriptor_loss_workspace_bytes(B, D, Hc, Wc))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    pad, n = 128 * HW + 1024, B * D * HW
    sums, p_sums = _nan_window(B * 3, 1024)
    norm, p_norm = _nan_window(B, 1024)
    g1, p_g1 = _nan_window(n, pad)
    g2, p_g2 = _nan_window(n, pad)
    st = _lib.current_stream(d1)
    _lib.call("xp_descriptor_loss_fwd", _lib.ptr(d1), _lib.ptr(d2), _lib.ptr(w1), _lib.ptr(w2), _lib.ptr(v1), _lib.ptr(v2), B, D, Hc, Wc, 8.0, 1.0, 0.2,
              250.0, _lib.ptr(ws), ctypes.c_size_t(nbytes), p_sums, p_norm, st)
    coef = torch.ones(B, dtype=torch.float32, device="cuda")
    _lib.call("xp_descriptor_loss_bwd", _lib.ptr(coef), B, D, Hc, Wc, 8.0, 1.0, 0.2, 250.0, _lib.ptr(ws), ctypes.c_size_t(nbytes), p_g1, p_g2, st)
    torch.cuda.synchronize()
    assert _window_intact(sums, B * 3, 1024) and _window_intact(norm, B, 1024)
    assert _window_intact(g1, n, pad) and _window_intact(g2, n, pad)
    a1, a2 = d1.clone().requires_grad_(True), d2.clone().requires_grad_(True)
    total, parts, nrm = losses.descriptor_loss_sums(a1, a2, w1, w2, v1, v2, 8.0, 1.0, 0.2, 250.0)
    total.sum().backward()
    assert torch.equal(sums[1024:1024 + B * 3].view(B, 3)[:, 0], total.detach()) and torch.equal(sums[1024:1024 + B * 3].view(B, 3)[:, 1:], parts)
    assert torch.equal(norm[1024:1024 + B], nrm)
    assert torch.equal(g1[pad:pad + n].view(B, D, Hc, Wc), a1.grad) and torch.equal(g2[pad:pad + n].view(B, D, Hc, Wc), a2.grad)


@pytest.mark.parametrize("D", [64, 192])
@pytest.mark.parametrize("which", ["small", "x37", "x3e4"])
def test_descriptor_scales_vs_float64(gpu_lib, which, D):
    """unit descriptors times 2^-10 x 1.37, 37 and 3e4 with the margins left at 1.0 / 0.2: the per-sample power of two (dl_scale_kernel),
    1 / S^2 on the dot and 1 / S on the gradient, against float64 and not only for invariance."""
    got, ref = _run_case(f"{which}/{D}")
    if which == "small":                     # every positive hinge active, no negative one
        assert float(ref["sums"][:, 2].abs().max()) == 0.0 and float(got["parts"][:, 1].abs().max()) == 0.0
        assert float(ref["sums"][:, 1].min()) > 0.0
    else:
        assert float(ref["sums"][:, 2].min()) > 0.0


@pytest.mark.parametrize("D", [64, 192])
def test_descriptor_mixed_batch_vs_float64(gpu_lib, D):
    """sample 0 at scale 1, sample 1 at 2^-7 x 1.1: each sample has its own S, and each is compared with float64 on its own scale."""
    _run_case(f"mixed/{D}")


@pytest.mark.parametrize("D", [64, 192])
def test_descriptor_zero_sample(gpu_lib, D):
    """sample 1 all zeros in both images (m == 0 -> S = 1): neg = 0, pos = lambda_d mp sum_s v_t v_r, gradients exactly 0, nothing NaN;
    sample 0 bit-equal to running alone."""
    from xpoint_amd import losses
    key = f"zero/{D}"
    got, ref = _run_case(key)
    d1, d2, w1, w2, v1, v2, thr = L.edge_desc_inputs(key)
    assert float(d1[1].abs().max()) == 0.0 and float(d2[1].abs().max()) == 0.0
    dy = w1[1, None, :, 0] - w2[1, :, None, 0]
    dx = w1[1, None, :, 1] - w2[1, :, None, 1]
    s = ((dy * dy + dx * dx).sqrt() <= thr).double()
    want = 250.0 * 1.0 * float((s * v2[1, :, None].double() * v1[1, None, :].double()).sum())
    assert want > 0 and float(ref["sums"][1, 1]) == want
    assert float(got["parts"][1, 1]) == 0.0 and float(got["parts"][1, 0]) == want and float(got["total"][1]) == want
    assert int(torch.count_nonzero(got["g1"][1])) == 0 and int(torch.count_nonzero(got["g2"][1])) == 0
    a1, a2 = d1[:1].cuda().requires_grad_(True), d2[:1].cuda().requires_grad_(True)
    total, parts, norm = losses.descriptor_loss_sums(a1, a2, w1[:1].cuda(), w2[:1].cuda(), v1[:1].cuda(), v2[:1].cuda(), thr, 1.0, 0.2, 250.0)
    (total / norm).mean().backward()
    assert torch.equal(total.detach(), got["total"][:1]) and torch.equal(parts, got["parts"][:1]) and torch.equal(norm, got["norm"][:1])
    # (total / norm).mean() divides by B: alone the upstream coefficient is twice the batch's, an exact factor
    assert torch.equal(a1.grad, 2.0 * got["g1"][:1]) and torch.equal(a2.grad, 2.0 * got["g2"][:1])


@pytest.mark.parametrize("D", [64, 192])
def test_descriptor_quarter_masks_vs_float64(gpu_lib, D):
    """cell masks with values in {0, 0.25, 0.5, 1}: times lambda_d = 250 they are fp16 numbers, so g is still exact in the backward and
    the 1e-4 bar holds.  Other mask values are carried with fp16's 2^-11 relative rounding in the backward, as xpoint_amd/losses.py says;
    that is not pinned here."""
    key = f"quarter/{D}"
    _, _, _, _, v1, v2, _ = L.edge_desc_inputs(key)
    for v in (v1, v2):
        assert set(v.unique().tolist()) == {0.0, 0.25, 0.5, 1.0}
    _run_case(key)


def test_descriptor_api_edges(gpu_lib):
    """no kernel runs: D outside the multiples of 16 in [16, 256] and host tensors raise; the workspace query is 0 past 256"""
    from xpoint_amd import _lib, losses
    for D in (8, 24, 272):
        x = torch.zeros(1, D, 2, 2, device="cuda")
        with pytest.raises(_lib.XPointHipError):
            losses.descriptor_loss_sums(x, x)
    with pytest.raises(_lib.XPointHipError):
        losses.descriptor_loss_sums(torch.zeros(1, 64, 2, 2), torch.zeros(1, 64, 2, 2))
    with pytest.raises(_lib.XPointHipError):
        losses.detector_loss_stats(torch.zeros(1, 65, 2, 2), torch.zeros(1, 16, 16), None, torch.zeros(1, 64, 2, 2), 0)
    for D in (272, 320, 1024):
        assert int(gpu_lib.xp_descriptor_loss_workspace_bytes(2, D, 8, 12)) == 0
    for D in range(16, 257, 16):
        for Hc, Wc in ((1, 1), (3, 43), (8, 12)):
            n = int(gpu_lib.xp_descriptor_loss_workspace_bytes(2, D, Hc, Wc))
            assert n > 0 and n % 256 == 0, (D, Hc, Wc, n)


# ------------------------------------------------------------------------------------------------------------------------------------
# detector loss
# ------------------------------------------------------------------------------------------------------------------------------------
def _det_config(kind, w, alpha, gamma):
    if kind == 0:
        return L.det_config("cross_entropy", w)
    return dict(L.det_config("focal_loss", 1.0), detector_focal_loss={"use": True, "alpha": alpha, "gamma": gamma})


def _det_check(tag, logits, kp, m, noise, kind, w=1.0, alpha=0.25, gamma=2.0, grad=3.0):
    """detector_loss_stats and XPointLoss.detector_loss on host inputs against detector_loss64 on the host; returns (total, stats, dlogits, labels)"""
    from xpoint_amd import losses
    ref = L.detector_loss64(logits, kp, m, noise, kind, w, alpha, gamma, grad=grad)
    B, _, Hc, Wc = logits.shape
    x = logits.cuda().requires_grad_(True)
    total, stats = losses.detector_loss_stats(x, kp.cuda(), _cuda(m), noise.cuda(), kind, w, alpha, gamma)
    labels = total.grad_fn.saved_tensors[1]
    assert labels.dtype == torch.int32 and torch.equal(labels.cpu().long().reshape(B, Hc, Wc), ref["labels"]), tag
    (grad * (total / stats[:, 1].float().clamp(min=1.0)).mean()).backward()
    for t in (total, stats, x.grad):
        assert bool(torch.isfinite(t).all()), tag
    _close(total, ref["total"], f"{tag}/total")
    _close(x.grad, ref["dlogits"], f"{tag}/dlogits")
    assert torch.equal(stats[:, 1].cpu(), ref["nvalid"]), tag
    assert torch.equal(stats[:, 2:7].sum(0).cpu(), ref["counts"]), (tag, stats[:, 2:7].sum(0), ref["counts"])
    assert float(stats[:, 3:7].sum()) == B * Hc * Wc
    crit = losses.XPointLoss(_det_config(kind, w, alpha, gamma))
    loss, comp = crit.detector_loss(crit.detector_loss_fn2, logits.cuda(), kp.cuda(), _cuda(m), noise=noise.cuda())
    assert bool(torch.isfinite(loss))
    _close(loss, ref["loss"], f"{tag}/loss")
    n = float(B * Hc * Wc)
    assert [round(comp[k] * n) for k in ("correct_ratio", "TP_ratio", "FP_ratio", "FN_ratio", "TN_ratio")] == ref["counts"].tolist()
    return total.detach(), stats, x.grad, labels


@pytest.mark.parametrize("shape", L.EDGE_DET_SHAPES, ids=IDS)
def test_detector_shapes_vs_float64(gpu_lib, shape):
    """one live thread; two blocks with 16 live threads in the second and two passes of the reduce (HW = 272); three blocks with one live
    thread in the last (HW = 513); B = 5.  Cross entropy with dustbin weight 0.5 and NO mask, focal with the mask of case_masks (which
    leaves the 1 x 1 image without a valid cell) and without one."""
    B, Hc, Wc = shape
    logits, kp, m = L.det_inputs("edge/det/" + IDS(shape), B, Hc, Wc, True)
    noise = L.det_noise(B, Hc, Wc, 1)
    _det_check(f"det/{IDS(shape)}/ce", logits, kp, None, noise, 0, 0.5)
    _det_check(f"det/{IDS(shape)}/focal", logits, kp, m, noise, 1)
    _det_check(f"det/{IDS(shape)}/focal_open", logits, kp, None, noise, 1)


def test_detector_batch_invariance_two_blocks(gpu_lib):
    from xpoint_amd import losses
    B, Hc, Wc = 3, 16, 17
    logits, kp, m = (t.cuda() for t in L.det_inputs("edge/det/3x16x17", B, Hc, Wc, True))
    noise = L.det_noise(B, Hc, Wc, 1).cuda()

    def det(sl, kind):
        x = logits[sl].clone().requires_grad_(True)
        total, stats = losses.detector_loss_stats(x, kp[sl], m[sl], noise[sl], kind, 0.5)
        total.sum().backward()
        return total.detach(), stats, x.grad
    for kind in (0, 1):
        full, again, one, last = det(slice(0, 3), kind), det(slice(0, 3), kind), det(slice(0, 1), kind), det(slice(2, 3), kind)
        for a, b, c, d in zip(full, again, one, last):
            assert torch.equal(a, b)
            assert torch.equal(a[:1], c)
            assert torch.equal(a[2:], d)


SATURATED = [(1, 1.0, a, g) for a, g in L.EDGE_DET_FOCAL] + [(0, 1.0, 0.25, 2.0), (0, 0.5, 0.25, 2.0)]


@pytest.mark.parametrize("kind,w,alpha,gamma", SATURATED, ids=lambda v: str(v))
def test_detector_saturation_and_prediction_ties(gpu_lib, kind, w, alpha, gamma):
    """(2, 16, 17) with whole waves of: the label's logit +60 (ce ~ 0, pt -> 1, q = 0 in f32: the q > 0 guard and powf(q, gamma - 1)), another
    logit +60 (ce ~ 60, pt -> 0), all 65 logits equal (prediction 0) and equal maxima at 7 and 64 (prediction 7); exact ties only.  Focal
    with gamma 2, 0, 1, 0.5, 5 and alpha 0.25, 0.5, 1; cross entropy with dustbin weight 1 and 0.5.  Everything finite, total and dlogits
    at the 1e-4 bar, the counters (which hold the predictions of the tied waves) exact."""
    logits, kp, m, noise, label = L.det_saturated()
    total, stats, dlogits, labels = _det_check(f"sat/{kind}/{w}/{alpha}/{gamma}", logits, kp, m, noise, kind, w, alpha, gamma)
    # the tied waves alone, without a mask: all-equal logits predict class 0, maxima at 7 and 64 predict 7
    from xpoint_amd import losses
    lab = label.reshape(2, -1)
    _, st = losses.detector_loss_stats(logits.cuda(), kp.cuda(), None, noise.cuda(), kind, w, alpha, gamma)
    pred = torch.argmax(torch.softmax(logits.float(), 1), 1).reshape(2, -1)
    assert bool((pred[:, 128:192] == 0).all()) and bool((pred[:, 192:256] == 7).all())
    assert int(st[:, 2].sum()) == int((pred == lab).sum())


def test_detector_label_ties(gpu_lib):
    """noise 0: several keypoints of one cell tie and the first in channel order wins (s > best); no keypoint: 64; noise exactly 2.0 in
    channel 5 of a cell without a keypoint: label 5 (2.0 > best is false); the float32 below 2.0 there: 64.  Exact against hard_labels."""
    kp, noise = L.det_label_ties()
    ref = L.hard_labels(kp, noise)
    assert int(ref[0, 1, 1]) == 21 and int(ref[1, 2, 3]) == 5 and int(ref[1, 2, 4]) == 64
    lab = kp.float().reshape(2, 16, 8, 17, 8).permute(0, 2, 4, 1, 3).reshape(2, 64, 16, 17)
    assert int((lab.sum(1) > 1).sum()) >= 8 and int((lab.sum(1) == 0).sum()) >= 8          # cells with several keypoints, cells with none
    logits, _, _ = L.det_inputs("edge/det/ties", 2, 16, 17, False)
    for kind in (0, 1):
        _, _, _, labels = _det_check(f"ties/{kind}", logits, kp, None, noise, kind)
        assert torch.equal(labels.cpu().long().reshape(2, 16, 17), ref)


def test_detector_all_invalid_sample(gpu_lib):
    """sample 1 with mask 0 everywhere: no valid cell (stats[1, 1] == 0), a finite loss equal to float64's (clamp(min=1)), dlogits[1]
    exactly 0; sample 0 bit-equal to running alone."""
    from xpoint_amd import losses
    B, Hc, Wc = 2, 16, 17
    logits, kp, m = L.det_inputs("edge/det/invalid", B, Hc, Wc, True)
    m = m.clone()
    m[1] = False
    noise = L.det_noise(B, Hc, Wc, 2)
    for kind in (0, 1):
        total, stats, dlogits, _ = _det_check(f"invalid/{kind}", logits, kp, m, noise, kind, 0.5, grad=1.0)
        assert float(stats[1, 1]) == 0.0 and float(stats[0, 1]) > 0.0 and float(total[1]) == 0.0
        assert int(torch.count_nonzero(dlogits[1])) == 0
        x = logits[:1].cuda().requires_grad_(True)
        t1, s1 = losses.detector_loss_stats(x, kp[:1].cuda(), m[:1].cuda(), noise[:1].cuda(), kind, 0.5)
        (t1 / s1[:, 1].float().clamp(min=1.0)).mean().backward()
        assert torch.equal(t1.detach(), total[:1]) and torch.equal(s1, stats[:1])
        assert torch.equal(x.grad, 2.0 * dlogits[:1])             # .mean() over B = 1 instead of 2: an exact factor


assert TOL == 1e-4
