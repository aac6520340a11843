"""GPU: the fused training losses (xpoint_amd.losses, csrc/desc_loss.hip, csrc/det_loss.hip) against the real reference's results
(tests/golden/g27_losses.npz, tools/make_golden_losses.py) and against the float64 restatement of tests/losses_f64.py.  Bar for losses and
gradients: max |got - ref| <= 1e-4 x max |ref| of each tensor (the project's f32 bar: README); integer counters exact."""
import numpy as np
import pytest
import torch

from tests import losses_f64 as L

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _close(got, ref, what, tol=TOL):
    got = torch.as_tensor(np.asarray(got.detach().cpu() if torch.is_tensor(got) else got)).double()
    ref = torch.as_tensor(np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref)).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, sc = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: max err {err:.3e}, scale {sc:.3e}, ratio {err / max(sc, 1e-300):.2e}")
    assert err <= tol * max(sc, 1e-30), (what, err, sc)


def _cuda(t):
    return None if t is None else t.cuda()


@pytest.mark.parametrize("name", list(L.DESC_CASES))
def test_descriptor_loss_vs_reference(gpu_lib, golden, name):
    from xpoint_amd import losses
    g = golden("g27_losses.npz")
    d1, d2, h1, h2, m1, m2, cfg, stride = L.desc_case(name, int(g[f"desc/{name}/seed"]))
    crit = losses.XPointLoss(dict(cfg, detector_handle_multiple_keypoints="hard_assignment"))
    a1, a2 = d1.cuda().requires_grad_(True), d2.cuda().requires_grad_(True)
    loss, pos, neg = crit.descriptor_loss(a1, a2, _cuda(h1), _cuda(h2), _cuda(m1), _cuda(m2))
    for k, v in (("loss", loss), ("pos", pos), ("neg", neg)):
        _close(v, g[f"desc/{name}/{k}"], f"{name}/{k}")
    if stride is not None:
        loss.backward()
        sd, sh, sw = stride
        _close(a1.grad[:, ::sd, ::sh, ::sw], g[f"desc/{name}/g1"], f"{name}/g1")
        _close(a2.grad[:, ::sd, ::sh, ::sw], g[f"desc/{name}/g2"], f"{name}/g2")


COMPONENTS = ("correct_ratio", "incorrect_ratio", "TP_ratio", "FP_ratio", "FN_ratio", "TN_ratio", "detector_loss", "detector_normalized_loss")


@pytest.mark.parametrize("name", list(L.DET_CASES))
def test_detector_loss_vs_reference(gpu_lib, golden, name):
    from xpoint_amd import losses
    g = golden("g27_losses.npz")
    logits, kp, m, fn, w = L.det_case(name)
    noise = torch.from_numpy(g[f"noise/{int(g[f'det/{name}/seed'])}/0"]).cuda()
    crit = losses.XPointLoss(L.det_config(fn, w))
    n = logits.shape[0] * logits.shape[2] * logits.shape[3]
    for kp_t, m_t in ((kp, m), (kp.to(torch.uint8), None if m is None else m.float())):          # bool, uint8 and float inputs
        x = logits.cuda().requires_grad_(True)
        loss, comp = crit.detector_loss(crit.detector_loss_fn2, x, kp_t.cuda(), _cuda(m_t), noise=noise)
        loss.backward()
        _close(loss, g[f"det/{name}/loss"], f"{name}/loss")
        _close(x.grad[:, ::L.LOGIT_STRIDE], g[f"det/{name}/dlogits"], f"{name}/dlogits")
        assert set(comp) == set(COMPONENTS)
        for k in COMPONENTS:
            ref = float(g[f"det/{name}/c_{k}"])
            assert isinstance(comp[k], float)
            if k.endswith("_ratio"):                      # integer counters behind the ratios: exact
                assert round(comp[k] * n) == round(ref * n), (k, comp[k], ref)
            else:
                assert abs(comp[k] - ref) <= TOL * abs(ref), (k, comp[k], ref)


@pytest.mark.parametrize("name", list(L.FORWARD_CASES))
def test_forward_vs_reference(gpu_lib, golden, name):
    from xpoint_amd import losses, utils
    g = golden("g27_losses.npz")
    seed = int(g[f"fwd/{name}/seed"])
    data, pred, pred2 = L.forward_case(name, seed)
    data = utils.data_to_device(data, "cuda")
    for p in (pred, pred2):
        for k in p:
            p[k] = p[k].cuda().requires_grad_(True)
    crit = losses.XPointLoss(L.FORWARD_CASES[name])
    # the reference drew its noise from the global generator; feed the stored draws through the same entry point
    draws = [torch.from_numpy(g[f"noise/{seed}/{k}"]).cuda() for k in (0, 1)]
    orig = crit.detector_loss
    crit.detector_loss = lambda fn, lg, kp, vm=None: orig(fn, lg, kp, vm, noise=draws.pop(0))
    loss, comp = crit({"data": data, "pred": pred, "pred2": pred2})
    loss.backward()
    _close(loss, g[f"fwd/{name}/loss"], f"{name}/loss")
    keys = [k[len(f"fwd/{name}/c_"):] for k in g.files if k.startswith(f"fwd/{name}/c_")]
    assert set(comp) == set(keys)
    n = pred["logits"].shape[0] * pred["logits"].shape[2] * pred["logits"].shape[3]
    for k in keys:
        ref = float(g[f"fwd/{name}/c_{k}"])
        if "_ratio" in k:
            assert round(comp[k] * n) == round(ref * n), (k, comp[k], ref)
        else:
            assert abs(comp[k] - ref) <= TOL * abs(ref), (k, comp[k], ref)
    _close(pred["logits"].grad[:, ::L.LOGIT_STRIDE], g[f"fwd/{name}/g_logits1"], f"{name}/g_logits1")
    _close(pred2["logits"].grad[:, ::L.LOGIT_STRIDE], g[f"fwd/{name}/g_logits2"], f"{name}/g_logits2")
    _close(pred["desc"].grad[:, ::L.FWD_DESC_STRIDE], g[f"fwd/{name}/g_desc1"], f"{name}/g_desc1")
    _close(pred2["desc"].grad[:, ::L.FWD_DESC_STRIDE], g[f"fwd/{name}/g_desc2"], f"{name}/g_desc2")


def _geometry(B, Hc, Wc, seed):
    """the test's own float32 coordinates, handed to both sides: cell centres moved by a smooth field of a few pixels"""
    return tuple(t.cuda() for t in L.geometry(B, Hc, Wc, seed))


def _check_vs_64(B, D, Hc, Wc, need=(True, True), grad=1.0, lam=250.0, thr=8.0, dtype=torch.float32, noncontig=False, tol=TOL):
    from xpoint_amd import losses
    d1, d2 = L.case_inputs(f"gpu64/{B}_{D}_{Hc}_{Wc}", B, D, Hc, Wc, True, 1.0, 0.6)
    d1, d2 = d1.cuda().to(dtype), d2.cuda().to(dtype)
    if noncontig:
        d1 = d1.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        d2 = d2.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    w1, w2, v1, v2 = _geometry(B, Hc, Wc, 7)
    ref = L.descriptor_loss64(d1, d2, w1, w2, v1, v2, thr, 1.0, 0.2, lam, grad=grad, chunk=512)
    a1, a2 = d1.clone().requires_grad_(need[0]), d2.clone().requires_grad_(need[1])
    total, parts, norm = losses.descriptor_loss_sums(a1, a2, w1, w2, v1, v2, thr, 1.0, 0.2, lam)
    tag = f"{B}x{D}x{Hc}x{Wc}"
    _close(total, ref["sums"][:, 0], tag + "/total", tol)
    _close(parts, ref["sums"][:, 1:], tag + "/parts", tol)
    _close(norm, ref["norm"], tag + "/norm", 1e-7)
    (grad * (total / norm).mean()).backward()
    for a, k, n in ((a1, "g1", need[0]), (a2, "g2", need[1])):
        if n:
            assert a.grad.dtype == dtype
            # an fp16 input gets its gradient back in fp16: one more rounding, half an ulp = 2^-11 of the element, at most of the scale
            _close(a.grad, ref[k], tag + "/" + k, tol if dtype == torch.float32 else tol + 2.0 ** -11)
        else:
            assert a.grad is None


@pytest.mark.parametrize("shape", [(1, 64, 8, 12), (3, 128, 32, 32), (1, 256, 25, 41), (1, 256, 60, 80), (3, 64, 60, 80)],
                         ids=lambda s: "x".join(map(str, s)))
def test_descriptor_loss_vs_float64(gpu_lib, shape):
    _check_vs_64(*shape)


def test_descriptor_loss_variants_vs_float64(gpu_lib):
    _check_vs_64(2, 256, 8, 12, need=(True, False))
    _check_vs_64(2, 256, 8, 12, need=(False, True))
    _check_vs_64(2, 128, 8, 12, grad=1024.0)                      # upstream gradient != 1 (GradScaler)
    _check_vs_64(2, 256, 8, 12, lam=0.3)                          # lambda_d that is no fp16 number: two sweeps combined in f32
    _check_vs_64(2, 64, 16, 16, noncontig=True)
    _check_vs_64(2, 64, 16, 16, dtype=torch.float16)              # cast to f32 like tensors_to_dtype; the gradient returns in fp16


def test_determinism_and_batch_invariance(gpu_lib):
    from xpoint_amd import losses
    B, D, Hc, Wc = 4, 256, 20, 25
    d1, d2 = (t.cuda() for t in L.case_inputs("gpu/inv", B, D, Hc, Wc, True, 1.0, 0.6))
    d1[1:] *= 37.0                                                # other samples with another range: sample 0's scale must not move
    w1, w2, v1, v2 = _geometry(B, Hc, Wc, 3)

    def run(sl):
        a1, a2 = d1[sl].clone().requires_grad_(True), d2[sl].clone().requires_grad_(True)
        total, parts, norm = losses.descriptor_loss_sums(a1, a2, w1[sl], w2[sl], v1[sl], v2[sl], 8.0, 1.0, 0.2, 250.0)
        total.sum().backward()
        return total.detach(), parts, norm, a1.grad, a2.grad
    full, again, one = run(slice(0, 4)), run(slice(0, 4)), run(slice(0, 1))
    for a, b, c in zip(full, again, one):
        assert torch.equal(a, b)
        assert torch.equal(a[:1], c)
    logits, kp, m, _, _ = L.det_case("ce_w1")
    logits, kp, m = logits.cuda(), kp.cuda(), m.cuda()
    noise = torch.rand(2, 64, 11, 12, device="cuda")

    def det(sl, kind):
        x = logits[sl].clone().requires_grad_(True)
        total, stats = losses.detector_loss_stats(x, kp[sl], m[sl], noise[sl], kind, 0.5)
        total.sum().backward()
        return total.detach(), stats, x.grad
    for kind in (0, 1):
        full, again, one = det(slice(0, 2), kind), det(slice(0, 2), kind), det(slice(0, 1), kind)
        for a, b, c in zip(full, again, one):
            assert torch.equal(a, b)
            assert torch.equal(a[:1], c)


def test_autograd_wiring(gpu_lib):
    from xpoint_amd import losses
    d1, d2 = (t.cuda() for t in L.case_inputs("gpu/wire", 1, 64, 8, 12, True, 1.0, 0.6))
    with torch.no_grad():
        total, _, _ = losses.descriptor_loss_sums(d1.clone().requires_grad_(True), d2)
    assert total.grad_fn is None and not total.requires_grad
    total, _, _ = losses.descriptor_loss_sums(d1, d2)
    assert total.grad_fn is None and not total.requires_grad
    a1 = d1.clone().requires_grad_(True)
    total, parts, norm = losses.descriptor_loss_sums(a1, d2)
    assert total.requires_grad and not parts.requires_grad and not norm.requires_grad
    # directional derivative against the float64 restatement (gradcheck is unusable in f32 across the hinges)
    loss = (total / norm).mean()
    loss.backward()
    u = torch.from_numpy(np.random.default_rng(0).standard_normal(tuple(d1.shape))).cuda()
    ref = L.descriptor_loss64(d1, d2, None, None, None, None, 8.0, 1.0, 0.2, 250.0)
    dd_ref = float((ref["g1"] * u).sum())
    dd_got = float((a1.grad.double() * u).sum())
    assert abs(dd_got - dd_ref) <= TOL * float((ref["g1"].abs() * u.abs()).sum()), (dd_got, dd_ref)
    eps = 1e-6
    hi = L.descriptor_loss64(d1.double() + eps * u, d2, None, None, None, None, 8.0, 1.0, 0.2, 250.0, want_grads=False)["loss"]
    lo = L.descriptor_loss64(d1.double() - eps * u, d2, None, None, None, None, 8.0, 1.0, 0.2, 250.0, want_grads=False)["loss"]
    fd = float(hi - lo) / (2 * eps)
    assert abs(fd - dd_got) <= 1e-3 * abs(fd) + 1e-9, (fd, dd_got)
    logits, kp, m, _, _ = L.det_case("focal")
    noise = torch.rand(2, 64, 11, 12, device="cuda")
    with torch.no_grad():
        t, _ = losses.detector_loss_stats(logits.cuda().requires_grad_(True), kp.cuda(), m.cuda(), noise, 1)
    assert t.grad_fn is None
    for kind in (0, 1):
        x = logits.cuda().requires_grad_(True)
        t, stats = losses.detector_loss_stats(x, kp.cuda(), m.cuda(), noise, kind, 0.5, 0.25, 2.0)
        ref = L.detector_loss64(logits.cuda(), kp.cuda(), m.cuda(), noise, kind, 0.5, 0.25, 2.0, grad=3.0)
        (3.0 * (t / stats[:, 1].float().clamp(min=1.0)).mean()).backward()
        _close(t, ref["total"], f"det{kind}/total")
        _close(x.grad, ref["dlogits"], f"det{kind}/dlogits")
        assert torch.equal(stats[:, 2:7].sum(0).cpu(), ref["counts"].cpu())


def test_footprint_below_one_pair_tensor(gpu_lib):
    from xpoint_amd import losses
    B, D, Hc, Wc = 8, 256, 60, 80
    one = B * (Hc * Wc) ** 2 * 4
    ws = int(gpu_lib.xp_descriptor_loss_workspace_bytes(B, D, Hc, Wc))
    d1 = torch.nn.functional.normalize(torch.randn(B, D, Hc, Wc, device="cuda"), dim=1).requires_grad_(True)
    d2 = torch.nn.functional.normalize(torch.randn(B, D, Hc, Wc, device="cuda"), dim=1).requires_grad_(True)
    crit = losses.XPointLoss({"detector_handle_multiple_keypoints": "hard_assignment"})
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, _, _ = crit.descriptor_loss(d1, d2, None, None, None, None)
    loss.backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base - 2 * d1.numel() * 4            # minus the two gradients
    print(f"workspace {ws / 2**20:.1f} MiB, peak beyond inputs and gradients {extra / 2**20:.1f} MiB, one pair tensor {one / 2**20:.1f} MiB")
    assert ws < one and extra < one, (ws, extra, one)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(d1.grad).all()) and bool(torch.isfinite(d2.grad).all())


def test_training_smoke_step(gpu_lib):
    from xpoint_amd import losses
    torch.manual_seed(0)
    B, H, W = 2, 64, 96
    head_l = torch.nn.Conv2d(16, 65, 1).cuda()
    head_d = torch.nn.Conv2d(16, 64, 1).cuda()
    feats = [torch.randn(B, 16, H // 8, W // 8, device="cuda") for _ in range(2)]
    data = {s: {"keypoints": torch.rand(B, H, W, device="cuda") < 0.01, "valid_mask": torch.ones(B, 1, H, W, dtype=torch.bool, device="cuda"),
                "homography": torch.eye(3, device="cuda").repeat(B, 1, 1)} for s in ("optical", "thermal")}
    crit = losses.XPointLoss({"detector_handle_multiple_keypoints": "hard_assignment", "lambda": 1.0})
    params = list(head_l.parameters()) + list(head_d.parameters())
    opt = torch.optim.Adam(params, lr=1e-2)
    before = [p.detach().clone() for p in params]
    for _ in range(3):
        preds = [{"logits": head_l(f), "desc": torch.nn.functional.normalize(head_d(f), dim=1)} for f in feats]
        loss, comp = crit({"data": data, "pred": preds[0], "pred2": preds[1]})
        assert bool(torch.isfinite(loss)), comp
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert all(not torch.equal(a, b.detach()) for a, b in zip(before, params))
