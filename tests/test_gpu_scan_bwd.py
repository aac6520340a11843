"""GPU: the HIP selective-scan backward (xp_selective_scan_bwd_typed, kernels.selective_scan_bwd) and the autograd wiring of
selective_scan_fn / cross_scan_fn / cross_merge_fn, against the real reference's gradients (tests/golden/g26) at the reference's bars and
against the float64 restatement of tests/test_cpu_scan_grad.py at the build's f32 target (max error <= 1e-4 x the tensor's scale)."""
import itertools

import numpy as np
import pytest
import torch

from oracle.refharness.make_golden import SCAN_CASES, scan_inputs
from tests.test_cpu_scan_grad import NAMES, Scan64, bars, g26_check, inputs64, scan_bwd64
from xpoint_amd import synth

pytestmark = pytest.mark.gpu


def _fwd_bwd(u, delta, A, B, C, D, bias, dout, softplus=True):
    from xpoint_amd.kernels import selective_scan_bwd, selective_scan_fwd
    _, x = selective_scan_fwd(u, delta, A, B, C, D, bias, softplus, 1, True)
    return selective_scan_bwd(u, delta, A, B, C, D, bias, dout, x, softplus, 1)


def _check64(got, ref_abs, tol=1e-4):
    """max |got - ref| <= tol x the tensor's scale: max |ref| for du, ddelta, dB, dC; the largest sum of absolute summands for dA, dD and
    ddelta_bias (ref_abs = scan_bwd64(..., abs_sums=True))."""
    ref, (absA, absD, absDB) = ref_abs
    scales = {"dA": absA, "dD": absD, "ddelta_bias": absDB}
    for k, gv, rv in zip(NAMES, got, ref):
        if rv is None:
            assert gv is None, k
            continue
        sc = float(scales[k].max()) if k in scales else float(rv.abs().max())
        err = float((gv.double().cpu() - rv).abs().max())
        assert err <= tol * max(sc, 1e-30), (k, err, sc)


@pytest.mark.parametrize("case", SCAN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bwd_vs_golden_and_restatement(gpu_lib, golden, case):
    g = golden("g26_selective_scan_bwd.npz")
    name = "scan/%d_%d_%d_%d_%d" % case
    B, K, C, N, L = case
    cpu = [torch.from_numpy(x) for x in scan_inputs(name, *case)]
    dout_c = torch.from_numpy(synth.uniform(name + "/dout", (B, K * C, L), -1.0, 1.0))
    u, delta, A, Bm, Cm, Dv, bias = [t.cuda() for t in cpu]
    dout = dout_c.cuda()
    got = _fwd_bwd(u, delta, A, Bm, Cm, Dv, bias, dout, True)
    if f"{name}/du" in g.files:
        g26_check([t.cpu().numpy() for t in got], g, name)
    _check64(got, scan_bwd64(*cpu, dout_c, True, abs_sums=True))
    got2 = _fwd_bwd(u, delta, A, Bm, Cm, None, None, dout, False)
    assert got2[5] is None and got2[6] is None
    if f"{name}/du_plain" in g.files:
        g26_check([t.cpu().numpy() if t is not None else None for t in got2], g, name, plain=True)
    _check64(got2, scan_bwd64(*cpu[:5], None, None, dout_c, False, abs_sums=True))


SHAPES = ([(1, 2, 3, 1, L, None) for L in (1, 3, 255, 2047, 2048, 2049, 4097)]
          + [(2, g, 4, n, 300, None) for n in (1, 4, 16) for g in (1, 2, 4)]
          + [(2, 2, 4, 1, 2100, 4), (1, 4, 2, 4, 600, 2), (2, 1, 6, 1, 517, 3)])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("variant", ["full", "plain"])
def test_bwd_shapes_vs_restatement(gpu_lib, shape, variant):
    *s, dd = shape
    u, delta, A, Bm, Cm, Dv, bias = inputs64(f"bwd/{shape}", *s, dd=dd)
    dout = torch.from_numpy(synth.uniform(f"bwd/{shape}/dout", tuple(u.shape), -1.0, 1.0)).double()
    if variant == "plain":
        Dv = bias = None
    sp = variant == "full"
    ins = [t.float() if t is not None else None for t in (u, delta, A, Bm, Cm, Dv, bias, dout)]
    got = _fwd_bwd(*[t.cuda() if t is not None else None for t in ins], sp)
    _check64(got, scan_bwd64(*ins, sp, abs_sums=True))


@pytest.mark.parametrize("itype", [torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("dout_f32", [True, False])
@pytest.mark.parametrize("L", [300, 4097])
def test_bwd_half_inputs(gpu_lib, itype, dout_f32, L):
    name = f"bwdh/{L}"
    cpu = inputs64(name, 2, 4, 6, 1, L)
    dout = torch.from_numpy(synth.uniform(name + "/dout", tuple(cpu[0].shape), -1.0, 1.0))
    half = [t.to(itype) if i in (0, 1, 3, 4) else t.float() for i, t in enumerate(cpu)]
    dh = dout.float() if dout_f32 else dout.to(itype)
    got = _fwd_bwd(*[t.cuda() for t in half], dh.cuda(), True)
    for i, t in enumerate(got):
        assert t.dtype == (itype if i in (0, 1, 3, 4) else torch.float32), (NAMES[i], t.dtype)
    ref = scan_bwd64(*[t.double() for t in half], dh.double(), True)
    b = bars(itype)
    for k, gv, rv in zip(NAMES, got, ref):
        rtol, atol = b[k]
        if k in ("dA", "dD", "ddelta_bias"):          # sums over L: compare relative to the sum of the absolute summands
            atol = max(atol, rtol * float(rv.abs().max()))
        torch.testing.assert_close(gv.double().cpu(), rv, rtol=rtol, atol=atol, msg=k)


def test_bwd_deterministic_and_batch_invariant(gpu_lib):
    shape = (3, 2, 12, 1, 4100)
    u, delta, A, Bm, Cm, Dv, bias = [t.float().cuda() for t in inputs64("bwd/det", *shape)]
    dout = torch.from_numpy(synth.uniform("bwd/det/dout", tuple(u.shape), -1.0, 1.0)).cuda()
    a = _fwd_bwd(u, delta, A, Bm, Cm, Dv, bias, dout)
    b = _fwd_bwd(u, delta, A, Bm, Cm, Dv, bias, dout)
    for k, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), k
    for s in range(3):
        one = _fwd_bwd(u[s:s + 1], delta[s:s + 1], A, Bm[s:s + 1], Cm[s:s + 1], Dv, bias, dout[s:s + 1])
        for i in (0, 1, 3, 4):
            assert torch.equal(one[i][0], a[i][s]), (NAMES[i], s)


def test_autograd_wiring(gpu_lib):
    from xpoint_amd.kernels import _selective_scan_fn_nograd, selective_scan_bwd, selective_scan_fn
    shape = (2, 4, 8, 1, 4500)
    ins = [t.float().cuda() for t in inputs64("bwd/ag", *shape)]
    dout = torch.from_numpy(synth.uniform("bwd/ag/dout", tuple(ins[0].shape), -1.0, 1.0)).cuda()
    with torch.no_grad():
        out0, last0 = selective_scan_fn(*ins, True, return_last_state=True)
    out_nograd = selective_scan_fn(*ins, True)                  # nothing requires grad: the inference path
    assert not out_nograd.requires_grad and torch.equal(out_nograd, out0)
    leaves = [t.clone().requires_grad_(True) for t in ins]
    out, last = selective_scan_fn(*leaves, True, return_last_state=True)
    assert out.requires_grad and not last.requires_grad
    assert torch.equal(out.detach(), out0) and torch.equal(last, last0)
    x = out.grad_fn.saved_tensors[-1].clone()                # the chunk states of the f32 forward that produced `out`
    grads = torch.autograd.grad(out, leaves, dout)
    _, x_fn = _selective_scan_fn_nograd(*ins, True, want_x=True)
    assert torch.equal(x, x_fn)
    direct = selective_scan_bwd(*ins, dout, x, True, 1)
    for k, gv, dv in zip(NAMES, grads, direct):
        assert torch.equal(gv, dv), k


CSM_FLAGS = list(itertools.product([True, False], [True, False], [False, True], [0, 1, 2]))


@pytest.mark.parametrize("flags", CSM_FLAGS, ids=str)
def test_cross_scan_merge_adjoint_and_grad(gpu_lib, flags):
    from xpoint_amd.kernels import cross_merge_fn, cross_scan_fn
    in_cf, out_cf, obo, scans = flags
    B, C, H, W = 2, 3, 5, 7
    if obo:
        xs = (B, 4, C, H, W) if in_cf else (B, H, W, 4, C)
    else:
        xs = (B, C, H, W) if in_cf else (B, H, W, C)
    ys = (B, 4, C, H, W) if out_cf else (B, H, W, 4, C)
    x = torch.from_numpy(synth.uniform(f"csm/{flags}/x", xs, -1, 1)).double()
    y = torch.from_numpy(synth.uniform(f"csm/{flags}/y", ys, -1, 1)).double()
    # the adjoint identity <scan(x), y> = <x, merge(y)> in float64 (the kernels move / add float32 values: exact products in float64)
    sx = cross_scan_fn(x.float().cuda(), in_cf, out_cf, obo, scans).double().cpu()
    my = cross_merge_fn(y.float().cuda(), in_cf, out_cf, obo, scans).double().cpu()
    lhs = float((sx.reshape(-1) * y.float().double().reshape(-1)).sum())
    rhs = float((x.float().double().reshape(-1) * my.reshape(-1)).sum())
    assert abs(lhs - rhs) <= 1e-5 * (abs(lhs) + 1.0), (lhs, rhs)
    # autograd through both ops vs a torch permutation restatement built from the forward itself (index tensor through the op)
    idx = torch.arange(int(np.prod(xs)), dtype=torch.float32).view(xs)
    perm = cross_scan_fn(idx.cuda(), in_cf, out_cf, obo, scans).cpu().long().reshape(-1)
    xg = x.float().cuda().requires_grad_(True)
    sy = cross_scan_fn(xg, in_cf, out_cf, obo, scans)
    wy = torch.from_numpy(synth.uniform(f"csm/{flags}/w", tuple(sy.shape), -1, 1)).cuda()
    (gx,) = torch.autograd.grad((sy * wy).sum(), xg)
    ref = torch.zeros(int(np.prod(xs)), dtype=torch.float64).index_add_(0, perm, wy.double().cpu().reshape(-1)).view(xs)
    torch.testing.assert_close(gx.double().cpu(), ref, rtol=0, atol=1e-6)
    yg = y.float().cuda().requires_grad_(True)
    my2 = cross_merge_fn(yg, in_cf, out_cf, obo, scans)
    wm = torch.from_numpy(synth.uniform(f"csm/{flags}/wm", tuple(my2.shape), -1, 1)).cuda()
    (gy,) = torch.autograd.grad((my2 * wm).sum(), yg)
    # merge is the transpose of scan: dL/dy[perm-position] = wm[x index]
    ref_y = wm.double().cpu().reshape(-1)[perm].view(ys)
    torch.testing.assert_close(gy.double().cpu(), ref_y, rtol=0, atol=1e-6)


def _ss2d_core(x, A_logs, Ds, dt_w, dt_b, xproj_w, scan_fn, sel_fn, merge_fn):
    B, C, H, W = x.shape
    K, L = 4, H * W
    xs = scan_fn(x)                                                    # (B, 4, C, L)
    R = dt_w.shape[2]
    N = 1
    x_dbl = torch.einsum("bkdl,kcd->bkcl", xs, xproj_w)                # (B, 4, R + 2N, L)
    dts, Bs, Cs = torch.split(x_dbl, [R, N, N], dim=2)
    dts = torch.einsum("bkrl,kdr->bkdl", dts, dt_w)
    ys = sel_fn(xs.reshape(B, -1, L), dts.reshape(B, -1, L), -torch.exp(A_logs), Bs.contiguous(), Cs.contiguous(), Ds, dt_b.reshape(-1))
    return merge_fn(ys.view(B, K, C, H, W))


def test_composed_ss2d_core_grads(gpu_lib):
    from xpoint_amd.kernels import cross_merge_fn, cross_scan_fn, selective_scan_fn
    B, C, H, W, R = 1, 768, 15, 20, 48
    u = lambda n, s, lo=-1.0, hi=1.0: torch.from_numpy(synth.uniform("ss2d_bwd/" + n, s, lo, hi)).double()   # noqa: E731
    params = {"x": u("x", (B, C, H, W)), "A_logs": u("A_logs", (4 * C, 1), -1.0, 0.5), "Ds": u("Ds", (4 * C,)),
              "dt_w": u("dt_w", (4, C, R), -0.1, 0.1), "dt_b": u("dt_b", (4, C), -4.0, -2.0)}
    xproj_w = u("xproj", (4, R + 2, C), -0.05, 0.05)
    wl = u("wl", (B, C, H * W))

    def ref_merge(y):
        Bb, K, Cc, Hh, Ww = y.shape
        y = y.view(Bb, K, Cc, -1)
        y = y[:, 0:2] + y[:, 2:4].flip(dims=[-1])
        return y[:, 0] + y[:, 1].view(Bb, -1, Ww, Hh).transpose(2, 3).contiguous().view(Bb, -1, Hh * Ww)

    def ref_scan(x):
        Bb, Cc, Hh, Ww = x.shape
        y = x.new_empty((Bb, 4, Cc, Hh * Ww))
        y[:, 0] = x.flatten(2, 3)
        y[:, 1] = x.transpose(2, 3).flatten(2, 3)
        y[:, 2:4] = torch.flip(y[:, 0:2], dims=[-1])
        return y

    def ref_sel(us, dts, A, Bs, Cs, Ds, db):
        return Scan64.apply(us, dts, A, Bs, Cs, Ds, db, True)

    p64 = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out64 = _ss2d_core(p64["x"], p64["A_logs"], p64["Ds"], p64["dt_w"], p64["dt_b"], xproj_w, ref_scan, ref_sel, ref_merge)
    g64 = torch.autograd.grad((out64 * wl).sum(), list(p64.values()))
    pg = {k: v.float().cuda().requires_grad_(True) for k, v in params.items()}
    out = _ss2d_core(pg["x"], pg["A_logs"], pg["Ds"], pg["dt_w"], pg["dt_b"], xproj_w.float().cuda(),
                     lambda x: cross_scan_fn(x, True, True, False, 0),
                     lambda *a: selective_scan_fn(*a, delta_softplus=True), lambda y: cross_merge_fn(y, True, True, False, 0))
    gg = torch.autograd.grad((out * wl.float().cuda()).sum(), list(pg.values()))
    for k, a, b in zip(params, gg, g64):
        err = float((a.double().cpu() - b).abs().max())
        assert err <= 1e-4 * float(b.abs().max()), (k, err, float(b.abs().max()))


def test_bwd_at_size_480x640_stage0(gpu_lib):
    shape = (1, 4, 96, 1, 19200)
    ins = inputs64("bwd/size", *shape)
    dout = torch.from_numpy(synth.uniform("bwd/size/dout", tuple(ins[0].shape), -1.0, 1.0)).double()
    f32 = [t.float() for t in ins] + [dout.float()]
    got = _fwd_bwd(*[t.cuda() for t in f32], True)
    _check64(got, scan_bwd64(*f32, True, abs_sums=True))


def test_bwd_argument_errors(gpu_lib):
    from xpoint_amd.kernels import selective_scan_bwd
    ins = [t.float().cuda() for t in inputs64("bwd/err", 1, 2, 2, 1, 4100)]
    dout = torch.zeros_like(ins[0])
    with pytest.raises(RuntimeError):
        selective_scan_bwd(*ins, dout, None, True, 1)                  # x is required past 2048
    with pytest.raises(RuntimeError):
        selective_scan_bwd(*ins, dout.half(), None, True, 1)           # dout: f32 or the input dtype
