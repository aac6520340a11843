"""A float64 restatement of the selective scan and its analytic backward (the test side of xpoint_amd/csrc/selective_scan_bwd.hip),
pinned by torch.autograd.gradcheck on tiny shapes and by the real reference's gradients (tests/golden/g26, tools/make_golden_scan_bwd.py).
The GPU tests (tests/test_gpu_scan_bwd.py) compare the HIP backward against `scan_bwd64`."""
import numpy as np
import pytest
import torch

from oracle.refharness.make_golden import scan_inputs
from xpoint_amd import synth


def _delta(delta, bias, softplus):
    t = delta + bias[:, None] if bias is not None else delta
    return (torch.where(t > 20, t, torch.log1p(torch.exp(t.clamp(max=20)))) if softplus else t), t


def scan_fwd64(u, delta, A, B, C, D=None, bias=None, softplus=True):
    """out (b, d, l) of the selective scan in float64, a per-step loop like the reference's selective_scan_torch (csms6s.py:25-68);
    delta may be grouped (b, dd, l) with d % dd == 0."""
    u, delta, A, B, C = (t.double() for t in (u, delta, A, B, C))
    b, d, L = u.shape
    g = B.shape[1]
    dl, _ = _delta(delta, bias.double() if bias is not None else None, softplus)
    dl = dl.repeat_interleave(d // dl.shape[1], 1)
    Bx = B.repeat_interleave(d // g, 1)
    Cx = C.repeat_interleave(d // g, 1)
    h = u.new_zeros((b, d, A.shape[1]))
    ys = []
    for i in range(L):
        h = torch.exp(dl[:, :, i, None] * A) * h + (dl[:, :, i] * u[:, :, i])[..., None] * Bx[:, :, :, i]
        ys.append((h * Cx[:, :, :, i]).sum(-1))
    y = torch.stack(ys, 2)
    return y + u * D.double()[:, None] if D is not None else y


def scan_bwd64(u, delta, A, B, C, D, bias, dout, softplus=True, abs_sums=False):
    """[du, ddelta, dA, dB, dC, dD, ddelta_bias] in float64, analytically: g_l = dL/dh_l = dy_l C_l + a_{l+1} g_{l+1}.
    abs_sums: also the sums of the absolute summands of dA, dD, ddelta_bias (the scale their rounding error is measured against)."""
    u, delta, A, B, C, dout = (t.double() for t in (u, delta, A, B, C, dout))
    b, d, L = u.shape
    grp, N = B.shape[1], A.shape[1]
    dd = delta.shape[1]
    rep = d // dd
    dl0, t = _delta(delta, bias.double() if bias is not None else None, softplus)
    dl = dl0.repeat_interleave(rep, 1)
    Bx = B.repeat_interleave(d // grp, 1)
    Cx = C.repeat_interleave(d // grp, 1)
    a = torch.exp(dl[:, :, None, :] * A[None, :, :, None])                     # (b, d, n, l)
    hs = u.new_zeros((b, d, N, L + 1))                                          # hs[..., l + 1] = h_l, hs[..., 0] = 0
    for i in range(L):
        hs[..., i + 1] = a[..., i] * hs[..., i] + (dl[:, :, i] * u[:, :, i])[..., None] * Bx[..., i]
    gs = u.new_zeros((b, d, N, L))
    q = u.new_zeros((b, d, N))
    for i in range(L - 1, -1, -1):
        gi = dout[:, :, i, None] * Cx[..., i] + q
        gs[..., i] = gi
        q = a[..., i] * gi
    hprev, h = hs[..., :-1], hs[..., 1:]
    gha = gs * hprev * a
    dA = (gha * dl[:, :, None, :]).sum((0, 3))
    ddl = (gha * A[None, :, :, None]).sum(2) + (gs * Bx).sum(2) * u
    du = (gs * Bx).sum(2) * dl + (dout * D.double()[:, None] if D is not None else 0)
    dB = (gs * (dl * u)[:, :, None, :]).view(b, grp, d // grp, N, L).sum(2)
    dC = (dout[:, :, None, :] * h).view(b, grp, d // grp, N, L).sum(2)
    if softplus:
        ddl = ddl.view(b, dd, rep, L) * torch.sigmoid(t)[:, :, None, :]
    ddelta = ddl.view(b, dd, rep, L).sum(2)
    dD = (dout * u).sum((0, 2)) if D is not None else None
    ddb = ddelta.sum((0, 2)) if bias is not None else None
    if abs_sums:
        return [du, ddelta, dA, dB, dC, dD, ddb], [(gha * dl[:, :, None, :]).abs().sum((0, 3)), (dout * u).abs().sum((0, 2)),
                                                   ddl.abs().view(b, dd, rep, L).sum((0, 2, 3))]
    return [du, ddelta, dA, dB, dC, dD, ddb]


class Scan64(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, bias, softplus):
        ctx.save_for_backward(u, delta, A, B, C, D, bias)
        ctx.softplus = softplus
        return scan_fwd64(u, delta, A, B, C, D, bias, softplus)

    @staticmethod
    def backward(ctx, dout):
        u, delta, A, B, C, D, bias = ctx.saved_tensors
        return (*scan_bwd64(u, delta, A, B, C, D, bias, dout, ctx.softplus), None)


def inputs64(name, b, g, c, n, L, dd=None):
    d = g * c
    dd = dd or d
    return [torch.from_numpy(synth.uniform(f"{name}/{k}", s, lo, hi).astype(np.float64)) for k, s, lo, hi in (
        ("u", (b, d, L), -1.7, 1.7), ("delta", (b, dd, L), 0.0, 0.5), ("A", (d, n), -0.5, 0.0), ("B", (b, g, n, L), -1.7, 1.7),
        ("C", (b, g, n, L), -1.7, 1.7), ("D", (d,), -1.7, 1.7), ("bias", (dd,), 0.0, 0.5))]


@pytest.mark.parametrize("shape,softplus", [((2, 2, 2, 1, 5, None), True), ((1, 2, 2, 3, 4, None), True), ((2, 1, 4, 2, 3, 2), True),
                                            ((1, 2, 2, 2, 4, 1), False)], ids=str)
def test_restatement_gradcheck(shape, softplus):
    *s, dd = shape
    ins = [t.requires_grad_(True) for t in inputs64("gc/%s" % (shape,), *s, dd=dd)]
    assert torch.autograd.gradcheck(lambda *a: Scan64.apply(*a, softplus), tuple(ins), eps=1e-6, atol=1e-7, rtol=1e-6)


def _g26_cases(golden):
    g = golden("g26_selective_scan_bwd.npz")
    return sorted({k.rsplit("/", 1)[0] for k in g.files})


def bars(itype=torch.float32):
    """The reference's gradient bars (test_selective_scan.py:401-404, 497-517): (rtol, atol) per gradient."""
    rtol, atol = {torch.float32: (6e-4, 2e-3), torch.float16: (3e-3, 5e-3), torch.bfloat16: (3e-2, 5e-2)}[itype]
    rtolw, atolw = 1e-3, 1e-3
    return {"du": (rtol * 2, atol * 2), "ddelta": (rtol * 5, atol * 10), "dB": (rtol, atol), "dC": (rtol, atol),
            "dA": (rtolw, atolw * 5), "dD": (rtolw, atolw), "ddelta_bias": (rtolw, atolw)}


NAMES = ("du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias")


def g26_check(got, g, name, plain=False, itype=torch.float32):
    """Assert the seven gradients `got` (numpy, f32 or f64) meet the reference's bars against g26."""
    _BARS = bars(itype)
    for k, v in zip(NAMES, got):
        key = f"{name}/{k}_plain" if plain else f"{name}/{k}"
        if key not in g.files:
            continue
        rtol, atol = _BARS[k]
        np.testing.assert_allclose(np.asarray(v, np.float32), g[key], rtol=rtol, atol=atol, err_msg=key)


def test_restatement_matches_g26(golden):
    g = golden("g26_selective_scan_bwd.npz")
    for name in _g26_cases(golden):
        case = tuple(int(v) for v in name.split("/")[1].split("_"))
        B, K, C, N, L = case
        u, delta, A, Bm, Cm, Dv, bias = [torch.from_numpy(x) for x in scan_inputs(name, *case)]
        dout = torch.from_numpy(synth.uniform(name + "/dout", (B, K * C, L), -1.0, 1.0))
        g26_check([t.numpy() for t in scan_bwd64(u, delta, A, Bm, Cm, Dv, bias, dout, True)], g, name)
        if f"{name}/du_plain" in g.files:
            g26_check([t.numpy() if t is not None else None for t in scan_bwd64(u, delta, A, Bm, Cm, None, None, dout, False)], g, name, True)
