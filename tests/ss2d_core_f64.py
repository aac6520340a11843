"""A float64 restatement of the training SS2D core in pixel layout (xpoint_amd.training.ss2d_core, csrc/train_ss2d.hip): the
routes of tests/vss_f64.cross_scan64 / cross_merge64, a plain Python scan over the route and torch's float64 autograd for every gradient.
tests/test_cpu_ss2d_train.py pins it: tests/vss_f64.vss_block64 rebuilt around core64 (vss_block64_core below) reproduces the block restatement, which
is itself pinned against the real reference.  tests/test_gpu_ss2d_train.py compares the HIP operator against it.

Inputs are hash uniforms (synth.uniform) the tests regenerate."""
import functools

import torch
import torch.nn.functional as F

from tests.vss_f64 import LEAVES, block_state, case_inputs, cross_merge64, cross_scan64
from xpoint_amd import synth


def _routes(t, k_dim):
    """t (B, H, W, 4, E), entry [..., k, :] belonging to route k at that pixel -> (B, 4, E, L): route k's own entries in route k's order."""
    d = t.permute(0, 3, 4, 1, 2)                                              # (B, 4, E, H, W)
    return torch.stack([cross_scan64(d[:, k])[:, k] for k in range(k_dim)], 1)


def core64(u, dtp, xd, R, A, Ds, dt_bias, dims):
    """ym (M, C) from u (M, C), dtp (M, 4 C) or (M, 4, C), xd (M, 4 (R + 2)) (only its B / C entries are read), A, Ds, dt_bias of 4 C elements each
    (route-major), dims = (B, H, W).  Differentiable in all six."""
    B, H, W = dims
    M, C = u.shape
    L = H * W
    xs = cross_scan64(u.view(B, H, W, C).permute(0, 3, 1, 2))                  # (B, 4, C, L)
    dts = _routes(dtp.reshape(B, H, W, 4, C), 4)                               # (B, 4, C, L)
    bcs = _routes(xd.view(B, H, W, 4, R + 2)[..., R:], 4)                      # (B, 4, 2, L)
    Bs, Cs = bcs[:, :, 0:1], bcs[:, :, 1:2]                                    # (B, 4, 1, L)
    dl = F.softplus(dts + dt_bias.reshape(1, 4, C, 1))                         # torch's threshold 20
    a = torch.exp(dl * A.reshape(1, 4, C, 1))
    bu = dl * Bs * xs
    h = u.new_zeros((B, 4, C))
    hs = []
    for l in range(L):
        h = a[..., l] * h + bu[..., l]
        hs.append(h)
    ys = Cs * torch.stack(hs, -1) + Ds.reshape(1, 4, C, 1) * xs
    return cross_merge64(ys, H, W).transpose(1, 2).reshape(M, C)


def vss_block64_core(p, x):
    """tests/vss_f64.vss_block64 (no stochastic depth) with x_proj and the dt projection in pixel layout and the SS2D core as core64."""
    B, H, W, C = x.shape
    M = B * H * W
    R = p["op.dt_projs_weight"].shape[2]
    t = F.layer_norm(x, (C,), p["norm.weight"], p["norm.bias"], 1e-5)
    t = t @ p["op.in_proj.weight"].t()
    t = F.silu(F.conv2d(t.permute(0, 3, 1, 2), p["op.conv2d.weight"], padding=1, groups=C)).permute(0, 2, 3, 1).reshape(M, C)
    xd = t @ p["op.x_proj_weight"].reshape(4 * (R + 2), C).t()                # (M, 4 (R + 2))
    dtp = torch.einsum("mkr,kdr->mkd", xd.view(M, 4, R + 2)[:, :, :R], p["op.dt_projs_weight"]).reshape(M, 4 * C)
    y = core64(t, dtp, xd, R, -torch.exp(p["op.A_logs"]), p["op.Ds"], p["op.dt_projs_bias"], (B, H, W)).view(B, H, W, C)
    y = F.layer_norm(y, (C,), p["op.out_norm.weight"], p["op.out_norm.bias"], 1e-5)
    x = x + y @ p["op.out_proj.weight"].t()
    t = F.layer_norm(x, (C,), p["norm2.weight"], p["norm2.bias"], 1e-5)
    t = F.gelu(t @ p["mlp.fc1.weight"].t() + p["mlp.fc1.bias"])
    return x + (t @ p["mlp.fc2.weight"].t() + p["mlp.fc2.bias"])


def vss_step64_core(case):
    """{'out', 'grad/x', 'grad/<leaf>'} of sum(out * R) for a case of tests/vss_f64.CASES, through vss_block64_core."""
    x, Rw = case_inputs(case)
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in block_state(case).items()}
    x = x.detach().double().clone().requires_grad_(True)
    out = vss_block64_core(p, x)
    grads = torch.autograd.grad((out * Rw.double()).sum(), [x] + [p[k] for k in LEAVES])
    res = {"out": out.detach(), "grad/x": grads[0]}
    res.update({"grad/" + k: g for k, g in zip(LEAVES, grads[1:])})
    return res


# ---- the operator's test inputs (tests/test_gpu_ss2d_train.py) ------------------------------------------------------------------------------
NAMES = ("u", "dtp", "xd", "A", "Ds", "dt_bias")
GRADS = ("du", "ddtp", "dbc", "dA", "dD", "ddt_bias")


def dt_rank(C):
    return (C + 15) // 16


def op_inputs(shape, variant="plain"):
    """{u, dtp, xd, A, Ds, dt_bias, dym} float32 for shape (B, H, W, C), and R.  variant: 'plain'; 'dt+30' / 'dt-30': dtp shifted (the linear branch of
    the softplus with a -> 0; dl -> 0 with a -> 1, the state crossing every chunk boundary undamped); 'smallA': A scaled by 1e-3."""
    B, H, W, C = shape
    M, R = B * H * W, dt_rank(C)
    un = lambda name, shp, lo, hi: torch.from_numpy(synth.uniform(f"ss2d_train/{shape}/{name}", shp, lo, hi))          # noqa: E731
    t = {"u": un("u", (M, C), -1.0, 1.0), "dtp": un("dtp", (M, 4 * C), -2.0, 2.0), "xd": un("xd", (M, 4 * (R + 2)), -1.0, 1.0),
         "A": -torch.exp(un("A", (4, C), -1.0, 1.0)), "Ds": un("Ds", (4, C), 0.5, 1.5), "dt_bias": un("dt_bias", (4, C), -4.0, -1.0),
         "dym": un("dym", (M, C), -1.0, 1.0)}
    if variant == "dt+30":
        t["dtp"] = t["dtp"] + 30.0
    elif variant == "dt-30":
        t["dtp"] = t["dtp"] - 30.0
    elif variant == "smallA":
        t["A"] = t["A"] * 1e-3
    else:
        assert variant == "plain", variant
    return t, R


def op_step64(t, R, dims):
    """{'ym', 'du', 'ddtp', 'dbc' (M, 4, 2), 'dA', 'dD', 'ddt_bias'} of core64 on the inputs t, float64."""
    leaves = [t[k].detach().double().clone().requires_grad_(True) for k in NAMES]
    ym = core64(*leaves[:3], R, *leaves[3:], dims)
    g = torch.autograd.grad(ym, leaves, t["dym"].double())
    M = t["u"].shape[0]
    return {"ym": ym.detach(), "du": g[0], "ddtp": g[1], "dbc": g[2].view(M, 4, R + 2)[:, :, R:].contiguous(), "dA": g[3], "dD": g[4], "ddt_bias": g[5]}


@functools.lru_cache(maxsize=None)
def op_reference(shape, variant="plain"):
    """op_step64 on op_inputs(shape, variant) (computed once per process; callers must not modify it)."""
    t, R = op_inputs(shape, variant)
    return op_step64(t, R, tuple(shape[:3]))
