"""Operator-level Python surface over the C ABI (thin: argument checks, output allocation, ctypes).

Mirrors the reference's operator interfaces for the hot path so parity tests read like the
reference's own: `selective_scan_fn` (reference vmamba_src/csms6s.py:112-126, pybind op
selective_scan_cuda_oflex.fwd, selective_scan_oflex.cpp:143-231).  Errors from the C ABI surface as
RuntimeError, like TORCH_CHECK failures do in the reference.  `cross_scan_fn` / `cross_merge_fn` mirror
vmamba_src/csm_triton.py:501-517 (same arguments, shapes and layouts).  `selective_scan_bwd` is the reference's
selective_scan_cuda_oflex.bwd (selective_scan_oflex.cpp:233-350); `selective_scan_fn`, `cross_scan_fn` and `cross_merge_fn` record an
autograd graph when an input requires grad and grad mode is on (reference SelectiveScanCuda, csms6s.py:71-110; CrossScanTritonF /
CrossMergeTritonF, csm_triton.py:403-500), and otherwise take their inference path unchanged."""
from __future__ import annotations

import torch

from . import _lib
from ._lib import c_i, ptr


def _f32c(t, name):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA(HIP) tensor")       # selective_scan_oflex.cpp:152-160
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: this build computes in float32 (got {t.dtype})")
    return t.contiguous()


_ITYPE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def selective_scan_fwd(u, delta, A, B, C, D=None, delta_bias=None, delta_softplus=True, nrows=1, out_float=True):
    """The pybind op of the reference, `selective_scan_cuda_oflex.fwd(u, delta, A, B, C, D, delta_bias, delta_softplus, nrows,
    out_float) -> [out, x]` (selective_scan_oflex.cpp:143-231): u, delta, B, C of one dtype in {float32, float16, bfloat16}; A, D,
    delta_bias float32; out float32 if out_float else the input dtype; x (B, D, ceil(L / 2048), 2 N) float32, last state =
    x[:, :, -1, 1::2].  nrows is a CUDA launch-shape hint there and is ignored here."""
    for t, n in ((u, "u"), (delta, "delta"), (A, "A"), (B, "B"), (C, "C"), (D, "D"), (delta_bias, "delta_bias")):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA(HIP) tensor")                     # selective_scan_oflex.cpp:152-160
    if u.dtype not in _ITYPE:
        raise RuntimeError(f"u: dtype must be float32, float16 or bfloat16 (got {u.dtype})")
    for t, n in ((delta, "delta"), (B, "B"), (C, "C")):
        if t.dtype != u.dtype:
            raise RuntimeError(f"{n} must have u's dtype {u.dtype} (got {t.dtype})")
    for t, n in ((A, "A"), (D, "D"), (delta_bias, "delta_bias")):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"{n} must be float32 (got {t.dtype})")
    if u.dim() != 3 or B.dim() != 4:
        raise RuntimeError("selective_scan_fwd: u must be (B, D, L) and B/C (B, G, N, L)")
    u, delta, A, B, C = u.contiguous(), delta.contiguous(), A.contiguous(), B.contiguous(), C.contiguous()
    D = D.contiguous() if D is not None else None
    delta_bias = delta_bias.contiguous() if delta_bias is not None else None
    batch, dim, L = u.shape
    _, G, N, L2 = B.shape
    if L2 != L or C.shape != B.shape or A.shape != (dim, N) or delta.shape[0] != batch or delta.shape[2] != L:
        raise RuntimeError("selective_scan_fwd: shape mismatch")
    if N > 256:
        raise RuntimeError("selective_scan_fwd: dstate must be <= 256")                # MAX_DSTATE, selective_scan_oflex.cpp:11
    out = torch.empty((batch, dim, L), device=u.device, dtype=torch.float32 if out_float else u.dtype)
    x = torch.empty((batch, dim, (L + 2047) // 2048, 2 * N), device=u.device, dtype=torch.float32)
    _lib.call("xp_selective_scan_fwd_typed", ptr(u), ptr(delta), ptr(A), ptr(B), ptr(C), ptr(D), ptr(delta_bias), ptr(out), ptr(x),
              c_i(_ITYPE[u.dtype]), c_i(int(bool(out_float))), c_i(batch), c_i(dim), c_i(delta.shape[1]), c_i(L), c_i(N), c_i(G),
              c_i(int(bool(delta_softplus))), _lib.current_stream(u))
    return [out, x]


def _selective_scan_fn_nograd(u, delta, A, B, C, D=None, delta_bias=None, delta_softplus=True, oflex=True, backend=None,
                              return_last_state=False, want_x=False):
    """u (B, K*C, L); delta (B, Dd, L) with K*C % Dd == 0; A (K*C, N); B, C (B, K, N, L); D, delta_bias
    (K*C)/(Dd).  Returns out (B, K*C, L) float32 (oflex: float output).  float16 / bfloat16 inputs go through
    selective_scan_fwd (the reference's half-input / float-output instantiations)."""
    if u.dtype in (torch.float16, torch.bfloat16):
        out, x = selective_scan_fwd(u, delta, A, B, C, D, delta_bias, delta_softplus, 1, oflex)
        if want_x:
            return out, x
        return (out, x[:, :, -1, 1::2].contiguous()) if return_last_state else out
    u, delta, A, B, C = (_f32c(t, n) for t, n in ((u, "u"), (delta, "delta"), (A, "A"), (B, "B"), (C, "C")))
    D = _f32c(D, "D"); delta_bias = _f32c(delta_bias, "delta_bias")
    if u.dim() != 3 or B.dim() != 4:
        raise RuntimeError("selective_scan_fn: u must be (B, D, L) and B/C (B, G, N, L)")
    batch, dim, L = u.shape
    _, G, N, L2 = B.shape
    if L2 != L or C.shape != B.shape or A.shape != (dim, N) or delta.shape[0] != batch or delta.shape[2] != L:
        raise RuntimeError("selective_scan_fn: shape mismatch")
    out = torch.empty_like(u)
    if want_x:          # the same kernels, plus the per-chunk states the backward restarts from
        x = torch.empty((batch, dim, (L + 2047) // 2048, 2 * N), device=u.device, dtype=torch.float32)
        with torch.cuda.device(u.device):
            _lib.call("xp_selective_scan_fwd_x", ptr(u), ptr(delta), ptr(A), ptr(B), ptr(C), ptr(D), ptr(delta_bias), ptr(out), None, ptr(x),
                      c_i(batch), c_i(dim), c_i(delta.shape[1]), c_i(L), c_i(N), c_i(G), c_i(int(bool(delta_softplus))), _lib.current_stream())
        return out, x
    last = torch.empty((batch, dim, N), device=u.device, dtype=torch.float32) if return_last_state else None
    with torch.cuda.device(u.device):
        _lib.call("xp_selective_scan_fwd", ptr(u), ptr(delta), ptr(A), ptr(B), ptr(C), ptr(D), ptr(delta_bias), ptr(out),
                  ptr(last), c_i(batch), c_i(dim), c_i(delta.shape[1]), c_i(L), c_i(N), c_i(G), c_i(int(bool(delta_softplus))),
                  _lib.current_stream())
    return (out, last) if return_last_state else out


def selective_scan_bwd(u, delta, A, B, C, D, delta_bias, dout, x, delta_softplus=True, nrows=1):
    """The pybind op of the reference, `selective_scan_cuda_oflex.bwd(u, delta, A, B, C, D, delta_bias, dout, x, delta_softplus, nrows)
    -> [du, ddelta, dA, dB, dC, dD, ddelta_bias]` (selective_scan_oflex.cpp:233-350).  u, delta, B, C of one dtype in {float32, float16,
    bfloat16}; A, D, delta_bias float32; dout float32 or the input dtype; x = the forward's chunk states (selective_scan_fwd's second output),
    required when L > 2048.  du, ddelta (summed over a grouped delta's repeat), dB, dC in the input dtype (dB, dC accumulated in float32);
    dA, dD, ddelta_bias float32 (dD / ddelta_bias None when D / delta_bias is None).  Deterministic: every sum runs in a fixed order."""
    for t, n in ((u, "u"), (delta, "delta"), (A, "A"), (B, "B"), (C, "C"), (D, "D"), (delta_bias, "delta_bias"), (dout, "dout"), (x, "x")):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA(HIP) tensor")
    if u.dtype not in _ITYPE:
        raise RuntimeError(f"u: dtype must be float32, float16 or bfloat16 (got {u.dtype})")
    for t, n in ((delta, "delta"), (B, "B"), (C, "C")):
        if t.dtype != u.dtype:
            raise RuntimeError(f"{n} must have u's dtype {u.dtype} (got {t.dtype})")
    for t, n in ((A, "A"), (D, "D"), (delta_bias, "delta_bias"), (x, "x")):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"{n} must be float32 (got {t.dtype})")
    if dout.dtype not in (u.dtype, torch.float32):
        raise RuntimeError(f"dout must be float32 or u's dtype {u.dtype} (got {dout.dtype})")   # selective_scan_oflex.cpp:249
    if u.dim() != 3 or B.dim() != 4:
        raise RuntimeError("selective_scan_bwd: u must be (B, D, L) and B/C (B, G, N, L)")
    batch, dim, L = u.shape
    _, G, N, L2 = B.shape
    Dd = delta.shape[1]
    if (L2 != L or C.shape != B.shape or A.shape != (dim, N) or delta.dim() != 3 or delta.shape[0] != batch or delta.shape[2] != L
            or tuple(dout.shape) != (batch, dim, L)):
        raise RuntimeError("selective_scan_bwd: shape mismatch")
    if N > 256:
        raise RuntimeError("selective_scan_bwd: dstate must be <= 256")
    if G <= 0 or dim % G or dim % Dd:
        raise RuntimeError("selective_scan_bwd: dim must be divisible by n_groups and delta_dim")
    if D is not None and tuple(D.shape) != (dim,):
        raise RuntimeError("selective_scan_bwd: D must be (dim,)")
    if delta_bias is not None and tuple(delta_bias.shape) != (Dd,):
        raise RuntimeError("selective_scan_bwd: delta_bias must be (delta_dim,)")
    nxc = (L + 2047) // 2048
    if x is None and nxc > 1:
        raise RuntimeError("selective_scan_bwd: x is required when L > 2048")             # selective_scan_oflex.cpp:306
    if x is not None and tuple(x.shape) != (batch, dim, nxc, 2 * N):
        raise RuntimeError(f"selective_scan_bwd: x must be {(batch, dim, nxc, 2 * N)} (got {tuple(x.shape)})")
    u, delta, A, B, C, dout = (t.contiguous() for t in (u, delta, A, B, C, dout))
    D = D.contiguous() if D is not None else None
    delta_bias = delta_bias.contiguous() if delta_bias is not None else None
    x = x.contiguous() if x is not None else None
    dev = u.device
    du = torch.empty_like(u)
    ddelta = torch.empty_like(delta)
    dA = torch.empty_like(A)
    dB = torch.empty_like(B)
    dC = torch.empty_like(C)
    dD = torch.empty_like(D) if D is not None else None
    ddb = torch.empty_like(delta_bias) if delta_bias is not None else None
    nbytes = int(_lib.load().xp_selective_scan_bwd_workspace_bytes(batch, dim, Dd, L, N, G))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.call("xp_selective_scan_bwd_typed", ptr(u), ptr(delta), ptr(A), ptr(B), ptr(C), ptr(D), ptr(delta_bias), ptr(dout), ptr(x),
                  ptr(du), ptr(ddelta), ptr(dA), ptr(dB), ptr(dC), ptr(dD), ptr(ddb), ptr(ws), _lib.c_sz(nbytes), c_i(_ITYPE[u.dtype]),
                  c_i(int(dout.dtype == torch.float32)), c_i(batch), c_i(dim), c_i(Dd), c_i(L), c_i(N), c_i(G),
                  c_i(int(bool(delta_softplus))), _lib.current_stream(dev))
    return [du, ddelta, dA, dB, dC, dD, ddb]


class _SelectiveScanFn(torch.autograd.Function):
    """Reference SelectiveScanCuda (csms6s.py:71-110): the forward keeps x (the chunk states), the backward is selective_scan_bwd."""

    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, delta_bias, delta_softplus, oflex, return_last_state):
        out, x = _selective_scan_fn_nograd(u, delta, A, B, C, D, delta_bias, delta_softplus, oflex, want_x=True)
        ctx.delta_softplus = bool(delta_softplus)
        ctx.save_for_backward(u, delta, A, B, C, D, delta_bias, x)
        if not return_last_state:
            return out
        last = x[:, :, -1, 1::2].contiguous()
        ctx.mark_non_differentiable(last)
        return out, last

    @staticmethod
    def backward(ctx, dout, *_dlast):
        u, delta, A, B, C, D, delta_bias, x = ctx.saved_tensors
        if dout.dtype not in (torch.float32, u.dtype):
            dout = dout.float()
        du, ddelta, dA, dB, dC, dD, ddb = selective_scan_bwd(u.contiguous(), delta.contiguous(), A.contiguous(), B.contiguous(),
                                                             C.contiguous(), D, delta_bias, dout, x, ctx.delta_softplus, 1)
        return du, ddelta, dA, dB, dC, dD, ddb, None, None, None


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def selective_scan_fn(u, delta, A, B, C, D=None, delta_bias=None, delta_softplus=True, oflex=True, backend=None,
                      return_last_state=False):
    """u (B, K*C, L); delta (B, Dd, L) with K*C % Dd == 0; A (K*C, N); B, C (B, K, N, L); D, delta_bias
    (K*C)/(Dd).  Returns out (B, K*C, L) float32 (oflex: float output).  float16 / bfloat16 inputs go through
    selective_scan_fwd (the reference's half-input / float-output instantiations).  With grad mode on and an input that requires grad,
    the call records an autograd graph whose backward is selective_scan_bwd (out is bit-identical to the no-grad call's; the last state
    is non-differentiable); otherwise it is the inference path alone."""
    if _needs_grad(u, delta, A, B, C, D, delta_bias):
        return _SelectiveScanFn.apply(u, delta, A, B, C, D, delta_bias, delta_softplus, oflex, return_last_state)
    return _selective_scan_fn_nograd(u, delta, A, B, C, D, delta_bias, delta_softplus, oflex, backend, return_last_state)


def _csm_dtype(t, who):
    if not t.is_cuda:
        raise RuntimeError(f"{who}: input must be a CUDA(HIP) tensor")
    if t.dtype not in _ITYPE:
        raise RuntimeError(f"{who}: dtype must be float32, float16 or bfloat16 (got {t.dtype})")
    return _ITYPE[t.dtype]


def _cross_scan(x, in_channel_first=True, out_channel_first=True, one_by_one=False, scans=0, force_torch=False):
    """Reference `cross_scan_fn` (csm_triton.py:501-507).  x: (B,C,H,W) | (B,H,W,C) | one_by_one: (B,4,C,H,W) | (B,H,W,4,C);
    returns (B,4,C,L) if out_channel_first else (B,L,4,C).  scans 0 cross scan, 1 unidirectional, 2 bidirectional.  `force_torch` is accepted and
    ignored (there is one implementation).  Differentiable: the backward is cross_merge_fn with the same flags (its exact adjoint).
    Two combinations deliberately implement the INTENDED permutation, not the reference's mis-indexed output (oracle/refharness/make_golden.py documents both):
    one_by_one + channel-last in + scans = 2, and channel-first in / channel-last out with scans = 1."""
    dt = _csm_dtype(x, "cross_scan_fn")
    if scans not in (0, 1, 2):
        raise RuntimeError(f"cross_scan_fn: scans must be 0, 1 or 2 (got {scans})")
    if x.dim() != (5 if one_by_one else 4):
        raise RuntimeError(f"cross_scan_fn: expected a {5 if one_by_one else 4}-d tensor, got {tuple(x.shape)}")
    if one_by_one:
        B, K, C, H, W = x.shape if in_channel_first else (x.shape[0], x.shape[3], x.shape[4], x.shape[1], x.shape[2])
        if K != 4:
            raise RuntimeError("cross_scan_fn: one_by_one input must hold 4 routes")
    else:
        B, C, H, W = x.shape if in_channel_first else (x.shape[0], x.shape[3], x.shape[1], x.shape[2])
    x = x.contiguous()
    y = torch.empty((B, 4, C, H * W) if out_channel_first else (B, H * W, 4, C), device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device):       # as the reference (csm_triton.py:231): the launch targets x's device, whichever device is current
        _lib.call("xp_cross_scan", ptr(x), ptr(y), c_i(dt), c_i(B), c_i(C), c_i(H), c_i(W), c_i(int(bool(in_channel_first))),
                  c_i(int(bool(out_channel_first))), c_i(int(bool(one_by_one))), c_i(scans), _lib.current_stream(x))
    return y


def _cross_merge(y, in_channel_first=True, out_channel_first=True, one_by_one=False, scans=0, force_torch=False):
    """Reference `cross_merge_fn` (csm_triton.py:511-517).  y: (B,4,C,H,W) if out_channel_first else (B,H,W,4,C) (the scan's OUT layout);
    returns (B,C,L) if in_channel_first else (B,L,C) — one_by_one: (B,4,C,L) / (B,L,4,C).  Adds associate as the reference's do.
    Differentiable: the backward is cross_scan_fn with the same flags (its exact adjoint)."""
    dt = _csm_dtype(y, "cross_merge_fn")
    if scans not in (0, 1, 2):
        raise RuntimeError(f"cross_merge_fn: scans must be 0, 1 or 2 (got {scans})")
    if y.dim() != 5:
        raise RuntimeError(f"cross_merge_fn: expected (B,4,C,H,W) or (B,H,W,4,C), got {tuple(y.shape)}")
    B, K, C, H, W = y.shape if out_channel_first else (y.shape[0], y.shape[3], y.shape[4], y.shape[1], y.shape[2])
    if K != 4:
        raise RuntimeError("cross_merge_fn: input must hold 4 routes")
    y = y.contiguous()
    if one_by_one:
        out = torch.empty((B, 4, C, H * W) if in_channel_first else (B, H * W, 4, C), device=y.device, dtype=y.dtype)
    else:
        out = torch.empty((B, C, H * W) if in_channel_first else (B, H * W, C), device=y.device, dtype=y.dtype)
    with torch.cuda.device(y.device):
        _lib.call("xp_cross_merge", ptr(y), ptr(out), c_i(dt), c_i(B), c_i(C), c_i(H), c_i(W), c_i(int(bool(in_channel_first))),
                  c_i(int(bool(out_channel_first))), c_i(int(bool(one_by_one))), c_i(scans), _lib.current_stream(y))
    return out


class _CrossScanF(torch.autograd.Function):
    """Reference CrossScanTritonF (csm_triton.py:403-450): the backward is the merge kernel with the same flags.  Both kernels index the
    routes through one pixel map and its inverse (cross_scan.hip cs_pixel / cs_pos), so the merge is the scan's exact transpose for every
    flag combination, the two where this build implements the intended permutation included."""

    @staticmethod
    def forward(ctx, x, in_cf, out_cf, one_by_one, scans):
        ctx.flags = (in_cf, out_cf, one_by_one, scans)
        ctx.xshape = x.shape
        return _cross_scan(x, in_cf, out_cf, one_by_one, scans)

    @staticmethod
    def backward(ctx, dy):
        in_cf, out_cf, one_by_one, scans = ctx.flags
        xs = ctx.xshape
        if one_by_one:
            B, C, H, W = (xs[0], xs[2], xs[3], xs[4]) if in_cf else (xs[0], xs[4], xs[1], xs[2])
        else:
            B, C, H, W = xs if in_cf else (xs[0], xs[3], xs[1], xs[2])
        dy = dy.contiguous().view((B, 4, C, H, W) if out_cf else (B, H, W, 4, C))
        return _cross_merge(dy, in_cf, out_cf, one_by_one, scans).view(xs), None, None, None, None


class _CrossMergeF(torch.autograd.Function):
    """Reference CrossMergeTritonF (csm_triton.py:453-500): the backward is the scan kernel with the same flags."""

    @staticmethod
    def forward(ctx, y, in_cf, out_cf, one_by_one, scans):
        ctx.flags = (in_cf, out_cf, one_by_one, scans)
        ctx.yshape = y.shape
        return _cross_merge(y, in_cf, out_cf, one_by_one, scans)

    @staticmethod
    def backward(ctx, dout):
        in_cf, out_cf, one_by_one, scans = ctx.flags
        ys = ctx.yshape
        B, C, H, W = (ys[0], ys[2], ys[3], ys[4]) if out_cf else (ys[0], ys[4], ys[1], ys[2])
        if one_by_one:
            dx = dout.contiguous().view((B, 4, C, H, W) if in_cf else (B, H, W, 4, C))
        else:
            dx = dout.contiguous().view((B, C, H, W) if in_cf else (B, H, W, C))
        return _cross_scan(dx, in_cf, out_cf, one_by_one, scans).view(ys), None, None, None, None


def cross_scan_fn(x, in_channel_first=True, out_channel_first=True, one_by_one=False, scans=0, force_torch=False):
    if _needs_grad(x):
        _csm_dtype(x, "cross_scan_fn")
        if scans not in (0, 1, 2):
            raise RuntimeError(f"cross_scan_fn: scans must be 0, 1 or 2 (got {scans})")
        return _CrossScanF.apply(x, bool(in_channel_first), bool(out_channel_first), bool(one_by_one), scans)
    return _cross_scan(x, in_channel_first, out_channel_first, one_by_one, scans, force_torch)


def cross_merge_fn(y, in_channel_first=True, out_channel_first=True, one_by_one=False, scans=0, force_torch=False):
    if _needs_grad(y):
        _csm_dtype(y, "cross_merge_fn")
        if scans not in (0, 1, 2):
            raise RuntimeError(f"cross_merge_fn: scans must be 0, 1 or 2 (got {scans})")
        return _CrossMergeF.apply(y, bool(in_channel_first), bool(out_channel_first), bool(one_by_one), scans)
    return _cross_merge(y, in_channel_first, out_channel_first, one_by_one, scans, force_torch)


cross_scan_fn.__doc__ = _cross_scan.__doc__
cross_merge_fn.__doc__ = _cross_merge.__doc__
