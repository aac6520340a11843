"""One block of the VMamba encoder (reference xpoint/models/vmamba_src/VMamba.py:1153-1234) as a trainable module (csrc/train_vss.hip, DESIGN.md
section 16): LayerNorm, in_proj, depthwise conv + SiLU, x_proj, the dt projection, the SS2D core composed from the differentiable cross-scan /
selective-scan / cross-merge operators — or, with `ss2d_core = "pixel"` (set_ss2d_core), one operator in pixel layout that keeps no route tensor
(csrc/train_ss2d.hip) — out_norm, out_proj and the MLP, with stochastic depth.  Its backward is HIP only and passes the gradient
through to its input, so blocks stack.  Every linear layer takes its input gradient by `_linear_dgrad` (the forward engine on the transposed weight).
Patch embed, the downsamplers and the stacking of the blocks are encoder.py's (VSSEncoder)."""
import math

import torch

from .. import _lib
from .._lib import ptr
from .ops import (TrainModule, _layernorm, _linear, _linear_dgrad, _need_device, _ss2d_core_bwd, _ss2d_core_fwd, add_scaled_rows, check_ss2d_core,
                  colsum_rows, dwconv3x3_silu_bwd, gelu_bwd, gelu_fwd, gemm_tn, layernorm_bwd, scale_grad, ss2d_takes_pixel)


def _dt_block_diagonal(dt_w, R2):
    """dt_projs_weight (4, C, R) as ONE (4 C, 4 (R + 2)) weight over the whole x_proj row: direction k's block under its own dt entries, zeros under
    the B / C entries and the other directions (K = R alone is no multiple of 4: R = 6 at C = 96, 2 at C = 32)."""
    K, C, R = dt_w.shape
    wbd = torch.zeros((K, C, K, R2), dtype=torch.float32, device=dt_w.device)
    for k in range(K):
        wbd[k, :, k, :R] = dt_w[k]
    return wbd.view(K * C, K * R2)


def _branch_bwd_open(dy, s, B, st):
    """A branch's backward begins: dy (M, C) -> (S g, {S, 1 / S}) of g = s[b] dy, the gradient of the branch's last layer (s None: g = dy)."""
    C = dy.shape[1]
    g = dy if s is None else add_scaled_rows(None, dy.view(B, -1, C), s, stream=st).view(-1, C)
    return scale_grad(g, stream=st)


def _branch_bwd_close(dt, x, norm_w, dy, B, want_dx, st):
    """A branch's backward ends: the gradient dt of the first LayerNorm's output -> (dx, dgamma, dbeta), dx with the residual's share dy, or None."""
    dx, dn_w, dn_b, _ = layernorm_bwd(dt, x, norm_w, stream=st)
    if not want_dx:
        return None, dn_w, dn_b
    ones, C = torch.ones(B, dtype=torch.float32, device=x.device), x.shape[1]
    return add_scaled_rows(dy.view(B, -1, C), dx.view(B, -1, C), ones, stream=st).view(-1, C), dn_w, dn_b


def _core_routes_fwd(t3, dtp, xd, R, A, Ds, dt_b, dims):
    """The SS2D core as the composition of the operator-level kernels: three cross-scans into (B, 4, C, L) route tensors, the selective scan, the
    cross-merge -> (ym (M, C), what _core_routes_bwd needs)."""
    from ..kernels import _cross_merge, _cross_scan, _selective_scan_fn_nograd
    B, H, W = dims
    M, C = t3.shape
    R2, L = R + 2, H * W
    xs = _cross_scan(t3.view(B, H, W, C), False, True, False, 0)                   # (B, 4, C, L)
    dts = _cross_scan(dtp.view(B, H, W, 4, C), False, True, True, 0)               # one_by_one, channel-last in: (B, 4, C, L)
    bc = _cross_scan(xd.view(M, 4, R2)[:, :, R:].reshape(B, H, W, 4, 2), False, True, True, 0)      # (B, 4, 2, L): B and C (d_state 1)
    Bs, Cs = bc[:, :, 0:1].contiguous(), bc[:, :, 1:2].contiguous()
    ys, xstate = _selective_scan_fn_nograd(xs.view(B, 4 * C, L), dts.view(B, 4 * C, L), A, Bs, Cs, Ds.detach(), dt_b.detach().reshape(-1), True, want_x=True)
    ym = _cross_merge(ys.view(B, 4, C, H, W), False, True, False, 0).view(M, C)
    return ym, (xs, dts, Bs, Cs, xstate)


def _core_routes_bwd(dym, kept, A, Ds, dt_b, dims):
    """dym (M, C) -> (du (M, C), ddtp (M, 4 C), dbc (M, 4, 2), dA, dD, ddt_bias): the adjoints of _core_routes_fwd's launches."""
    from ..kernels import _cross_merge, _cross_scan, selective_scan_bwd
    xs, dts, Bs, Cs, xstate = kept
    B, H, W = dims
    M, C = dym.shape
    L = H * W
    dys = _cross_scan(dym.view(B, H, W, C), False, True, False, 0)                 # the merge's adjoint: (B, 4, C, L)
    du, ddelta, dA, dB, dC, dD, ddb = selective_scan_bwd(xs.view(B, 4 * C, L), dts.view(B, 4 * C, L), A, Bs, Cs, Ds, dt_b.reshape(-1),
                                                         dys.view(B, 4 * C, L), xstate, True, 1)
    dt3 = _cross_merge(du.view(B, 4, C, H, W), False, True, False, 0).view(M, C)   # the scan's adjoint
    ddtp = _cross_merge(ddelta.view(B, 4, C, H, W), False, True, True, 0).view(M, 4 * C)
    dbc = _cross_merge(torch.cat([dB, dC], 2).view(B, 4, 2, H, W), False, True, True, 0).view(M, 4, 2)
    return dt3, ddtp, dbc, dA, dD, ddb


class _SsmBranchFn(torch.autograd.Function):
    """x (M, C) rows of (B, H, W) -> x + s[b] out_proj(out_norm(SS2D(silu(dwconv(in_proj(LN(x))))))); s None: no factor, the residual rides in the
    out_proj launch.  Parameters in the reference's order.  core: the form of the SS2D core between dtp and ym, 'routes' (_core_routes_fwd / _bwd) or
    'pixel' (ops.ss2d_core's launches, at the shapes ss2d_takes_pixel names)."""

    @staticmethod
    def forward(ctx, x, s, dims, norm_w, norm_b, xproj_w, A_logs, Ds, dt_w, dt_b, on_w, on_b, in_w, conv_w, out_w, core="routes"):
        B, H, W = dims
        M, C = x.shape
        R = dt_w.shape[2]
        R2, L = R + 2, H * W
        st = _lib.current_stream(x)
        t1 = _layernorm(x, norm_w, norm_b, st)
        t2 = _linear(t1, in_w, st)
        w9c = conv_w.reshape(C, 9).t().contiguous()
        t3 = torch.empty_like(t2)
        _lib.call("xp_dwconv3x3_silu", ptr(t2), ptr(w9c), ptr(t3), B, H, W, C, st)
        xd = _linear(t3, xproj_w.reshape(4 * R2, C), st)                              # x_proj in pixel layout: (M, 4 (R + 2))
        wbd = _dt_block_diagonal(dt_w, R2)
        dtp = _linear(xd, wbd, st)                                                     # (M, 4 C): every direction's dt at its pixel
        A = -torch.exp(A_logs.detach().float())
        pixel = check_ss2d_core(core, "VSSBlock") == "pixel" and ss2d_takes_pixel(B, H, W, C)
        if pixel:
            ym, ws = _ss2d_core_fwd(t3, dtp, xd, R, A, Ds.detach(), dt_b.detach(), dims, 0, st)
            kept = (ws,)          # the chunk states; dtp, a route tensor's size, is not kept: the backward repeats its GEMM (the same bits)
        else:
            ym, kept = _core_routes_fwd(t3, dtp, xd, R, A, Ds, dt_b, dims)
        yn = _layernorm(ym, on_w, on_b, st)
        if s is None:
            out = _linear(yn, out_w, st, res=x)
        else:
            out = add_scaled_rows(x.view(B, L, C), _linear(yn, out_w, st).view(B, L, C), s, stream=st).view(M, C)
        ctx.dims, ctx.has_s, ctx.pixel = dims, s is not None, pixel          # the backward takes the form the forward took
        ctx.save_for_backward(x, t1, t2, t3, xd, A, ym, yn, w9c, wbd, norm_w, xproj_w, Ds, dt_w, dt_b, on_w, in_w, out_w, *kept,
                              *(() if s is None else (s,)))
        return out

    @staticmethod
    def backward(ctx, dy):
        saved = ctx.saved_tensors
        x, t1, t2, t3, xd, A, ym, yn, w9c, wbd, norm_w, xproj_w, Ds, dt_w, dt_b, on_w, in_w, out_w = saved[:18]
        kept = saved[18:len(saved) - ctx.has_s]
        B, H, W = ctx.dims
        M, C = x.shape
        R = dt_w.shape[2]
        R2, L = R + 2, H * W
        st = _lib.current_stream(x)
        dy = dy.contiguous()
        gs, sc = _branch_bwd_open(dy, saved[-1] if ctx.has_s else None, B, st)
        d_out_w = gemm_tn(gs, yn, p_scale=sc, stream=st)
        dyn = _linear_dgrad(gs, sc, out_w, st)
        dym, d_on_w, d_on_b, _ = layernorm_bwd(dyn, ym, on_w, stream=st)
        if ctx.pixel:
            dt3, ddtp, dbc, dA, dD, ddb = _ss2d_core_bwd(dym, t3, _linear(xd, wbd, st), xd, R, A, Ds, dt_b, kept[0], ctx.dims, 0, st)
        else:
            dt3, ddtp, dbc, dA, dD, ddb = _core_routes_bwd(dym, kept, A, Ds, dt_b, ctx.dims)
        # the dt projection: one block-diagonal GEMM over the whole x_proj row; its weight gradient is the diagonal blocks of one gemm_tn result
        g2, sc2 = scale_grad(ddtp, out=ddtp, stream=st)
        d_wbd = gemm_tn(g2, xd, p_scale=sc2, stream=st).view(4, C, 4, R2)
        d_dt_w = torch.stack([d_wbd[k, :, k, :R] for k in range(4)], 0)
        dxd = _linear_dgrad(g2, sc2, wbd, st)                                          # exact zeros under the B / C entries: wbd's columns there are 0
        dxd.view(M, 4, R2)[:, :, R:] = dbc
        g3, sc3 = scale_grad(dxd, out=dxd, stream=st)
        xw = xproj_w.reshape(4 * R2, C)
        d_xproj = gemm_tn(g3, t3, p_scale=sc3, stream=st).view(4, R2, C)
        dt3 = _linear_dgrad(g3, sc3, xw, st, res=dt3)                                  # + the scan's share, in the epilogue
        dt2, dw9c, sc4 = dwconv3x3_silu_bwd(t2.view(B, H, W, C), w9c, dt3.view(B, H, W, C), scaled=True, stream=st)
        dt2 = dt2.view(M, C)
        d_conv_w = dw9c.t().reshape(C, 1, 3, 3)
        d_in_w = gemm_tn(dt2, t1, p_scale=sc4, stream=st)
        dt1 = _linear_dgrad(dt2, sc4, in_w, st)
        dx, d_norm_w, d_norm_b = _branch_bwd_close(dt1, x, norm_w, dy, B, ctx.needs_input_grad[0], st)
        # A = -exp(A_logs): dA_logs = dA A (parameter-sized)
        return (dx, None, None, d_norm_w, d_norm_b, d_xproj, (dA.view(A.shape) * A).view(4 * C, 1), dD.view(Ds.shape), d_dt_w, ddb.view(4, C), d_on_w, d_on_b, d_in_w,
                d_conv_w, d_out_w, None)


class _MlpBranchFn(torch.autograd.Function):
    """x (M, C) rows of B samples -> x + s[b] fc2(GELU(fc1(LN(x)))); s None: no factor, the residual rides in the fc2 launch."""

    @staticmethod
    def forward(ctx, x, s, batch, n_w, n_b, w1, b1, w2, b2):
        M, C = x.shape
        st = _lib.current_stream(x)
        t = _layernorm(x, n_w, n_b, st)
        keep = any(ctx.needs_input_grad)
        if keep:
            pre = _linear(t, w1, st, bias=b1)
            h = gelu_fwd(pre, stream=st)
        else:                    # nothing to keep: the GELU rides in fc1's epilogue, the inference path's launch (the same bits)
            pre, h = None, _linear(t, w1, st, bias=b1, act=1)
        if s is None:
            out = _linear(h, w2, st, bias=b2, res=x)
        else:
            out = add_scaled_rows(x.view(batch, -1, C), _linear(h, w2, st, bias=b2).view(batch, -1, C), s, stream=st).view(M, C)
        ctx.batch, ctx.has_s = batch, s is not None
        if keep:
            ctx.save_for_backward(x, t, pre, h, n_w, w1, w2, *(() if s is None else (s,)))
        return out

    @staticmethod
    def backward(ctx, dy):
        x, t, pre, h, n_w, w1, w2 = ctx.saved_tensors[:7]
        B = ctx.batch
        st = _lib.current_stream(x)
        dy = dy.contiguous()
        gs, sc = _branch_bwd_open(dy, ctx.saved_tensors[7] if ctx.has_s else None, B, st)
        db2 = colsum_rows(gs, sc, stream=st)
        dw2 = gemm_tn(gs, h, p_scale=sc, stream=st)
        dh = _linear_dgrad(gs, sc, w2, st)
        dpre, sc1 = gelu_bwd(dh, pre, scaled=True, stream=st)
        db1 = colsum_rows(dpre, sc1, stream=st)
        dw1 = gemm_tn(dpre, t, p_scale=sc1, stream=st)
        dt = _linear_dgrad(dpre, sc1, w1, st)
        dx, dn_w, dn_b = _branch_bwd_close(dt, x, n_w, dy, B, ctx.needs_input_grad[0], st)
        return dx, None, None, dn_w, dn_b, dw1, db1, dw2, db2


def drop_path_rates(depths, drop_path_rate):
    """The reference's per-block stochastic-depth rates: linspace(0, DROP_PATH_RATE, sum(DEPTHS)) (VMamba.py:1289), as a flat list."""
    return [float(v) for v in torch.linspace(0, float(drop_path_rate), int(sum(depths)))]


def _drop_path_draws(p, seed, sample_ids, branch):
    """keep / (1 - p) per sample from the Philox stream keyed by (seed, 2 sample id + branch): a sample's draw never depends on its batch neighbours."""
    import numpy as np
    out = []
    for sid in sample_ids:
        u = np.random.Generator(np.random.Philox(key=[int(seed) & (2 ** 64 - 1), 2 * int(sid) + branch])).random()
        out.append(0.0 if u < p else 1.0 / (1.0 - p))
    return out


class VSSBlock(TrainModule):
    """One VSS block of the VMamba encoder (reference VMamba.py:1153-1234; SS2D forwardv2 / forward_corev2 with v05_noz, d_state 1, SSM_RATIO 1.0, no
    convolution bias) with the reference's state_dict names under `{encoder}layers.{stage}.blocks.{block}.`:

        blk = training.VSSBlock.from_model(net, stage=0, block=1).cuda().train()
        y = blk(x_nhwc, seed=step)                                  # (B, H, W, C) -> (B, H, W, C); x may require grad: blocks stack
        net.load_state_dict(blk.state_dict(), strict=False)         # the inference model with the tuned block

    x = x + drop_path(op(norm(x))); x = x + drop_path(mlp(norm2(x))).  Dense layers run on the split-fp16 engine (their operands must stay below 65504 in
    magnitude: LayerNorm outputs and O(1) activations in this network); gradients of any finite range are accepted.  Stochastic depth (`.train()` and
    drop_path > 0): each branch of each sample is multiplied by keep / (1 - p), the draws keyed by (seed, sample id, branch) or given as
    drop_path_scale = (s1, s2).  In `.eval()`, or with rate 0, the residual adds ride in the dense launches, as in the inference path.
    `t(leaf)` takes the name below the block's prefix."""

    def __init__(self, dim, dt_rank=None, mlp_ratio=4.0, drop_path=0.0, stage=0, block=0, encoder="encoder."):
        super().__init__()
        C = self.dim = int(dim)
        if C % 4 or C > 1024 or C < 4:
            raise ValueError(f"VSSBlock: dim must be a multiple of 4 in [4, 1024] (got {dim})")
        R = self.dt_rank = int(dt_rank) if dt_rank is not None else (C + 15) // 16
        H4 = self.hidden = int(C * mlp_ratio)
        if H4 % 4:
            raise ValueError(f"VSSBlock: the MLP width {H4} must be a multiple of 4")
        self.drop_path = float(drop_path)
        if not 0.0 <= self.drop_path < 1.0:
            raise ValueError(f"VSSBlock: drop_path must be in [0, 1) (got {drop_path})")
        if encoder not in ("encoder.", "encoder_thermal.", "encoder_optical."):
            raise ValueError(f"VSSBlock: encoder must be 'encoder.', 'encoder_thermal.' or 'encoder_optical.' (got {encoder!r})")
        self.prefix = f"{encoder}layers.{int(stage)}.blocks.{int(block)}."
        self.ss2d_core = "routes"          # the form of the SS2D core in training: 'routes' or 'pixel' (set_ss2d_core)
        nn = torch.nn
        blk = nn.Module()          # parameter containers with the reference's names, order and initialisation; forward() never calls them
        blk.norm = nn.LayerNorm(C)
        op = nn.Module()
        op.x_proj_weight = nn.Parameter(torch.empty(4, R + 2, C).uniform_(-C ** -0.5, C ** -0.5))
        op.A_logs = nn.Parameter(torch.zeros(4 * C, 1))                                  # log(arange(1, d_state + 1)), d_state 1
        op.Ds = nn.Parameter(torch.ones(4 * C))
        op.dt_projs_weight = nn.Parameter(torch.empty(4, C, R).uniform_(-R ** -0.5, R ** -0.5))
        dt = torch.exp(torch.rand(4, C) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3)).clamp(min=1e-4)
        op.dt_projs_bias = nn.Parameter(dt + torch.log(-torch.expm1(-dt)))               # softplus^-1 (VMamba.py:196-211)
        op.out_norm = nn.LayerNorm(C)
        op.in_proj = nn.Linear(C, C, bias=False)
        op.conv2d = nn.Conv2d(C, C, 3, padding=1, groups=C, bias=False)
        op.out_proj = nn.Linear(C, C, bias=False)
        blk.op = op
        blk.norm2 = nn.LayerNorm(C)
        mlp = nn.Module()
        mlp.fc1, mlp.fc2 = nn.Linear(C, H4), nn.Linear(H4, C)
        blk.mlp = mlp
        node = self
        parts = self.prefix.rstrip(".").split(".")
        for name in parts[:-1]:
            child = nn.Module()
            node.add_module(name, child)
            node = child
        node.add_module(parts[-1], blk)

    @classmethod
    def from_model(cls, net, stage, block, encoder="encoder."):
        """Block `block` of stage `stage` of a loaded models.XPoint (VMamba encoder), as a copy, with the reference's stochastic-depth rate for
        that block.  encoder: 'encoder.', or 'encoder_thermal.' / 'encoder_optical.' of a multispectral model."""
        sd = net.state_dict()
        pre = f"{encoder}layers.{int(stage)}.blocks.{int(block)}."
        if pre + "norm.weight" not in sd:
            raise RuntimeError(f"VSSBlock.from_model: the model holds no {pre}norm.weight")
        model = net.config['use_attention']['model_parameters']['MODEL']
        depths = list(model['VSSM']['DEPTHS'])
        rates = drop_path_rates(depths, model.get('DROP_PATH_RATE', 0.0))
        C, R = sd[pre + "norm.weight"].shape[0], sd[pre + "op.dt_projs_weight"].shape[2]
        blk = cls(C, dt_rank=R, mlp_ratio=sd[pre + "mlp.fc1.weight"].shape[0] / C, drop_path=rates[sum(depths[:int(stage)]) + int(block)],
                  stage=stage, block=block, encoder=encoder)
        return blk._load_slice(sd)

    def forward(self, x_nhwc, drop_path_scale=None, seed=0, sample_ids=None):
        """x_nhwc (B, H, W, C) float32 on the GPU -> (B, H, W, C).  drop_path_scale = (s1, s2): two (B,) tensors that replace the stochastic-depth
        draws of the two branches; else, in training with drop_path > 0, the draws are keyed by (seed, sample_ids[b], branch) (sample_ids: default
        0 .. B - 1)."""
        _need_device(x_nhwc, "VSSBlock")
        if x_nhwc.dtype != torch.float32:
            raise TypeError(f"VSSBlock: the input must be float32, got {x_nhwc.dtype}")
        C = self.dim
        if x_nhwc.dim() != 4 or x_nhwc.shape[-1] != C:
            raise ValueError(f"VSSBlock: x_nhwc must be (B, H, W, {C}), got {tuple(x_nhwc.shape)}")
        if self.t("norm.weight").device != x_nhwc.device:
            raise _lib.XPointHipError("VSSBlock: parameters and x_nhwc live on different devices")
        B, H, W, _ = x_nhwc.shape
        dev = x_nhwc.device
        s1 = s2 = None
        if drop_path_scale is not None:
            s1, s2 = (torch.as_tensor(s, dtype=torch.float32, device=dev).contiguous() for s in drop_path_scale)
            if tuple(s1.shape) != (B,) or tuple(s2.shape) != (B,):
                raise ValueError(f"VSSBlock: drop_path_scale must be two ({B},) tensors")
        elif self.training and self.drop_path > 0.0:
            ids = range(B) if sample_ids is None else [int(v) for v in torch.as_tensor(sample_ids).reshape(-1).tolist()]
            if len(ids) != B:
                raise ValueError(f"VSSBlock: sample_ids must be ({B},)")
            s1, s2 = (torch.tensor(_drop_path_draws(self.drop_path, seed, ids, br), dtype=torch.float32, device=dev) for br in (0, 1))
        x = x_nhwc.contiguous().view(B * H * W, C)
        t = self.t
        with torch.cuda.device(dev):
            x = _SsmBranchFn.apply(x, s1, (B, H, W), t("norm.weight"), t("norm.bias"), t("op.x_proj_weight"), t("op.A_logs"), t("op.Ds"),
                                   t("op.dt_projs_weight"), t("op.dt_projs_bias"), t("op.out_norm.weight"), t("op.out_norm.bias"),
                                   t("op.in_proj.weight"), t("op.conv2d.weight"), t("op.out_proj.weight"), self.ss2d_core if self.training else "routes")
            x = _MlpBranchFn.apply(x, s2, B, t("norm2.weight"), t("norm2.bias"), t("mlp.fc1.weight"), t("mlp.fc1.bias"), t("mlp.fc2.weight"),
                                   t("mlp.fc2.bias"))
        return x.view(B, H, W, C)


def set_ss2d_core(module, kind):
    """Chooses the form of the SS2D core for every VSS block under `module` (a VSSBlock, VSSEncoder or XPointNet): 'routes', the default — the
    cross-scan / selective-scan / cross-merge composition over (B, 4, C, L) route tensors — or 'pixel', the one operator in pixel layout
    (ops.ss2d_core), which keeps no route tensor.  The two agree to rounding, not bit for bit.  `.eval()` forwards are the same under both.  Returns
    the module."""
    check_ss2d_core(kind, "set_ss2d_core")
    # the attribute lives on VSSBlock and on VSSEncoder (which runs its blocks itself); XPointNet keeps its encoders in `_encoders`, outside its children
    holders = [h for m in module.modules() for h in (m, *getattr(m, "_encoders", {}).values()) if isinstance(getattr(h, "ss2d_core", None), str)]
    for h in holders:
        h.ss2d_core = kind
    if not holders:
        raise ValueError(f"set_ss2d_core: {type(module).__name__} holds no VSS block")
    return module
