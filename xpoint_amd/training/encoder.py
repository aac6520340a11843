"""The whole VMamba encoder (reference xpoint/models/vmamba_src/VMamba.py:1507-1525 VSSM.forward: patch embed :1405-1420, the VSS blocks, downsample
v3 :1433-1440 after stages 0-2, depth_to_space(4) :1500-1505) as ONE trainable module on top of VSSBlock's two autograd functions (DESIGN.md section
19).  The three kinds of strided layer get their backward here: conv3x3_s2_wgrad / conv3x3_s2_dgrad for the stride-2 convolutions, stem_conv_wgrad
for the 1-channel stem.  torch only concatenates / permutes (the depth-to-space adjoint is a view + permute).  No CPU fallback."""
import torch

from .. import _lib
from .ops import (TrainModule, _layernorm, _need_device, colsum_rows, conv3x3_s2_dgrad, conv3x3_s2_fwd, conv3x3_s2_wgrad, gelu_bwd, gelu_fwd,
                  layernorm_bwd, stem_conv, stem_conv_wgrad)
from .vss import VSSBlock, _MlpBranchFn, _SsmBranchFn, drop_path_rates

_ENCODERS = ("encoder.", "encoder_thermal.", "encoder_optical.")


class _ConvS2LnFn(torch.autograd.Function):
    """x (B, H, W, Ci) -> LayerNorm(conv3x3 stride 2 zero pad (x) + bias): patch embed's second half and downsample v3.  w in the reference's
    (Co, Ci, 3, 3)."""

    @staticmethod
    def forward(ctx, x, w, b, ln_w, ln_b):
        st = _lib.current_stream(x)
        B, H, W, Ci = x.shape
        Co = w.shape[0]
        w_ohwi = w.permute(0, 2, 3, 1).contiguous()
        c = conv3x3_s2_fwd(x, w_ohwi, b.contiguous(), stream=st)
        y = _layernorm(c.view(-1, Co), ln_w, ln_b, st).view(c.shape)
        ctx.save_for_backward(x, c, w_ohwi, ln_w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, c, w_ohwi, ln_w = ctx.saved_tensors
        st = _lib.current_stream(x)
        B, H, W, Ci = x.shape
        Co = w_ohwi.shape[0]
        dc, d_ln_w, d_ln_b, sc = layernorm_bwd(dy.contiguous().view(-1, Co), c.view(-1, Co), ln_w, scaled=True, stream=st)
        db = colsum_rows(dc, sc, stream=st)
        dcn = dc.view(c.shape)
        dw = conv3x3_s2_wgrad(x, dcn, dy_scale=sc, stream=st).permute(0, 3, 1, 2)
        dx = conv3x3_s2_dgrad(dcn, w_ohwi, (H, W), dy_scale=sc, stream=st) if ctx.needs_input_grad[0] else None
        return dx, dw, db, d_ln_w, d_ln_b


class _StemFn(torch.autograd.Function):
    """img (B, H, W) -> GELU(LayerNorm(conv3x3 stride 2 (gray replicated to 3 channels) + bias)): patch embed's first half.  w is the reference's
    (E / 2, 3, 3, 3); the forward folds it over the three identical input channels, as models.XPoint.pack_weights does."""

    @staticmethod
    def forward(ctx, img, w, b, ln_w, ln_b):
        st = _lib.current_stream(img)
        Co = w.shape[0]
        w9co = w.double().sum(dim=1).permute(1, 2, 0).reshape(9, Co).float().contiguous()
        c = stem_conv(img, w9co, b, stream=st)
        n = _layernorm(c.view(-1, Co), ln_w, ln_b, st)
        y = gelu_fwd(n, stream=st).view(c.shape)
        ctx.save_for_backward(img, c, n, ln_w)
        return y

    @staticmethod
    def backward(ctx, dy):
        img, c, n, ln_w = ctx.saved_tensors
        st = _lib.current_stream(img)
        Co = c.shape[-1]
        dn, _ = gelu_bwd(dy.contiguous().view(-1, Co), n, stream=st)
        dc, d_ln_w, d_ln_b, sc = layernorm_bwd(dn, c.view(-1, Co), ln_w, scaled=True, stream=st)
        db = colsum_rows(dc, sc, stream=st)
        dw9 = stem_conv_wgrad(img, dc.view(c.shape), dy_scale=sc, stream=st)                   # (9, Co)
        dw = dw9.t().reshape(Co, 1, 3, 3).expand(Co, 3, 3, 3).contiguous()                    # the 9-tap gradient in all three channel slots
        return None, dw, db, d_ln_w, d_ln_b


def _depth_to_space4(x):
    """out[n, 4 h + i, 4 w + j, c] = x[n, h, w, (4 i + j) Cq + c] (VMamba.py:1500-1505) as a view + permute: autograd's adjoint is the inverse permutation."""
    B, H, W, C = x.shape
    return x.view(B, H, W, 4, 4, C // 16).permute(0, 1, 3, 2, 4, 5).reshape(B, 4 * H, 4 * W, C // 16)


class VSSEncoder(TrainModule):
    """The VMamba encoder of models.XPoint as a trainable module, every tensor under the reference's `{encoder}*` names, in its order:

        enc = training.VSSEncoder.from_model(net, encoder="encoder.").cuda().train()
        y = enc(images, seed=step)            # (B, 1, H, W) float32 in [0, 1] -> enc_nhwc (B, H / 8, W / 8, E / 2); y.backward(d_enc) fills every .grad
        net.load_state_dict(enc.state_dict(), strict=False)

    Four stages of `depths` VSS blocks at EMBED_DIM x 1, 2, 4, 8 channels.  Stochastic depth (`.train()`, DROP_PATH_RATE > 0): block i runs at rate
    linspace(0, rate, sum(depths))[i], its draws keyed by (seed, sample id, branch, block index), or given as drop_path_scale = a list of (s1, s2) per
    block.  In `.eval()` the forward records nothing; in `.train()` with every rate 0 it gives the same bits.  The image takes no gradient."""

    def __init__(self, embed_dim=96, depths=(2, 2, 9, 2), mlp_ratio=4.0, drop_path_rate=0.0, encoder="encoder."):
        super().__init__()
        E = self.embed_dim = int(embed_dim)
        self.depths = [int(d) for d in depths]
        if len(self.depths) != 4:
            raise ValueError(f"VSSEncoder: the VMamba encoder needs exactly 4 stages (depths has {len(self.depths)} entries)")
        if E % 8 or E < 8 or E > 128:
            raise ValueError(f"VSSEncoder: embed_dim must be a multiple of 8 in [8, 128] (got {embed_dim})")
        if encoder not in _ENCODERS:
            raise ValueError(f"VSSEncoder: encoder must be 'encoder.', 'encoder_thermal.' or 'encoder_optical.' (got {encoder!r})")
        self.prefix = encoder
        self.mlp_ratio = float(mlp_ratio)
        self.rates = drop_path_rates(self.depths, drop_path_rate)
        self.ss2d_core = "routes"          # the form of every block's SS2D core in training: 'routes' or 'pixel' (training.set_ss2d_core)
        nn = torch.nn
        root = nn.Module()          # parameter containers with the reference's names and order; forward() never calls them
        pe = nn.Module()
        pe.add_module("0", nn.Conv2d(3, E // 2, 3, stride=2, padding=1))
        pe.add_module("2", nn.LayerNorm(E // 2))
        pe.add_module("5", nn.Conv2d(E // 2, E, 3, stride=2, padding=1))
        pe.add_module("7", nn.LayerNorm(E))
        root.patch_embed = pe
        layers = nn.Module()
        i = 0
        for s, depth in enumerate(self.depths):
            C = E * 2 ** s
            layer, blocks = nn.Module(), nn.Module()
            for j in range(depth):
                blk = VSSBlock(C, mlp_ratio=mlp_ratio, drop_path=self.rates[i], stage=s, block=j, encoder=encoder)
                blocks.add_module(str(j), blk.get_submodule(blk.prefix.rstrip(".")))          # the block's parameter set under its reference name
                i += 1
            layer.blocks = blocks
            if s < 3:
                ds = nn.Module()
                ds.add_module("1", nn.Conv2d(C, 2 * C, 3, stride=2, padding=1))
                ds.add_module("3", nn.LayerNorm(2 * C))
                layer.downsample = ds
            layers.add_module(str(s), layer)
        root.layers = layers
        self.add_module(encoder.rstrip("."), root)

    @classmethod
    def from_model(cls, net, encoder="encoder."):
        """The encoder of a loaded models.XPoint (VMamba encoder), as a copy, with the configuration's depths and stochastic-depth rate."""
        if encoder not in _ENCODERS:
            raise ValueError(f"VSSEncoder: encoder must be 'encoder.', 'encoder_thermal.' or 'encoder_optical.' (got {encoder!r})")
        sd = net.state_dict()
        if encoder + "patch_embed.0.weight" not in sd:
            raise RuntimeError(f"VSSEncoder.from_model: the model holds no {encoder}patch_embed.0.weight")
        model = net.config['use_attention']['model_parameters']['MODEL']
        vssm = model['VSSM']
        enc = cls(int(vssm['EMBED_DIM']), list(vssm['DEPTHS']), float(vssm.get('MLP_RATIO', 4.0)), float(model.get('DROP_PATH_RATE', 0.0)), encoder)
        return enc._load_slice(sd)

    def _block_scales(self, B, dev, drop_path_scale, seed, sample_ids):
        """[(s1, s2) or (None, None)] per block: the given factors, or in training the draws keyed by (seed, sample id, branch, block index)."""
        nb = sum(self.depths)
        if drop_path_scale is not None:
            if len(drop_path_scale) != nb:
                raise ValueError(f"VSSEncoder: drop_path_scale must hold one (s1, s2) per block ({nb})")
            out = []
            for pair in drop_path_scale:
                s1, s2 = (torch.as_tensor(s, dtype=torch.float32, device=dev).contiguous() for s in pair)
                if tuple(s1.shape) != (B,) or tuple(s2.shape) != (B,):
                    raise ValueError(f"VSSEncoder: every drop_path_scale entry must be two ({B},) tensors")
                out.append((s1, s2))
            return out
        if not self.training or not any(r > 0.0 for r in self.rates):
            return [(None, None)] * nb
        ids = range(B) if sample_ids is None else [int(v) for v in torch.as_tensor(sample_ids).reshape(-1).tolist()]
        if len(ids) != B:
            raise ValueError(f"VSSEncoder: sample_ids must be ({B},)")
        return [tuple(torch.tensor(drop_path_draws(r, seed, ids, br, i), dtype=torch.float32, device=dev) for br in (0, 1)) if r > 0.0 else (None, None)
                for i, r in enumerate(self.rates)]

    def forward(self, images, drop_path_scale=None, seed=0, sample_ids=None):
        """images (B, 1, H, W) float32 on the GPU, H and W multiples of 32 -> enc_nhwc (B, H / 8, W / 8, embed_dim / 2)."""
        if images.dim() != 4 or images.shape[1] != 1:
            raise RuntimeError("image must be (B,1,H,W)")          # models.XPoint's text: it takes no 3-channel image either
        if images.dtype != torch.float32:
            raise TypeError(f"VSSEncoder: the input must be float32, got {images.dtype}")
        B, _, H, W = images.shape
        if H % 32 or W % 32 or H < 32 or W < 32:
            raise ValueError(f"VSSEncoder: H and W must be multiples of 32 for the VMamba encoder (got {H}x{W})")
        _need_device(images, "VSSEncoder")
        t = self.t
        if t("patch_embed.0.weight").device != images.device:
            raise _lib.XPointHipError("VSSEncoder: parameters and images live on different devices")
        dev = images.device
        scales = self._block_scales(B, dev, drop_path_scale, seed, sample_ids)
        E = self.embed_dim
        with torch.cuda.device(dev), torch.set_grad_enabled(torch.is_grad_enabled() and self.training):
            x = _StemFn.apply(images.contiguous().view(B, H, W), t("patch_embed.0.weight"), t("patch_embed.0.bias"), t("patch_embed.2.weight"),
                              t("patch_embed.2.bias"))
            x = _ConvS2LnFn.apply(x, t("patch_embed.5.weight"), t("patch_embed.5.bias"), t("patch_embed.7.weight"), t("patch_embed.7.bias"))
            i = 0
            for s, depth in enumerate(self.depths):
                C = E * 2 ** s
                _, h, w, _ = x.shape
                for j in range(depth):
                    p = f"layers.{s}.blocks.{j}."
                    s1, s2 = scales[i]
                    r = x.reshape(B * h * w, C)
                    r = _SsmBranchFn.apply(r, s1, (B, h, w), t(p + "norm.weight"), t(p + "norm.bias"), t(p + "op.x_proj_weight"), t(p + "op.A_logs"),
                                           t(p + "op.Ds"), t(p + "op.dt_projs_weight"), t(p + "op.dt_projs_bias"), t(p + "op.out_norm.weight"),
                                           t(p + "op.out_norm.bias"), t(p + "op.in_proj.weight"), t(p + "op.conv2d.weight"), t(p + "op.out_proj.weight"),
                                           self.ss2d_core if self.training else "routes")
                    r = _MlpBranchFn.apply(r, s2, B, t(p + "norm2.weight"), t(p + "norm2.bias"), t(p + "mlp.fc1.weight"), t(p + "mlp.fc1.bias"),
                                           t(p + "mlp.fc2.weight"), t(p + "mlp.fc2.bias"))
                    x = r.view(B, h, w, C)
                    i += 1
                if s < 3:
                    p = f"layers.{s}.downsample."
                    x = _ConvS2LnFn.apply(x, t(p + "1.weight"), t(p + "1.bias"), t(p + "3.weight"), t(p + "3.bias"))
            return _depth_to_space4(x)


def drop_path_draws(p, seed, sample_ids, branch, block):
    """keep / (1 - p) per sample from the Philox stream keyed by (seed, (sample id, branch, block index)): two blocks never share a draw, and a sample's
    draw never depends on its batch neighbours.  (VSSBlock on its own keeps its (seed, 2 sample id + branch) keying.)"""
    import numpy as np
    out = []
    for sid in sample_ids:
        key = [int(seed) & (2 ** 64 - 1), ((int(sid) << 1 | int(branch)) << 20 | int(block)) & (2 ** 64 - 1)]
        out.append(0.0 if np.random.Generator(np.random.Philox(key=key)).random() < p else 1.0 / (1.0 - p))
    return out
