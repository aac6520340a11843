"""The whole VMamba XPoint as ONE trainable model (reference XPoint.py:181-214 forward, :283-323 forward_impl, train.py's `net.parameters()`): the
encoder(s), the detector / descriptor heads and, where the configuration has one, the homography head, forward and backward on the HIP library
(DESIGN.md section 20).

    model = training.XPointNet.from_model(net).cuda().train()
    optimizer = training.Adam(model.parameters(), lr=1e-4)          # or torch.optim.Adam; training.fit is the whole run
    loss, components = training.train_step(model, data, losses.XPointLoss(cfg), optimizer, seed=step)
    net.load_state_dict(model.state_dict(), strict=False)        # the inference model with everything tuned

The parts are training.VSSEncoder, training.XPointHeads and training.RegNetHead as they stand; what connects them is the input gradient of the
trunk's reflection-padded convolution (xp_conv3x3_rp_dgrad_h2), through which the heads' loss reaches every `encoder*.` tensor.  The homography head
reads DETACHED encoder maps, as the reference does (XPoint.py:305/309), so its loss trains `hm_regressor.*` only.  Parameters and buffers appear
under the reference's checkpoint names.  No CPU fallback."""
import torch

from .encoder import VSSEncoder
from .heads import XPointHeads
from .ops import TrainModule, _need_device
from .regnet import RegNetHead

_HEADS = ("detector_head_convolutions", "descriptor_head_convolutions")
MIXED_PRECISION_REFUSAL = ("XPointNet: config['mixed_precision'] = True is not built (no autocast / GradScaler training): the training kernels are the "
                           "f32-grade class only")


class XPointNet(TrainModule):
    """Encoder(s) + heads (+ homography head) of a VMamba models.XPoint that takes pairs.  One VSSEncoder under `encoder.`, or two under
    `encoder_thermal.` / `encoder_optical.` when the configuration is multispectral: a spectrum's batch then goes to the encoder its `is_optical`
    flags name."""

    def __init__(self, encoders, heads, regnet=None):
        super().__init__()
        if not encoders or any(not isinstance(e, VSSEncoder) for e in encoders):
            raise ValueError("XPointNet: encoders must be a non-empty list of VSSEncoder")
        prefixes = sorted(e.prefix for e in encoders)
        if prefixes not in (["encoder."], ["encoder_optical.", "encoder_thermal."]):
            raise ValueError(f"XPointNet: one 'encoder.' or the pair 'encoder_thermal.' / 'encoder_optical.' (got {prefixes})")
        if heads.in_channels != encoders[0].embed_dim // 2 or any(e.embed_dim != encoders[0].embed_dim for e in encoders):
            raise ValueError("XPointNet: the heads' in_channels must be the encoders' embed_dim / 2")
        self.multispectral = len(encoders) == 2
        # the parts keep their forward; their parameter containers are registered HERE, under the reference's names and in its order (encoder,
        # hm_regressor, detector head, descriptor head), so that a part and this module hold the same Parameter objects
        self._encoders = {e.prefix: e for e in encoders}
        self._part = {"heads": heads, "regnet": regnet}          # in a dict: not registered as children a second time
        for pre in (["encoder."] if not self.multispectral else ["encoder_thermal.", "encoder_optical."]):
            self.add_module(pre.rstrip("."), self._encoders[pre].get_submodule(pre.rstrip(".")))
        if regnet is not None:
            self.hm_regressor = regnet.hm_regressor
        for name in _HEADS:
            self.add_module(name, heads.get_submodule(name))

    def _parts(self):
        return list(self._encoders.values()) + [p for p in self._part.values() if p is not None]

    def train(self, mode=True):
        super().train(mode)
        for part in self._parts():
            part.training = bool(mode)          # the parts' children are this module's children: super() has set them
        return self

    @staticmethod
    def check_config(cfg):
        """Refuses a model configuration (the merged `net.config`) that XPointNet does not train: a conv encoder, `mixed_precision: true`, no pairs."""
        ua = cfg['use_attention']
        if not (ua['check'] and ua['type'] == 'VMamba'):
            raise NotImplementedError("XPointNet: config['use_attention'] must select the VMamba encoder (conv-encoder training is not built)")
        if cfg['mixed_precision']:
            raise NotImplementedError(MIXED_PRECISION_REFUSAL)
        if not cfg['takes_pair']:
            raise NotImplementedError("XPointNet: config['takes_pair'] must be True (the losses need both spectra)")

    @classmethod
    def from_model(cls, net):
        """The trainable copy of a loaded models.XPoint: VMamba encoder, takes_pair.  A conv encoder or `mixed_precision: true` is refused."""
        cfg = net.config
        cls.check_config(cfg)
        prefixes = ["encoder_thermal.", "encoder_optical."] if cfg['multispectral'] else ["encoder."]
        regnet = None
        if cfg['homography_regression_head']['check']:
            if cfg['homography_regression_head']['type'] != "RegNet":
                raise NotImplementedError("XPointNet: only config['homography_regression_head']['type'] 'RegNet' is built")
            regnet = RegNetHead.from_model(net)
        return cls([VSSEncoder.from_model(net, encoder=p) for p in prefixes], XPointHeads.from_model(net), regnet)

    def _encoder_of(self, spectrum, n):
        """The encoder a spectrum's batch of n images goes to: by its `is_optical` flags when multispectral (XPoint.py:293-303)."""
        if not self.multispectral:
            return self._encoders["encoder."]
        if 'is_optical' not in spectrum:
            raise RuntimeError("multispectral XPoint: every spectrum's dict needs is_optical (one bool per image)")
        f = torch.as_tensor(spectrum['is_optical'])
        f = (f.unsqueeze(0) if f.dim() == 1 else f)[:, 0].to(torch.bool).cpu()
        if f.numel() != n:
            raise RuntimeError("is_optical must hold one flag per image")
        if bool(f.any()) != bool(f.all()):
            raise ValueError("XPointNet: a spectrum's batch mixes is_optical flags; every image of one batch must go to the same encoder")
        return self._encoders["encoder_optical." if bool(f[0]) else "encoder_thermal."]

    def forward_single(self, spectrum, seed=0, sample_ids=None):
        """One spectrum's dict {'image' (B, 1, H, W), ['is_optical'], ...} (SyntheticShapes.load_batch's) -> the prediction dict `forward` builds
        per spectrum ('logits', 'desc', detached 'encoder_output').  The batch goes to the encoder `_encoder_of` names (its `is_optical` flags when
        multispectral), then to the heads.  sample_ids (B,) are the draw ids THEMSELVES (default 0 .. B - 1): `forward` on a pair batch is
        forward_single(optical, seed, 2 ids) and forward_single(thermal, seed, 2 ids + 1), bit for bit.  The homography head takes no part."""
        images = spectrum['image']
        _need_device(images, "XPointNet")
        n = images.shape[0]
        ids = torch.arange(n) if sample_ids is None else torch.as_tensor(sample_ids).reshape(-1).cpu().to(torch.int64)
        if ids.numel() != n:
            raise ValueError(f"XPointNet: sample_ids must be ({n},)")
        enc = self._encoder_of(spectrum, n)(images, seed=seed, sample_ids=ids)
        pred = self._part["heads"]._forward(enc)
        pred['encoder_output'] = enc.detach().permute(0, 3, 1, 2)
        return pred

    def forward(self, data, seed=0, sample_ids=None):
        """data = {'optical': {'image' (B, 1, H, W), ['is_optical'], ...}, 'thermal': {...}} (augmentation.augment_pair_batch's dict) ->
        (pred_optical, pred_thermal, pred_hm), the reference's triple.  A prediction holds 'logits' (B, 65, H / 8, W / 8), 'desc' (B, D, H / 8, W / 8)
        and the detached 'encoder_output' (B, E / 2, H / 8, W / 8), all channel-last in memory; 'prob' is NOT produced (no loss reads it; the
        inference model gives it).  pred_hm (B, 8) or None.  The encoder and the heads run once per spectrum, so each spectrum has its own BatchNorm
        statistics and the running ones update twice.  seed keys stochastic depth and the homography head's dropout (pass the step number);
        sample_ids (B,) name the pairs (default 0 .. B - 1): pair i draws as sample 2 i (optical) and 2 i + 1 (thermal), so the two spectra never
        share a draw and a pair's draws do not depend on its batch neighbours."""
        opt, th = data['optical'], data['thermal']
        n = opt['image'].shape[0]
        if th['image'].shape[0] != n:
            raise ValueError("XPointNet: the optical and the thermal batch must hold the same number of images")
        ids = torch.arange(n) if sample_ids is None else torch.as_tensor(sample_ids).reshape(-1).cpu().to(torch.int64)
        if ids.numel() != n:
            raise ValueError(f"XPointNet: sample_ids must be ({n},)")
        encoders = [self._encoder_of(spectrum, n) for spectrum in (opt, th)]
        preds, maps = [], []
        for k, spectrum in enumerate((opt, th)):
            images = spectrum['image']
            _need_device(images, "XPointNet")
            enc = encoders[k](images, seed=seed, sample_ids=2 * ids + k)
            pred = self._part["heads"]._forward(enc)
            maps.append(enc.detach())
            pred['encoder_output'] = maps[-1].permute(0, 3, 1, 2)
            preds.append(pred)
        regnet = self._part["regnet"]
        pred_hm = None if regnet is None else regnet(maps[0], maps[1], seed=seed, sample_ids=None if sample_ids is None else ids)
        return preds[0], preds[1], pred_hm


def train_step(model, data, loss_fn, optimizer, seed=0):
    """One training step of the whole model on a pair batch (finetune_step without a frozen net): zero_grad, forward, loss, backward,
    optimizer.step.  `seed` keys the step's stochastic depth and dropout (pass the step number).  Returns (loss, loss_components)."""
    model.train()
    optimizer.zero_grad(set_to_none=True)
    pred, pred2, pred_hm = model(data, seed=seed)
    loss_input = {'data': data, 'pred': pred, 'pred2': pred2}
    if pred_hm is not None:
        loss_input['pred_hm'] = pred_hm
    loss, components = loss_fn(loss_input)
    loss.backward()
    optimizer.step()
    return loss.detach(), components


def pretrain_step(model, data, loss_fn, optimizer, seed=0):
    """`train_step` for a single-image batch (SyntheticShapes.load_batch's dict) and a loss with `descriptor_loss: false`: the detector's
    pretraining step on synthetic shapes.  zero_grad, forward_single, loss, backward, optimizer.step; returns (loss, loss_components).  The
    descriptor head exists (the reference's `descriptor_head: false` builds none) and receives ZERO gradients: under training.Adam with
    weight_decay 0 its parameters and moments keep their bits."""
    if loss_fn.config['descriptor_loss']:
        raise ValueError("pretrain_step: the loss must be configured with 'descriptor_loss': False (a single image has no pair to describe)")
    model.train()
    optimizer.zero_grad(set_to_none=True)
    pred = model.forward_single(data, seed=seed)
    loss, components = loss_fn({'data': data, 'pred': pred})
    loss.backward()
    optimizer.step()
    return loss.detach(), components
