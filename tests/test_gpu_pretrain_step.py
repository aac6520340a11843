"""The detector's pretraining step on synthetic shapes: XPointNet.forward_single against forward on a pair batch (bit for bit), one
training.pretrain_step on a SyntheticShapes.load_batch batch (finite loss, gradients everywhere but the descriptor head, whose parameters and
Adam moments keep their bits), ten steps on one batch (the loss falls, two runs agree bit for bit).  The small model: EMBED_DIM 32,
DEPTHS [1, 1, 1, 1], 64 x 64, batch 2."""
import pytest
import torch

from tests.training_cases import AUG_CFG, LOSS_CFG, _bits
from xpoint_amd import synth

pytestmark = pytest.mark.gpu
H = W = 64
PRETRAIN_LOSS = dict(LOSS_CFG, descriptor_loss=False)
DESCRIPTOR = "descriptor_head_convolutions."


def _model(drop_path_rate):
    from xpoint_amd import models, training as T
    cfg = synth.xpoint_exp1_config(H, W, vssm={"EMBED_DIM": 32, "DEPTHS": [1, 1, 1, 1]})
    cfg["mixed_precision"] = False
    cfg["use_attention"]["model_parameters"]["MODEL"]["DROP_PATH_RATE"] = drop_path_rate
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    return T.XPointNet.from_model(net.to("cuda").eval()).cuda().train()


def _batch(indices=(4, 9), seed=2):
    from xpoint_amd import synthetic_shapes as ss
    ds = ss.SyntheticShapes({'generation_size': [128, 128], 'image_size': [H, W],
                             'generation': {'generate_background': {'min_kernel_size': 9, 'max_kernel_size': 15}}})
    return ds.load_batch(list(indices), "cuda:0", seed=seed, is_optical=True)


def test_forward_single_is_forward_one_spectrum_at_a_time(gpu_lib):
    from tests.test_gpu_xpoint_training import _pair_batch
    data = _pair_batch(2, H, W, AUG_CFG)
    model = _model(0.2)
    ids = torch.tensor([5, 9])
    pred_o, pred_t, _ = model(data, seed=4, sample_ids=ids)
    for pred, spectrum, k in ((pred_o, 'optical', 0), (pred_t, 'thermal', 1)):
        single = model.forward_single(data[spectrum], seed=4, sample_ids=2 * ids + k)
        assert sorted(single) == sorted(pred)
        for key in pred:
            assert torch.equal(_bits(single[key]), _bits(pred[key])), f"{spectrum}/{key}"
    other = model.forward_single(data['optical'], seed=4, sample_ids=2 * ids + 1)          # the thermal twin's draws: another stochastic depth
    assert other['logits'].shape == pred_o['logits'].shape
    with pytest.raises(ValueError, match="sample_ids"):
        model.forward_single(data['optical'], seed=4, sample_ids=[1, 2, 3])


def test_one_pretrain_step(gpu_lib):
    from xpoint_amd import losses, training as T
    data = _batch()
    assert data['image'].shape == (2, 1, H, W) and bool(data['keypoints'].any())
    model = _model(0.0)
    opt = T.Adam(model.parameters(), lr=1e-4, weight_decay=0)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    torch.manual_seed(3)                                    # the detector loss draws its label noise from torch's generator
    loss, components = T.pretrain_step(model, data, losses.XPointLoss(PRETRAIN_LOSS), opt, seed=0)
    assert bool(torch.isfinite(loss)) and 'descriptor_loss' not in components
    names = [k for k, _ in model.named_parameters()]
    assert any(k.startswith(DESCRIPTOR) for k in names) and any(k.startswith("encoder.") for k in names)
    for k, p in model.named_parameters():
        if k.startswith(DESCRIPTOR):
            assert p.grad is None or not bool(p.grad.any()), k
            assert torch.equal(_bits(p.detach()), _bits(before[k])), k
            st = opt.state[p]
            assert not bool(st['exp_avg'].any()) and not bool(st['exp_avg_sq'].any()), k
            assert torch.equal(_bits(st['exp_avg']), torch.zeros_like(_bits(st['exp_avg']))), k          # +0.0, not -0.0
        else:
            assert k.startswith("encoder.") or k.startswith("detector_head_convolutions."), k
            assert p.grad is not None and bool(p.grad.any()) and bool(torch.isfinite(p.grad).all()), k
            assert not torch.equal(p.detach(), before[k]), k
    with pytest.raises(ValueError, match="descriptor_loss"):
        T.pretrain_step(model, data, losses.XPointLoss(LOSS_CFG), opt, seed=1)


def test_ten_steps_lower_the_loss_and_repeat_bit_for_bit(gpu_lib):
    from xpoint_amd import losses, training as T
    data = _batch()
    loss_fn = losses.XPointLoss(PRETRAIN_LOSS)
    runs = []
    for _ in range(2):
        model = _model(0.2)
        opt = T.Adam(model.parameters(), lr=1e-3, weight_decay=0)
        torch.manual_seed(3)
        history = [T.pretrain_step(model, data, loss_fn, opt, seed=step)[0] for step in range(10)]
        runs.append([_bits(torch.stack(history))] + [_bits(v.float()) for v in model.state_dict().values()])
        values = torch.stack(history).tolist()
        print("pretrain_step losses:", [round(v, 4) for v in values])
        assert all(v == v and abs(v) != float("inf") for v in values) and values[-1] < values[0]
    assert all(torch.equal(a, b) for a, b in zip(*runs))
