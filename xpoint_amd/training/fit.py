"""training.fit: the training run of the reference's train.py for what the HIP library trains — the VMamba XPoint on pairs, `mixed_precision: false`,
a folder dataset.  `python -m xpoint_amd.cli train -y cfg.yaml [-w e20.model]` is its command line.

    history = training.fit(yaml.safe_load(open("configs/cmt.yaml")), weight_file=None, device="cuda:0", seed=0)

Config keys, the reference's: training.{output_directory, n_epochs, learningrate, weight_decay, batchsize, save_every_n_epoch, use_writer},
training.scheduler.{use_scheduler, type: StepLR | ExponentialLR, step_size, gamma}, training.validation.{compute_validation_loss, every_nth_epoch,
keypoints}; `num_worker` and `allow_gpu` are accepted and ignored; `training.mixed_precision: true` is refused with XPointNet's message.  New,
optional: training.validation.foldername (the folder-mode counterpart of the reference's `filename`), training.log_every (a `batch_loss` record every
that many steps), training.max_norm (global-norm clipping, off by default as in the reference), training.ss2d_core ('routes', the default, or 'pixel':
training.set_ss2d_core; checked before anything is built and written into params.yaml), training.validation.compute_metrics with
training.validation.metric_thresholds (default [3]): after the validation loss, evaluation.compute_metrics_batched(reference_quirks=False) of the
inference network on the validation pairs (prediction settings from config['prediction'] over predict.DEFAULT_PREDICTION) — `validation_metrics`
in the history and validation/{repeatability, nn_map, m_score, h_correctness}_<th> in learningcurve.jsonl; without the key nothing changes.

What is kept from train.py: params.yaml with the four sections at the start; the weights of -w loaded with strict=False after
fix_model_weigth_keys, zero loaded keys refused; the start epoch parsed from an `e<N>.model` name; loss.space_to_depth_ratio from the model; Adam with
weight decay; the scheduler stepped once per epoch after the checkpoint; validation when epoch % every_nth_epoch == 0, on the dataset's own
augmentation block; `e<N>.model` every save_every_n_epoch epochs and `latest.model` at the end, state dicts under the reference's names; the
scalar names of its SummaryWriter.

Stated differences:
  - Validation runs in .eval() under no_grad.  The reference never leaves train mode there, so its validation batches are normalised with their own
    statistics and MOVE the BatchNorm running statistics; here validation leaves every buffer untouched.
  - The optimiser is training.Adam: torch.optim.Adam's update, with a device-side guard that skips a step whose gradients are not finite (the
    reference has this only under GradScaler); the number of skipped steps is logged.
  - Shuffling, the augmentation draws and the loss's label noise are seeded per (seed, epoch), and train_step's seed is the global step number, so an
    epoch is reproducible without replaying the earlier ones (the reference draws everything from the process-wide generators).
  - Next to each `e<N>.model` an `e<N>.optim` holds the optimiser and scheduler state; `fit(..., weight_file=".../e<N>.model")` loads it when it is
    there and resume_optimizer holds, and then continues the run bit for bit.  The reference always restarts the optimiser.
  - The epoch's loss accumulates on the device and is read once per epoch (plus once per log_every steps); the reference calls loss.item() every
    step.  XPointLoss itself still reads its components back (losses.py), which this loop does not change.
  - Augmentation runs per batch on the GPU (augmentation.augment_pair_batch), not per sample in the dataset; ImagePairDataset keeps refusing the
    `augmentation` key.  With use_writer the scalars go to `learningcurve.jsonl`, one JSON record per line (tensorboard is not required).
  - The warped image is labelled with the warped points (augment_pair_batch's labels_follow_warp default).
No CPU fallback."""
import copy
import json
import os
import random

import numpy as np
import torch
import yaml

from .. import _lib
from .model import MIXED_PRECISION_REFUSAL, XPointNet, train_step
from .ops import check_ss2d_core
from .optim import Adam
from .vss import set_ss2d_core


def _start_epoch(weight_file):
    """train.py:71-74: the N of an `e<N>.model` file name, else 0."""
    try:
        return int(os.path.split(weight_file)[-1].split('.')[0][1:])
    except ValueError:
        return 0


def _seed_epoch(seed, epoch):
    """The generators of one epoch, keyed by (seed, epoch): the shuffle, the photometric scalars; Python's and numpy's process-wide generators (the
    homographies and the crop offsets draw from them) and torch's (the detector loss's label noise)."""
    keys = np.random.SeedSequence([int(seed), int(epoch)]).generate_state(4)
    random.seed(int(keys[2]))
    np.random.seed(int(keys[2]))
    torch.manual_seed(int(keys[3]))
    return np.random.default_rng(int(keys[0])), np.random.default_rng(int(keys[1]))


def _add(total, components):
    for k, v in components.items():
        total[k] = total.get(k, 0.0) + float(v)


def _dataset(ds_cfg):
    from .. import datasets
    ds_cfg = dict(ds_cfg)
    ds_cfg.pop('type', None)
    if ds_cfg.get('keypoints_filename') is None:
        raise ValueError("fit: the dataset needs keypoint labels (keypoints_filename: the .npz `cli export` writes)")
    return datasets.ImagePairDataset(ds_cfg)


def validation_metric_thresholds(val):
    """The thresholds of the matching metrics of a validation pass, or None when they are off.  training.validation.compute_metrics is read only
    when a validation folder is in use (compute_validation_loss); metric_thresholds (default [3]) must be a non-empty list of at most 16
    positive numbers, each of which serves as repeatability distance, keypoint distance and warp-error threshold."""
    val = val or {}
    if not val.get('compute_validation_loss', False) or not val.get('compute_metrics', False):
        return None
    if val.get('foldername') is None:
        raise ValueError("fit: training.validation.foldername is needed (folder datasets only; the reference's `filename` is an HDF5 file)")
    ths = val.get('metric_thresholds', [3])
    ok = isinstance(ths, (list, tuple)) and 1 <= len(ths) <= 16 and all(
        isinstance(t, (int, float)) and not isinstance(t, bool) and np.isfinite(t) and t > 0 for t in ths)
    if not ok or len(set(ths)) != len(ths):
        raise ValueError(f"fit: training.validation.metric_thresholds must be a list of 1 to 16 distinct positive numbers (got {ths!r})")
    return list(ths)


def _validation_metrics(net, model, val_dataset, bs, device, config, ths):
    """evaluation.compute_metrics_batched(reference_quirks=False) of the inference network with the model's current weights on the validation
    pairs as they are (no augmentation: identity homographies), as plain numbers per threshold."""
    from .. import evaluation, predict
    net.load_state_dict(model.state_dict(), strict=False)
    net.eval()
    cfg = {'prediction': predict._cfg(config.get('prediction'))}
    ransac = cfg['prediction'].get('reprojection_threshold', 3)

    def loader():
        for k in range(0, len(val_dataset), bs):
            yield val_dataset.load_batch(list(range(k, min(k + bs, len(val_dataset)))), device)

    out = evaluation.compute_metrics_batched(net, loader(), device, cfg, cfg['prediction']['detection_threshold'], list(ths), list(ths), list(ths),
                                             [ransac], reference_quirks=False)
    hom = out['homography'][ransac]
    return {'repeatability': {th: float(out['repeatability']['repeatability_mean'][th]) for th in ths},
            'nn_map': {th: float(out['descriptor'][th]['nn_map']) for th in ths},
            'm_score': {th: float(out['descriptor'][th]['m_score']) for th in ths},
            'h_correctness': {th: float(hom['h_correctness']['epsilon_warp_th' + str(th)]) for th in ths},
            'average_h_error': float(hom['average_h_error']),
            'n_kp_optical': float(out['repeatability']['n_kp_optical']), 'n_kp_thermal': float(out['repeatability']['n_kp_thermal'])}


def fit(config, weight_file=None, device="cuda:0", seed=0, resume_optimizer=True):
    """Trains models.XPoint(config['model']) as the module docstring says and returns the per-epoch means: {'epoch': [N, ...], 'loss': [...],
    'components': [{...}, ...], 'validation_loss': [... or None], 'validation_components': [...], 'learning_rate': [...], 'skipped_steps': [...]}
    (skipped_steps: the optimiser's count at the end of each epoch)."""
    from .. import augmentation, losses, models, utils
    tr = config['training']
    if tr.get('mixed_precision', False):
        raise NotImplementedError(MIXED_PRECISION_REFUSAL)
    core = check_ss2d_core(tr.get('ss2d_core', 'routes'), "fit: training.ss2d_core")
    metric_ths = validation_metric_thresholds(tr.get('validation'))
    net = getattr(models, config['model'].get('type', 'XPoint'))(config['model'])
    XPointNet.check_config(net.config)
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.XPointHipError("fit: training needs a GPU device (xpoint_amd has no CPU fallback)")

    out_dir = str(tr['output_directory'])
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'params.yaml'), 'wt') as fh:
        yaml.safe_dump({'model': config['model'], 'loss': config['loss'], 'training': dict(config['training'], ss2d_core=core), 'dataset': config['dataset']}, fh)

    ds_cfg = copy.deepcopy(config['dataset'])
    aug_cfg = ds_cfg.pop('augmentation', None) or {}
    dataset = _dataset(ds_cfg)
    val = tr.get('validation') or {}
    val_dataset = None
    if val.get('compute_validation_loss', False):
        if val.get('foldername') is None:
            raise ValueError("fit: training.validation.foldername is needed (folder datasets only; the reference's `filename` is an HDF5 file)")
        val_dataset = _dataset(dict(ds_cfg, foldername=val['foldername'], keypoints_filename=val.get('keypoints')))

    start_epoch = 0
    if weight_file is not None:
        start_epoch = _start_epoch(weight_file)
        weights = utils.fix_model_weigth_keys(torch.load(weight_file, map_location=torch.device('cpu')))
        missing, unexpected = net.load_state_dict(weights, strict=False)
        loaded = set(weights.keys()) - set(missing)
        print(f"Successfully loaded {len(loaded)} keys.\nMissing keys: {len(missing)}\nUnexpected keys: {len(unexpected)}")
        if len(loaded) < 1:
            raise ValueError("No weights were loaded correctly! Please check the model and weights file.")
    net.to(device)
    print('Training on device: {}'.format(device))

    with torch.cuda.device(device):
        model = set_ss2d_core(XPointNet.from_model(net), core).to(device).train()
        has_hm = any(k.startswith("hm_regressor.") for k, _ in model.named_parameters())
        loss_cfg = {k: v for k, v in config['loss'].items() if k != 'type'}
        loss_cfg['space_to_depth_ratio'] = net.get_encoder_downsample_ratio()
        loss_fn = getattr(losses, config['loss'].get('type', 'XPointLoss'))(loss_cfg)

        optimizer = Adam(model.parameters(), lr=float(tr['learningrate']), weight_decay=float(tr.get('weight_decay', 0.0)),
                         max_norm=tr.get('max_norm'))
        scheduler = None
        sch = tr.get('scheduler') or {}
        if sch.get('use_scheduler', False):
            from torch.optim import lr_scheduler
            if sch['type'] == 'StepLR':
                scheduler = lr_scheduler.StepLR(optimizer, step_size=sch['step_size'], gamma=sch['gamma'])
            elif sch['type'] == 'ExponentialLR':
                scheduler = lr_scheduler.ExponentialLR(optimizer, gamma=sch['gamma'])
            else:
                raise ValueError(f"fit: training.scheduler.type must be StepLR or ExponentialLR (got {sch['type']!r})")
        if weight_file is not None and resume_optimizer and start_epoch > 0:
            sibling = os.path.join(os.path.dirname(weight_file), f"e{start_epoch}.optim")
            if os.path.basename(weight_file) == f"e{start_epoch}.model" and os.path.exists(sibling):
                saved = torch.load(sibling, map_location=torch.device('cpu'))
                optimizer.load_state_dict(saved['optimizer'])
                if scheduler is not None and saved.get('scheduler') is not None:
                    scheduler.load_state_dict(saved['scheduler'])
                print(f"Resumed the optimiser from {sibling}")

        n_epochs, bs = int(tr['n_epochs']), int(tr['batchsize'])
        save_every, log_every = int(tr.get('save_every_n_epoch', 0)), int(tr.get('log_every', 0) or 0)
        steps_per_epoch = (len(dataset) + bs - 1) // bs
        writer = open(os.path.join(out_dir, 'learningcurve.jsonl'), 'at') if tr.get('use_writer', False) else None

        def write(tag, step, scalars):
            if writer is not None:
                writer.write(json.dumps({'tag': tag, 'step': int(step), 'scalars': scalars}) + "\n")
                writer.flush()

        def save(name):
            net.load_state_dict(model.state_dict(), strict=False)
            torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, os.path.join(out_dir, name))

        history = {k: [] for k in ('epoch', 'loss', 'components', 'validation_loss', 'validation_components', 'learning_rate', 'skipped_steps')}
        try:
            for epoch in range(start_epoch, n_epochs):
                rng_shuffle, rng_aug = _seed_epoch(seed, epoch)
                order = rng_shuffle.permutation(len(dataset))
                epoch_loss = torch.zeros((), dtype=torch.float32, device=device)
                epoch_components = {}
                for i in range(steps_per_epoch):
                    step = epoch * steps_per_epoch + i
                    batch = dataset.load_batch([int(j) for j in order[i * bs:(i + 1) * bs]], device)
                    data = augmentation.augment_pair_batch(batch, aug_cfg, rng_aug, seed=step, hm_input=has_hm)
                    loss, components = train_step(model, data, loss_fn, optimizer, seed=step)
                    epoch_loss += loss
                    _add(epoch_components, components)
                    if log_every and (step + 1) % log_every == 0:
                        write('batch', step + 1, dict({'batch_loss': float(loss)}, **{'batch_loss/' + k: float(v) for k, v in components.items()}))

                val_loss, val_components, val_metrics = None, {}, None
                if val_dataset is not None and epoch % int(val.get('every_nth_epoch', 1)) == 0:
                    model.eval()
                    total = torch.zeros((), dtype=torch.float32, device=device)
                    n_val = (len(val_dataset) + bs - 1) // bs
                    with torch.no_grad():
                        for k in range(n_val):
                            batch = val_dataset.load_batch(list(range(k * bs, min((k + 1) * bs, len(val_dataset)))), device)
                            data = augmentation.augment_pair_batch(batch, aug_cfg, rng_aug, seed=k, hm_input=has_hm)
                            pred, pred2, pred_hm = model(data, seed=0)
                            loss_input = {'data': data, 'pred': pred, 'pred2': pred2}
                            if pred_hm is not None:
                                loss_input['pred_hm'] = pred_hm
                            loss, components = loss_fn(loss_input)
                            total += loss
                            _add(val_components, components)
                        if metric_ths is not None:
                            val_metrics = _validation_metrics(net, model, val_dataset, bs, device, config, metric_ths)
                    model.train()
                    val_loss = float(total) / n_val
                    val_components = {k: v / n_val for k, v in val_components.items()}

                mean_loss = float(epoch_loss) / steps_per_epoch          # the epoch's one read of the loss
                mean_components = {k: v / steps_per_epoch for k, v in epoch_components.items()}
                lr = float(optimizer.param_groups[0]['lr'])
                skipped = optimizer.last_step()['skipped_steps']
                scalars = dict({'loss': mean_loss, 'learning_rate': lr, 'skipped_steps': skipped}, **{'loss/' + k: v for k, v in mean_components.items()})
                if val_loss is not None:
                    scalars.update({'validation_loss': val_loss}, **{'validation_loss/' + k: v for k, v in val_components.items()})
                if val_metrics is not None:
                    for name in ('repeatability', 'nn_map', 'm_score', 'h_correctness'):
                        scalars.update({f'validation/{name}_{th}': v for th, v in val_metrics[name].items()})
                if metric_ths is not None:
                    history.setdefault('validation_metrics', []).append(val_metrics)
                write('epoch', epoch + 1, scalars)
                for k, v in (('epoch', epoch + 1), ('loss', mean_loss), ('components', mean_components), ('validation_loss', val_loss),
                             ('validation_components', val_components), ('learning_rate', lr), ('skipped_steps', skipped)):
                    history[k].append(v)
                print(f"epoch {epoch + 1}/{n_epochs}: loss {mean_loss:.6f}" + ("" if val_loss is None else f", validation loss {val_loss:.6f}") +
                      f", lr {lr:g}, skipped steps {skipped}")

                saving = save_every > 0 and (epoch + 1) % save_every == 0
                if saving:
                    save(f"e{epoch + 1}.model")
                if scheduler is not None:
                    scheduler.step()
                if saving:          # after the scheduler's step: the state the next epoch starts from
                    torch.save({'optimizer': optimizer.state_dict(), 'scheduler': None if scheduler is None else scheduler.state_dict(),
                                'epoch': epoch + 1}, os.path.join(out_dir, f"e{epoch + 1}.optim"))
            save('latest.model')
        finally:
            if writer is not None:
                writer.close()
    return history
