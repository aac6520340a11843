"""Thin command-line front ends of the two prediction flows, the label export, the training run and the synthetic-shapes generator, with the reference scripts' arguments
(predict_align_image_pair.py:24-37, predict_keypoints.py: the same -y / -m / -v / -i / -s options; train.py: -y / -w):

    python -m xpoint_amd.cli align     -y configs/cipdp.yaml -m model_weights/XPoint-EXP1 -v latest [-i 0] [-n 1] [-s 0] [-e] [-o out.npz]
    python -m xpoint_amd.cli keypoints -y configs/cipdp.yaml -m model_weights/XPoint-EXP1 -v latest [-i 0] [-n 1] [-s 0] [-e [-t 3]] [-o out.npz]
    python -m xpoint_amd.cli export    -y configs/config_export_keypoints.yaml -m model_weights/XPoint-EXP1 -v latest -o labels.npz
                                       [-i 0] [-n all] [-s 0] [--chunk K]
    python -m xpoint_amd.cli train     -y configs/cmt.yaml [-w <output_directory>/e20.model] [-s 0]
    python -m xpoint_amd.cli benchmark -y configs/cipdp.yaml -m model_weights/XPoint-EXP1 -v latest [-s 0] [-o out.json]
    python -m xpoint_amd.cli synth     -y configs/config_synthetic_shapes.yaml -n 16 -o shapes.npz [-i 0] [-s 0] [--textured-polygons]

`synth` is show_synthetic_images.py without the plots: samples -i .. -i + n - 1 of the SyntheticShapes dataset of the YAML's `dataset:` block
(xpoint_amd.synthetic_shapes: rendered on the GPU, then augmented as the block says), written to -o as image (n, 1, h, w) f32, keypoints
(n, h, w) bool, valid_mask (n, 1, h, w) bool and is_optical (n, 1) bool.  Sample i depends on (-s, i) alone.  -m, -v are not used.
--textured-polygons sets the block's `textured_polygons: true`: draw_multiple_polygons is accepted and `primitives: 'all'` means all nine.

`benchmark` is the -e half of benchmark.py:175-249 (see `benchmark`): repeatability, NN-mAP, M-score and homography correctness over the WHOLE
folder dataset in batches of prediction.batchsize (evaluation.compute_metrics_batched), with the script's threshold lists (1..10 for the
repeatability, keypoint and warp thresholds, [2] for RANSAC) and prediction.detection_threshold; it prints the script's result lines and, with
-o, writes the JSON the script writes.  The script's timing experiment and plots are not part of it; -i and -n are not used.

`train` is train.py (xpoint_amd.training.fit, whose docstring lists what is kept and what differs): the VMamba XPoint on pairs of a folder dataset
with keypoint labels, Adam with weight decay and a device-side guard against non-finite gradients, the LR schedule, validation, `params.yaml`,
`e<N>.model` / `latest.model` (and `e<N>.optim`, from which -w e<N>.model resumes the optimiser) in training.output_directory.  It reads everything
from the YAML; -m, -v, -i, -n are not used.

What is kept from the scripts: the YAML handling (model params from <model-dir>/params.yaml overwrite config['model'], the
`use_attention` height / width patch of predict_align_image_pair.py:50-54), `<model-dir>/<version>.model` loaded with
`strict=False` after `fix_model_weigth_keys`, the seeds, the per-sample flow.  What is not: plotting (-p, -r) and the HDF5
datasets — the dataset must be a folder dataset (`dataset.foldername`, xpoint_amd/datasets.py).  `align -e` adds the registration
step (robust homography per pair) and prints the inlier counts.  Prints one line per sample and a timing summary.

`keypoints -e [-t 3]` is the evaluation half of predict_keypoints.py:88-142 (see `evaluate_keypoints`): the repeatability of the detector
over the WHOLE dataset in batches of prediction.batchsize, printed in the script's three lines and, with -o, stored as repeatability_mean,
repeatability, n_kp_optical, n_kp_thermal and distance_threshold next to the per-sample keypoints.  When the dataset carries keypoint labels
(dataset.keypoints_filename: an .npz as `export` writes it) it additionally reports mAP and the mean prediction-label distance per spectrum.

`export` is export_keypoints.py: label export by homographic adaptation (xpoint_amd.homographies, config key
prediction.homographic_adaptation) with the model params of <model-dir>/params.yaml, takes_pair and the homography head off, seeds as
in the script, box_nms with prediction.nms / detection_threshold / topk, keypoints = nonzero(prob > detection_threshold).  The output
is an .npz with the keys <name>/keypoints, or <name>/keypoints_optical and <name>/keypoints_thermal for the window aggregation.  Not
supported: HDF5 output, the HDF5 datasets, -skip and the -f backup files (h5py is not available); the dataset must be a folder dataset.
--chunk sets the homographies per forward (default: the library's); it does not change the result."""
from __future__ import annotations

import argparse
import os
import random
import time

import numpy as np
import torch
import yaml


def load_config(yaml_config: str, model_dir: str) -> dict:
    with open(yaml_config, 'r') as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    with open(os.path.join(model_dir, 'params.yaml'), 'r') as f:
        config['model'] = yaml.load(f, Loader=yaml.FullLoader)['model']          # overwrite the model params
    ua = config['model'].get('use_attention')
    if ua and ua.get('check'):                                                    # predict_align_image_pair.py:50-54
        ph, pw = ua['height'], ua['width']
        ua.setdefault('model_parameters', {}).setdefault('DATA', {})['IMG_SIZE'] = (ph, pw)
        ua['height'] = config['dataset']['height']
        ua['width'] = config['dataset']['width']
    return config


def build(config: dict, model_dir: str, version: str, device: str):
    from . import datasets
    ds_cfg = dict(config['dataset'])
    ds_cfg.pop('type', None)
    ds_cfg['single_image'] = False
    dataset = datasets.ImagePairDataset(ds_cfg)
    return dataset, build_net(config, model_dir, version, device)


def build_net(config: dict, model_dir: str, version: str, device: str):
    from . import models, utils
    net = getattr(models, config['model']['type'])(config['model'])
    if version != 'none':
        weights = torch.load(os.path.join(model_dir, version + '.model'), map_location=torch.device('cpu'))
        weights = utils.fix_model_weigth_keys(weights)
        missing, unexpected = net.load_state_dict(weights, strict=False)
        loaded = set(weights.keys()) - set(missing)
        print(f"Successfully loaded {len(loaded)} keys.\nMissing keys: {len(missing)}\nUnexpected keys: {len(unexpected)}")
        if len(loaded) < 1:
            raise ValueError("No weights were loaded correctly! Please check the model and weights file.")
    net.to(device)
    net.eval()
    return net


def evaluate_keypoints(args, config, dataset, net) -> dict:
    """predict_keypoints.py:88-142 for a pair dataset: seeds as the script, compute_repeatability_multispectral over the whole dataset in
    batches of prediction.batchsize, the script's three printed lines; returns repeatability_mean, repeatability, n_kp_optical,
    n_kp_thermal, distance_threshold.

    Extension: when the dataset carries keypoint labels, compute_detector_metrics runs once per spectrum on the same crops (the seeds are set
    again before every pass) and detector_<spectrum>_{precision, recall, prob, dist, mAP, mean_dist} are added.  The reference offers these
    numbers only for single-image HDF5 datasets (its `else` branch); here they come from the pair dataset's per-spectrum labels, through a
    single-image forward — the model built with takes_pair and the homography head off, as `export` builds it."""
    import copy
    from . import evaluation
    pred = config['prediction']
    bs = int(pred.get('batchsize', 1))

    def seed():
        random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)

    def loader(spec=None):
        for i0 in range(0, len(dataset), bs):
            batch = dataset.load_batch(list(range(i0, min(i0 + bs, len(dataset)))), args.device)
            yield batch if spec is None else dict(batch[spec])

    seed()
    mean, rep, n_o, n_t = evaluation.compute_repeatability_multispectral(net, loader(), args.device, config, distance_thresh=args.threshold)
    print('Repeatability: {}'.format(mean))
    print('Number of optical keypoints: {}'.format(np.mean(n_o)))
    print('Number of thermal keypoints: {}'.format(np.mean(n_t)))
    res = {'repeatability_mean': mean, 'repeatability': np.asarray(rep, np.float64), 'n_kp_optical': np.asarray(n_o, np.int64),
           'n_kp_thermal': np.asarray(n_t, np.int64), 'distance_threshold': args.threshold}
    if dataset.config['keypoints_filename'] is not None:
        net1 = net
        if net.takes_pair():
            cfg1 = copy.deepcopy(config)
            cfg1['model']['takes_pair'] = False
            if 'homography_regression_head' in cfg1['model']:
                cfg1['model']['homography_regression_head']['check'] = False
            net1 = build_net(cfg1, args.model_dir, args.version, args.device)
        for spec in ('optical', 'thermal'):
            seed()
            precision, recall, prob, dist = evaluation.compute_detector_metrics(net1, loader(spec), args.device, pred)
            m_ap = float(evaluation.compute_mAP(precision, recall))
            mean_dist = float(dist.mean()) if len(dist) else float('nan')
            print('{}: mAP: {}'.format(spec, m_ap))
            print('{}: Average distance of the predictions to the labels within the radius: {}'.format(spec, mean_dist))
            res.update({f'detector_{spec}_precision': precision, f'detector_{spec}_recall': recall, f'detector_{spec}_prob': prob,
                        f'detector_{spec}_dist': dist, f'detector_{spec}_mAP': m_ap, f'detector_{spec}_mean_dist': mean_dist})
    return res


BENCHMARK_THRESHOLDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]      # benchmark.py:133-135: repeatability, keypoint distance and warp error
BENCHMARK_RANSAC_THRESHOLDS = [2]                           # benchmark.py:136


def _jsonable(x):
    """Plain Python for json.dumps: numpy scalars and arrays become numbers and lists, dictionary keys become strings (as json.dumps does)."""
    if isinstance(x, dict):
        return {str(k): _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    return x


def benchmark_results(out, config, model_dir, version, detection_threshold) -> dict:
    """The dictionary benchmark.py:214-237 writes for one detection threshold, from compute_metrics' return: `repeatability`, `descriptor`
    ({'th_kp_<th>': {'nn_map', 'm_score'}}), `homography` and the bookkeeping keys (without the timing experiment's entries)."""
    ds = config['dataset']
    res = {'repeatability': out['repeatability'],
           'descriptor': {'th_kp_{}'.format(th): {k: out['descriptor'][th][k] for k in ('nn_map', 'm_score') if k in out['descriptor'][th]}
                          for th in out['descriptor']},
           'homography': out['homography'],
           'model_dir': model_dir, 'model_version': version, 'height-width': '{},{}'.format(ds['height'], ds['width']),
           'dataset': ds['filename'] if ds.get('filename') else ds['foldername'],
           'nms': config['prediction']['nms'], 'detection_th': detection_threshold,
           'threshold_keypoints_for_descriptor': list(BENCHMARK_THRESHOLDS), 'threshold_homography_epsilon': list(BENCHMARK_THRESHOLDS),
           'threshold_repeatability_distance_th': list(BENCHMARK_THRESHOLDS), 'ransac_reproj_thresholds': list(BENCHMARK_RANSAC_THRESHOLDS)}
    return _jsonable(res)


def benchmark(args):
    """The -e half of benchmark.py:175-249: evaluation.compute_metrics_batched over the whole folder dataset in batches of
    prediction.batchsize with the script's threshold lists, its printed result lines, and with -o its JSON (benchmark_results).  The timing
    experiment and the plots of the script are not part of this; HDF5 datasets are not supported."""
    import json
    from . import evaluation, predict
    random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)
    config = load_config(args.yaml_config, args.model_dir)
    if config['dataset'].get('filename') is not None or config['dataset'].get('foldername') is None:
        raise SystemExit("benchmark: only folder datasets are supported (dataset.foldername)")
    try:                                                                         # benchmark.py:57-60
        config['model']['homography_regression_head']['check'] = not bool(config['prediction']['disable_hmhead'])
    except (KeyError, TypeError):
        pass
    config['prediction'] = predict._cfg(config.get('prediction'))
    if not torch.cuda.is_available():
        raise SystemExit("xpoint_amd runs on the GPU only (no CPU fallback)")
    print('Predicting on device: {}'.format(args.device))
    dataset, net = build(config, args.model_dir, args.version, args.device)
    pred = config['prediction']
    bs = int(pred.get('batchsize', 1))
    detection_threshold = pred['detection_threshold']
    print("MODEL : ", args.model_dir)
    print("Keypoint detection threshold : ", [detection_threshold])

    def loader():
        for i0 in range(0, len(dataset), bs):
            yield dataset.load_batch(list(range(i0, min(i0 + bs, len(dataset)))), args.device)

    t0 = time.perf_counter()
    with torch.no_grad():
        out = evaluation.compute_metrics_batched(net, loader(), args.device, config, detection_threshold,
                                                 thresh_repeatability=list(BENCHMARK_THRESHOLDS), thresh_keypoints=list(BENCHMARK_THRESHOLDS),
                                                 thresh_warp=list(BENCHMARK_THRESHOLDS), ransac_reproj_thresholds=list(BENCHMARK_RANSAC_THRESHOLDS))
    dt = time.perf_counter() - t0
    print("-----------repeatability Results:--------------")
    rep = out["repeatability"]
    print('Repeatability: {}'.format(rep['repeatability_mean']))
    print('Number of optical keypoints: {}'.format(rep['n_kp_optical']))
    print('Number of thermal keypoints: {}'.format(rep['n_kp_thermal']))
    print("-------Descriptor Results:-------------")
    for key in out["descriptor"]:
        print('th kp : {}, NN-mAP: {}'.format(key, out["descriptor"][key]['nn_map']))
        print('th kp : {}, M-Score: {}'.format(key, out["descriptor"][key]['m_score']))
    print("-------Homography correctness Results:-------------")
    for th in out["homography"]:
        print('th ransac reprojection : {}, Homography correctness: {}'.format(th, out["homography"][th]['h_correctness']))
    print(f"benchmark: {len(dataset)} pair(s), {dt * 1e3:.1f} ms")
    res = benchmark_results(out, config, args.model_dir, args.version, detection_threshold)
    if args.output:
        d = os.path.dirname(args.output)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.output, 'w') as fh:
            fh.write(json.dumps(res, indent=4))
        print("-----done : ", args.output, "\n")
    return res


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m xpoint_amd.cli", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('flow', choices=['align', 'keypoints', 'export', 'train', 'benchmark', 'synth'])
    ap.add_argument('-y', '--yaml-config', default='configs/cipdp.yaml', help='YAML config file')
    ap.add_argument('-m', '--model-dir', default='model_weights/xpoint', help='Directory of the model')
    ap.add_argument('-v', '--version', default='latest', help='Model version (name of the param file), none for no weights')
    ap.add_argument('-i', '--index', default=0, type=int, help='Index of the first sample')
    ap.add_argument('-n', '--count', default=None, type=int, help='Number of consecutive samples (default 1; export: all)')
    ap.add_argument('-e', dest='evaluation', action='store_true',
                    help='align: also estimate the homography of every pair and warp the optical image with it; keypoints: compute the repeatability '
                         'over the whole dataset (and, if the dataset has keypoint labels, mAP and the mean label distance per spectrum)')
    ap.add_argument('-t', dest='threshold', default=3, type=int, help='keypoints -e: distance threshold for two keypoints to be considered a match')
    ap.add_argument('--save-warped', default=None, metavar='DIR', help='align -e: write the warped optical image of every sample to DIR/<name>_warped.png')
    ap.add_argument('-s', '--seed', default=0, type=int, help='Seed of the random generators')
    ap.add_argument('-o', '--output', default=None, help='write keypoints / matches of the samples to this .npz (benchmark: the result JSON; synth: the samples)')
    ap.add_argument('--chunk', default=None, type=int, help='export: homographies per forward (does not change the result)')
    ap.add_argument('-w', '--weight-file', default=None, help='train: file containing the weights to initialize the weights (e<N>.model resumes at epoch N)')
    ap.add_argument('--textured-polygons', action='store_true', help="synth: set the dataset's textured_polygons key (draw_multiple_polygons; 'all' = the nine primitives)")
    ap.add_argument('--device', default='cuda:0')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.flow == 'export':
        return export(args)
    if args.flow == 'benchmark':
        return benchmark(args)
    if args.flow == 'train':
        return train(args)
    if args.flow == 'synth':
        return synth_shapes(args)
    if args.count is None:
        args.count = 1

    random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)
    config = load_config(args.yaml_config, args.model_dir)
    if not torch.cuda.is_available():
        raise SystemExit("xpoint_amd runs on the GPU only (no CPU fallback)")
    print('Predicting on device: {}'.format(args.device))
    dataset, net = build(config, args.model_dir, args.version, args.device)
    from . import predict
    pred_cfg = {k: v for k, v in config.get('prediction', {}).items() if k in predict.DEFAULT_PREDICTION or k == 'reprojection_threshold'}
    out = {}
    t_total = 0.0
    with torch.no_grad():
        if args.flow == 'keypoints' and args.evaluation:
            out.update(evaluate_keypoints(args, config, dataset, net))
        for idx in range(args.index, min(args.index + args.count, len(dataset))):
            data = dataset.load_batch([idx], args.device)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            if args.flow == 'align':
                _, _, res = predict.predict_align_image_pair(net, data, pred_cfg, estimate_homography=args.evaluation)
            else:
                ko, kt = predict.predict_keypoints(net, data, pred_cfg)
                res = [dict(kp_optical=ko[0], kp_thermal=kt[0])]
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            t_total += dt
            r = res[0]
            name = data.get('name', [str(idx)])[0]
            line = f"{name}: {len(r['kp_optical'])} / {len(r['kp_thermal'])} keypoints"
            if 'matches' in r:
                line += f", {len(r['matches'])} matches"
            if 'matchesMask' in r:
                line += f", {int(np.sum(r['matchesMask']))} inliers"
            print(line + f"  ({dt * 1e3:.1f} ms)")
            out[f"{idx}/kp_optical"] = r['kp_optical'].cpu().numpy(); out[f"{idx}/kp_thermal"] = r['kp_thermal'].cpu().numpy()
            if 'matches' in r:
                out[f"{idx}/matches"] = np.array([(m.queryIdx, m.trainIdx) for m in r['matches']], dtype=np.int64).reshape(-1, 2)
            if 'H_est' in r:
                out[f"{idx}/H_est"] = np.asarray(r['H_est'])
            if 'warped_optical' in r:
                out[f"{idx}/warped_optical"] = r['warped_optical'].cpu().numpy()
                if args.save_warped:
                    import os
                    from PIL import Image
                    os.makedirs(args.save_warped, exist_ok=True)
                    Image.fromarray(out[f"{idx}/warped_optical"]).save(os.path.join(args.save_warped, f"{name}_warped.png"))
    print(f"{args.flow}: {sum(1 for k in out if k.endswith('/kp_optical'))} sample(s), {t_total * 1e3:.1f} ms")
    if args.output:
        np.savez(args.output, **out)
    return out


def train(args):
    """train.py (see the module docstring): xpoint_amd.training.fit on the YAML config."""
    with open(args.yaml_config, 'r') as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    if not torch.cuda.is_available():
        raise SystemExit("xpoint_amd runs on the GPU only (no CPU fallback)")
    from . import training
    return training.fit(config, weight_file=args.weight_file, device=args.device, seed=args.seed)


def synth_shapes(args):
    """show_synthetic_images.py without the plots (see the module docstring)."""
    if not args.output:
        raise SystemExit("synth: -o/--output (.npz) is required")
    with open(args.yaml_config, 'r') as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    ds = dict(config.get('dataset', {}))
    if ds.get('type', 'SyntheticShapes') != 'SyntheticShapes':
        raise SystemExit(f"synth: dataset.type must be 'SyntheticShapes', got {ds.get('type')!r}")
    ds.pop('type', None)
    if args.textured_polygons:
        ds['textured_polygons'] = True
    if not torch.cuda.is_available():
        raise SystemExit("xpoint_amd runs on the GPU only (no CPU fallback)")
    from . import synthetic_shapes
    dataset = synthetic_shapes.SyntheticShapes(ds)
    n = 1 if args.count is None else args.count
    bs = int(config.get('training', {}).get('batchsize', 32))
    parts = []
    t0 = time.perf_counter()
    for i0 in range(args.index, args.index + n, bs):
        parts.append(dataset.load_batch(list(range(i0, min(i0 + bs, args.index + n))), args.device, seed=args.seed))
    torch.cuda.synchronize()
    out = {k: torch.cat([p[k] for p in parts]).cpu().numpy() for k in ('image', 'keypoints', 'valid_mask', 'is_optical')}
    print(f"synth: {n} sample(s) of {tuple(out['image'].shape[2:])}, {int(out['keypoints'].sum())} keypoints, {(time.perf_counter() - t0) * 1e3:.1f} ms")
    d = os.path.dirname(args.output)
    if d:
        os.makedirs(d, exist_ok=True)
    np.savez(args.output, **out)
    return out


def export(args):
    """export_keypoints.py (see the module docstring)."""
    if not args.output:
        raise SystemExit("export: -o/--output (.npz) is required")
    with open(args.yaml_config, 'r') as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    with open(os.path.join(args.model_dir, 'params.yaml'), 'r') as f:
        config['model'] = yaml.load(f, Loader=yaml.FullLoader)['model']          # overwrite the model params
    ds = config.get('dataset', {})
    if ds.get('filename') is not None or ds.get('foldername') is None:
        raise SystemExit("export: only folder datasets are supported (dataset.foldername); HDF5 datasets (dataset.filename) need h5py, "
                         "which is not available")
    config['model']['takes_pair'] = False                                         # export_keypoints.py
    if 'homography_regression_head' in config['model']:
        config['model']['homography_regression_head']['check'] = False
        if 'disable_hmhead' in config['prediction']:
            config['model']['homography_regression_head']['check'] = not bool(config['prediction']['disable_hmhead'])
    torch.manual_seed(args.seed); random.seed(args.seed); np.random.seed(args.seed)
    if not torch.cuda.is_available():
        raise SystemExit("xpoint_amd runs on the GPU only (no CPU fallback)")
    from . import utils
    dataset, net = build(config, args.model_dir, args.version, args.device)
    pred = config['prediction']
    ha_cfg = pred['homographic_adaptation']
    window = ha_cfg.get('aggregation', 'prod') == 'window'
    bs = int(pred.get('batchsize', 1))
    last = len(dataset) if args.count is None else min(args.index + args.count, len(dataset))
    out = {}
    t0 = time.perf_counter()
    with torch.no_grad():
        for i0 in range(args.index, last, bs):
            batch = dataset.load_batch(list(range(i0, min(i0 + bs, last))), args.device)
            r = utils.homographic_adaptation_multispectral(batch, net, ha_cfg, chunk=args.chunk)
            probs = {'optical': r['out_optical']['prob'], 'thermal': r['out_thermal']['prob']} if window else {'': r['out']['prob']}
            if pred['nms'] > 0:
                probs = {k: utils.box_nms(v, pred['nms'], pred['detection_threshold'], keep_top_k=pred['topk'], on_cpu=pred.get('cpu_nms', False))
                         for k, v in probs.items()}
            for b, name in enumerate(batch['name']):
                counts = []
                for k, v in probs.items():
                    kp = torch.nonzero(v[b].squeeze() > pred['detection_threshold']).cpu().numpy()
                    out[f"{name}/keypoints" + (f"_{k}" if k else "")] = kp
                    counts.append(len(kp))
                print(f"{name}: {' / '.join(map(str, counts))} keypoints")
    torch.cuda.synchronize()
    print(f"export: {len(out) // len(probs) if out else 0} sample(s), {(time.perf_counter() - t0) * 1e3:.1f} ms")
    d = os.path.dirname(args.output)
    if d:
        os.makedirs(d, exist_ok=True)
    np.savez(args.output, **out)
    return out


if __name__ == "__main__":
    main()
