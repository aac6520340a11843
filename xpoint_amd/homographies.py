"""Homographic adaptation (reference xpoint/utils/homographies.py:40-300, 303-453) on the GPU: label export's pseudo ground truth.

The reference runs one homography at a time, one spectrum per forward.  Here the `num` views (view 0 = the original images, views
1 .. num-1 = the sampled homographies) go through the model in forwards of `chunk` views each (optical and thermal in one batch, per-image
`is_optical` flags), and everything around the forwards is HIP (csrc/homadapt.hip): the batched kornia-semantics warp into the forward's
input batch, the valid masks, the Gaussian filter, and one fused unwarp + aggregate + accumulate launch per chunk (the finalize folded
into the last).  The model is batch-invariant bit for bit, so `chunk` does not change a bit of the result.

Reproduced quirks of the reference (homographic_adaptation_multispectral):
  * desc_optical / desc_thermal are the descriptors of the LAST warped forward (of the original forward when num == 1);
  * the i = 0 term (the original images) goes in unmasked and `count` starts at 1;
  * prod takes sqrt after the division by count, sum multiplies by 0.5, window does neither;
  * min_count zeroes pixels with count < min_count (both outputs in window mode);
  * weighted_window=False turns every positive windowed value into 1;
  * filter_size > 0 is utils.get_gaussian_filter behind a reflection pad, applied to the forward output in the warped frame before the
    unwarp; it is rejected together with window;
  * images are warped with ('bilinear', 'reflection'), probabilities unwarped with 'bilinear' / zeros, the valid mask with 'nearest';
    kornia 0.1.4 normalises with (w - 1) while grid_sample samples with align_corners=False: the half-pixel inconsistency is kept.
  * homographic_adaptation (single spectrum) averages whatever the aggregation key says and checks neither aggregation nor window.
Deliberate differences:
  * the reference's loop calls net(input) with a single-image dict, which raises KeyError for a takes_pair=True model (XPoint.py:187;
    export_keypoints.py forces takes_pair=False for that reason).  Here the flow calls net.forward_raw with per-image is_optical flags,
    so both model kinds work;
  * the reference's dict_update writes the caller's keys INTO its module-level default config (later calls inherit them); here the
    defaults are copied first.
"""
from __future__ import annotations

import copy
from math import pi

import numpy as np
import torch

from . import _lib
from ._lib import ptr

homography_adaptation_default_config = {
    'num': 100,
    'aggregation': 'prod',
    'homographies': {
        'translation': True,
        'rotation': True,
        'scaling': True,
        'perspective': True,
        'scaling_amplitude': 0.15,
        'perspective_amplitude_x': 0.15,
        'perspective_amplitude_y': 0.15,
        'patch_ratio': 0.9,
        'max_angle': pi,
        'allow_artifacts': True,
    },
    'erosion_radius': 5,
    'mask_border': True,
    'min_count': 2,
    'filter_size': 0,
    'weighted_window': True,
}

_MODES = {'single': 0, 'prod': 1, 'sum': 2, 'window': 3}        # XP_HA_SINGLE / PROD / SUM / WINDOW


# ------------------------------------------------------------------------------------------------ homography sampling (host, numpy)
def get_perspective_transform(src, dst):
    """cv2.getPerspectiveTransform: the 3 x 3 map of four float32 points src -> dst, from the 8 x 8 linear system in float64
    (the products x * u of the last two columns are float32 products, as OpenCV forms them from Point2f)."""
    src = np.asarray(src, dtype=np.float32).reshape(4, 2)
    dst = np.asarray(dst, dtype=np.float32).reshape(4, 2)
    a = np.zeros((8, 8), dtype=np.float64)
    b = np.zeros(8, dtype=np.float64)
    for i in range(4):
        x, y = src[i]
        u, v = dst[i]
        a[i, 0] = a[i + 4, 3] = x
        a[i, 1] = a[i + 4, 4] = y
        a[i, 2] = a[i + 4, 5] = 1.0
        a[i, 6] = -(x * u); a[i, 7] = -(y * u)
        a[i + 4, 6] = -(x * v); a[i + 4, 7] = -(y * v)
        b[i] = u; b[i + 4] = v
    return np.append(np.linalg.solve(a, b), 1.0).reshape(3, 3)


def sample_homography(image_shape, perspective=True, scaling=True, rotation=True, translation=True, n_scales=10, n_angles=25,
                      scaling_amplitude=0.2, perspective_amplitude_x=0.1, perspective_amplitude_y=0.1, patch_ratio=0.8, max_angle=pi / 2,
                      allow_artifacts=True, translation_overflow=0.1, corner_homography={}):
    """A random homography (float64 3 x 3, the map of the image corners to a perturbed patch), with the reference's sequence of draws from
    the legacy global np.random generator: the order of the enabled transforms is shuffled BEFORE any transform draws, and the scale /
    angle transforms draw all n_scales / n_angles candidates before picking one."""
    def t_perspective(pts):
        t_min, t_max = -pts.min(axis=0), 1.0 - pts.max(axis=0)
        t_max[1] = min(abs(t_min[1]), abs(t_max[1]))
        t_min[1] = -t_max[1]
        amp = np.array([perspective_amplitude_x, perspective_amplitude_y])
        lo, hi = (-amp, amp) if allow_artifacts else (np.maximum(-amp, t_min), np.minimum(amp, t_max))
        dy = np.random.uniform(lo[1], hi[1])
        left = np.random.uniform(lo[0], hi[0])
        right = np.random.uniform(lo[0], hi[0])
        return pts + np.array([[left, dy], [left, -dy], [right, dy], [right, -dy]])

    def t_scale(pts):
        scales = np.random.uniform(-scaling_amplitude, scaling_amplitude, n_scales) + 1.0
        center = pts.mean(axis=0)
        scaled = (pts - center)[None] * scales[:, None, None] + center
        if allow_artifacts:
            valid = np.arange(n_scales)
        else:
            valid = [i for i in range(n_scales) if scaled[i].max() < 1.0 and scaled[i].min() >= 0.0]
        return scaled[np.random.choice(valid)]

    def t_translation(pts):
        t_min, t_max = -pts.min(axis=0), 1.0 - pts.max(axis=0)
        if allow_artifacts:
            t_min -= translation_overflow
            t_max += translation_overflow
        return pts + np.array([np.random.uniform(t_min[0], t_max[0]), np.random.uniform(t_min[1], t_max[1])])

    def t_rotation(pts):
        angles = np.append(np.random.uniform(-max_angle, max_angle, n_angles), 0)
        center = pts.mean(axis=0)
        rot = np.stack([np.cos(angles), -np.sin(angles), np.sin(angles), np.cos(angles)], axis=1).reshape(-1, 2, 2)
        rotated = np.matmul(np.tile((pts - center)[None], [n_angles + 1, 1, 1]), rot) + center
        if allow_artifacts:
            valid = np.arange(n_angles)
        else:
            valid = [i for i in range(len(angles)) if rotated[i].max() < 1.0 and rotated[i].min() >= 0.0]
        return rotated[np.random.choice(valid)]

    pts1 = np.array([[0., 0.], [0., 1.], [1., 1.], [1., 0.]])
    pts2 = (1 - patch_ratio) * 0.5 + patch_ratio * pts1
    functions = [f for f, on in ((t_perspective, perspective), (t_scale, scaling), (t_translation, translation), (t_rotation, rotation)) if on]
    order = np.arange(len(functions))
    np.random.shuffle(order)
    for i in order:
        pts2 = functions[i](pts2)
    shape = np.asarray(image_shape)[::-1]
    return get_perspective_transform((pts1 * shape).astype(np.float32), (pts2 * shape).astype(np.float32))


def sample_homography_corner(image_shape, config):
    """reference homographies.py:455-477 (the homography head's training pairs): a patch_size square at a random position at least rho
    from the border, its four corners perturbed by up to rho pixels each; returns the INVERSE of the map patch corners -> perturbed
    corners (float64 3 x 3).  The draws come from Python's `random` in the reference's order: position x, position y, then (dx, dy) of
    the top-left, top-right, bottom-right and bottom-left corner.  image_shape = (h, w); config = {'rho', 'patch_size'}."""
    import random
    imsize = image_shape[1], image_shape[0]
    rho, patch_size = int(config["rho"]), int(config["patch_size"])
    position_p = (random.randint(rho, imsize[0] - rho - patch_size), random.randint(rho, imsize[1] - rho - patch_size))
    four_points = [position_p, (patch_size + position_p[0], position_p[1]), (patch_size + position_p[0], patch_size + position_p[1]),
                   (position_p[0], patch_size + position_p[1])]
    perturbed = [(p[0] + random.randint(-rho, rho), p[1] + random.randint(-rho, rho)) for p in four_points]
    return np.linalg.inv(get_perspective_transform(np.float32(four_points), np.float32(perturbed)))


# ------------------------------------------------------------------------------------------------ kornia 0.1.4 matrix chain (host, f32)
def _normal_transform_pixel(h, w):
    n = torch.tensor([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0], [0.0, 0.0, 1.0]])
    n[0, 0] = n[0, 0] * 2.0 / (w - 1.0)
    n[1, 1] = n[1, 1] * 2.0 / (h - 1.0)
    return n.unsqueeze(0)


def sampling_matrix(M, h, w):
    """The normalised matrix kornia 0.1.4's warp_perspective_tensor(src, M, (h, w)) samples with (src and destination of one size):
    inverse(N * M * N^-1), N = normal_transform_pixel(h, w), in f32 on the CPU as the reference computes it.  M: (3, 3) f32 tensor."""
    n = _normal_transform_pixel(h, w)
    m_norm = torch.matmul(n, torch.matmul(M.reshape(1, 3, 3), torch.inverse(n)))
    return torch.inverse(m_norm)[0]


# ------------------------------------------------------------------------------------------------ the flow
def _config(cfg, multispectral):
    from .utils import dict_update          # (utils re-exports this module's names: imported here, not at module level)
    config = dict_update(copy.deepcopy(homography_adaptation_default_config), copy.deepcopy(cfg or {}))
    if config['num'] < 1:
        raise ValueError('num must be larger than 0 for the homographic adaptation')
    if config['filter_size'] % 2 == 0 and config['filter_size'] != 0:
        raise ValueError('The filter_size must be uneven')
    if multispectral:
        if config['aggregation'] == 'window' and config['filter_size'] > 0:
            raise ValueError('Window aggregation assumes keypoints in the binary heatmap! (Filter size must be 0 if window is set)')
        if config['aggregation'] not in ('prod', 'sum', 'window'):
            raise ValueError('Unknown aggregation: ' + config['aggregation'])
        if config['aggregation'] == 'window':
            assert config['window_size'] % 2 != 0          # search_window's assertion (a missing window_size is the reference's KeyError)
    return config


def _homographies(config, shape, homographies):
    num = config['num']
    if homographies is None:
        return [sample_homography(np.array(shape), **config['homographies']) for _ in range(num - 1)]
    hs = [np.asarray(h, dtype=np.float64).reshape(3, 3) for h in homographies]
    if len(hs) != num - 1:
        raise ValueError(f"homographies: expected num - 1 = {num - 1} matrices, got {len(hs)}")
    return hs


def _gaussian_weights(ks):
    """utils.get_gaussian_filter(ks).weight (reference utils.py:194-227) as a flat f32 tensor."""
    sigma = 0.3 * ((ks - 1) * 0.5 - 1) + 0.8
    xg = torch.arange(ks).repeat(ks).view(ks, ks)
    xy = torch.stack([xg, xg.t()], dim=-1)
    mean, var = (ks - 1) / 2., sigma ** 2.
    k = (1. / (2. * pi * var)) * torch.exp(-torch.sum((xy - mean) ** 2., dim=-1) / (2 * var))
    return (k / torch.sum(k)).float().reshape(-1)


def _flags(d, B):
    f = d.get('is_optical') if isinstance(d, dict) else None
    if f is None:
        return [True] * B
    f = torch.as_tensor(f).reshape(-1).cpu()
    if f.numel() == 1:
        f = f.repeat(B)
    return [bool(v) for v in f]


def _run(images, flags, net, config, mode, homographies, chunk):
    """images: list of S (B, 1, H, W) device tensors (optical, thermal or the single spectrum); flags: S lists of B bools."""
    dev = images[0].device
    if not images[0].is_cuda:
        raise RuntimeError("xpoint_amd homographic adaptation runs on the GPU only (no CPU fallback): move the data to 'cuda'")
    S = len(images)
    B, _, H, W = images[0].shape
    num = config['num']
    hs = _homographies(config, (H, W), homographies)
    chunk = max(1, min(num, int(chunk) if chunk else max(1, 32 // (S * B))))
    lib = _lib.load()
    st = _lib.current_stream(dev)
    src = torch.cat([im.reshape(B, H, W).float() for im in images]).contiguous()          # (S * B, H, W): one view's input images
    hs32 = [torch.from_numpy(h.astype(np.float32)) for h in hs]
    warp_m = torch.stack([sampling_matrix(h, H, W) for h in hs32]).to(dev) if hs else None
    unwarp_m = torch.stack([sampling_matrix(torch.inverse(h), H, W) for h in hs32]).to(dev) if hs else None
    masks = None
    if hs:
        masks = torch.empty((len(hs), H, W), dtype=torch.uint8, device=dev)
        tmp = torch.empty_like(masks) if config['erosion_radius'] > 0 else None
        Hd = _lib.matrix_table(np.stack(hs), len(hs), dev, "homographic_adaptation")
        _lib.check(lib.xp_ha_valid_mask(ptr(Hd), ptr(masks), ptr(tmp), len(hs), H, W,
                                        int(config['erosion_radius']), int(bool(config['mask_border'])), st), "xp_ha_valid_mask")
    fs = int(config['filter_size'])
    gw = _gaussian_weights(fs).to(dev) if fs > 0 else None
    acc0 = torch.empty((B, 1, H, W), device=dev)
    acc1 = torch.empty((B, 1, H, W), device=dev) if mode == _MODES['window'] else None
    count = torch.empty((B, 1, H, W), device=dev)
    view_flags = [f for fl in flags for f in fl]
    desc = None
    for v0 in range(0, num, chunk):
        nv = min(chunk, num - v0)
        last = v0 + nv == num
        batch = torch.empty((nv * S * B, 1, H, W), device=dev)
        first = 1 if v0 == 0 else 0
        if first:
            batch[:S * B, 0].copy_(src)
        if nv > first:
            j0 = v0 + first - 1                       # index of the chunk's first homography
            _lib.check(lib.xp_ha_warp(ptr(src), ptr(batch[first * S * B:]), ptr(warp_m[j0:]), S * B, (nv - first) * S * B, H, W, H, W,
                                      1, 1, st), "xp_ha_warp")
        raw = net.forward_raw(batch, want_prob=True, want_desc=last, is_optical=view_flags * nv)
        prob = raw.get("prob")
        if prob is None:
            raise RuntimeError("homographic adaptation needs the detector probabilities (force_return_logits must be off)")
        if gw is not None:
            filt = torch.empty_like(prob)
            _lib.check(lib.xp_ha_gaussian(ptr(prob), ptr(filt), ptr(gw), prob.shape[0], H, W, fs, st), "xp_ha_gaussian")
            prob = filt
        j0 = max(v0 - 1, 0)
        ns = nv - first
        _lib.check(lib.xp_ha_accumulate(ptr(prob), ptr(unwarp_m[j0:]) if ns else None, ptr(masks[j0:]) if ns else None, ptr(acc0), ptr(acc1),
                                        ptr(count), B, nv, first, H, W, mode, int(config.get('window_size', 1)),
                                        int(bool(config['weighted_window'])), int(last), float(config['min_count']), st), "xp_ha_accumulate")
        if last:
            d = raw["desc_nhwc"][(nv - 1) * S * B:]
            desc = [net._nchw(d[s * B:(s + 1) * B].contiguous()) for s in range(S)]
    return acc0, acc1, count, desc


def homographic_adaptation_multispectral(data, net, homographic_adaptation_config={}, homographies=None, chunk=None, return_count=False):
    """Reference homographies.py:40-200 (see the module docstring for the reproduced quirks).  data: the pair dict of the dataset
    ({'optical': {'image' (B,1,H,W), 'is_optical'}, 'thermal': {...}}) on the GPU.  Returns the reference's dict
    {'out': {'prob'}, 'out_optical': {'prob'}, 'out_thermal': {'prob'}, 'desc_optical', 'desc_thermal'}; `out` is None in window mode,
    out_optical / out_thermal are None otherwise.
    homographies: num - 1 float64 3 x 3 matrices used instead of sampling; chunk: views (original + homographies) per forward, default
    max(1, 32 // (2 B)); return_count: add the per-pixel count of valid views as out_dict['count']."""
    config = _config(homographic_adaptation_config, True)
    agg = config['aggregation']
    B = data['optical']['image'].shape[0]
    acc0, acc1, count, desc = _run([data['optical']['image'], data['thermal']['image']],
                                   [_flags(data['optical'], B), _flags(data['thermal'], B)], net, config, _MODES[agg], homographies, chunk)
    window = agg == 'window'
    out = {"out": {"prob": None if window else acc0}, "out_optical": {"prob": acc0 if window else None},
           "out_thermal": {"prob": acc1 if window else None}, "desc_optical": desc[0], "desc_thermal": desc[1]}
    if return_count:
        out["count"] = count
    return out


def homographic_adaptation(data, net, homographic_adaptation_config={}, homographies=None, chunk=None, return_count=False):
    """Reference homographies.py:232-300: the mean of the unwarped probabilities of one spectrum over the valid views.  data:
    {'image' (B,1,H,W), ['is_optical' (B,1)]} on the GPU.  Returns out (B,1,H,W), or (out, count) with return_count."""
    config = _config(homographic_adaptation_config, False)
    B = data['image'].shape[0]
    acc0, _, count, _ = _run([data['image']], [_flags(data, B)], net, config, _MODES['single'], homographies, chunk)
    return (acc0, count) if return_count else acc0
