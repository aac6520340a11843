"""Training-pair augmentation on the GPU (reference xpoint/datasets/augmentation/augmentation.py, photometric_augmentation.py and
ImagePairDataset.__getitem__ :349-430), for whole batches: the batched device dict of `ImagePairDataset.load_batch` in, the batched
training dict of `XPointLoss.forward` and the homography head out.  The reference augments one sample at a time on the host with
OpenCV; here the scalars are drawn on the host and every pixel is touched by HIP kernels only (csrc/augment.hip).  No launch count
depends on the batch size.  There is no CPU fallback: a CPU tensor raises XPointHipError.

homographic_augmentation   cv2.warpPerspective (INTER_LINEAR, BORDER_REFLECT_101 or BORDER_CONSTANT) in the 1/32-pixel scheme of
                           csrc/warp.hip, compute_valid_mask by xp_ha_valid_mask itself, and the label map scattered through
                           warp_keypoints (f64, truncation toward zero) / filter_points / generate_keypoint_map.
photometric_augmentation   the six primitives of photometric_augmentation.py as a per-sample program: samples of one batch run
                           different orders in the same launches (1 prologue + 2 blur passes when additive_shade is among the
                           primitives + one launch per primitive: at most 9).
augment_pair_batch         __getitem__ :349-430 for a batch, with hm_input / hfour_points of prep_hm_regression_input.

Deliberate differences from the reference:
  * images are f32 throughout (the reference carries float64 until the final .astype(np.float32)); the tests bound the difference
    by the project's parity tolerance 1e-4;
  * additive_shade rasterises its ellipses by the analytic inside test of the rotated ellipse (in f64), cv2.ellipse fills a
    fixed-point polygon approximation: boundary pixels of the 0/1 mask can differ, ahead of a blur tens of pixels wide.  A half
    axis of 0 (images under 20 pixels) is widened to half a pixel.  The Gaussian blur uses getGaussianKernel's formula at every size
    (OpenCV substitutes fixed tables for sizes <= 7, which kernel_size_range [250, 350] never reaches);
  * the noise fields come from a counter-based generator in the kernel (Philox4x32-10, key = (seed, sample id, primitive), counter =
    pixel index; uniform = (x >> 8) * 2^-24, normal by Box-Muller), not from np.random: a sample's noise depends on (seed, sample id)
    only, never on its batch neighbours.  `sample_photometric_params` draws the reference's scalars from the reference's
    distributions in the reference's order, from a numpy Generator: no stream parity with the legacy np.random is claimed;
  * `labels_follow_warp=True` (default) labels the warped image with the WARPED points.  The reference's pair branch throws the warped
    points away (:407-415 label the warped image with the unwarped points); `labels_follow_warp=False` reproduces that."""
from __future__ import annotations

import ctypes
import random as _random

import numpy as np
import torch

from . import _lib
from ._lib import ptr
from . import homographies as _hom

PRIMITIVES = ['additive_gaussian_noise', 'additive_speckle_noise', 'random_brightness', 'random_contrast', 'additive_shade', 'motion_blur']
_OP = {name: i for i, name in enumerate(PRIMITIVES)}        # XP_AUG_* opcodes
_MOTION_MAX = 11                                            # the device's motion-kernel table holds 11 x 11


def _need_device(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise _lib.XPointHipError(f"{what} needs device tensors: xpoint_amd has no CPU fallback")


def homographic_augmentation(images, keypoint_maps, homographies, warp=None, border_reflect=True, valid_border_margin=0, mask_border=True):
    """The reference's homographic_augmentation for a batch, given the homographies.

    images (B, 1, h, w) f32 device; keypoint_maps (B, h, w) bool device or None; homographies (B, 3, 3) f64 (numpy or device), the
    forward maps as cv2.warpPerspective takes them; warp (B) bool (default: all True).  Returns (warped images, warped keypoint maps
    or None, valid_mask (B, 1, h, w) bool).  Per sample:
      image   cv2.warpPerspective(image, H, (w, h), INTER_LINEAR, BORDER_REFLECT_101 if border_reflect else BORDER_CONSTANT); with
              border_reflect=False bit-equal to utils.warp_perspective;
      mask    compute_valid_mask(shape, H, valid_border_margin * 2, mask_border), written by xp_ha_valid_mask;
      labels  every set pixel through warp_keypoints (f64 division, truncation toward zero: -0.9 -> 0 is kept), filter_points,
              generate_keypoint_map.
    A sample with warp[i] == False passes through untouched with an all-ones mask (the reference's dummy_valid_mask; an identity warp
    would lose its frame to mask_border).  Three launches (five with an erosion) for any B."""
    _need_device(images, "homographic_augmentation")
    if images.dim() != 4 or images.shape[1] != 1 or images.dtype != torch.float32:
        raise ValueError(f"homographic_augmentation: images must be (B, 1, h, w) float32, got {tuple(images.shape)} {images.dtype}")
    B, _, h, w = images.shape
    dev = images.device
    src = images.contiguous()
    Hd = _lib.matrix_table(homographies, B, dev, "homographic_augmentation")
    flags = None
    if warp is not None:
        flags = torch.as_tensor(warp).to(device=dev, dtype=torch.bool).reshape(-1).to(torch.uint8).contiguous()
        if flags.shape[0] != B:
            raise ValueError(f"homographic_augmentation: {flags.shape[0]} warp flags for {B} images")
    if keypoint_maps is not None:
        _need_device(keypoint_maps, "homographic_augmentation")
        if tuple(keypoint_maps.shape) != (B, h, w):
            raise ValueError(f"homographic_augmentation: keypoint maps must be {(B, h, w)}, got {tuple(keypoint_maps.shape)}")
    with torch.cuda.device(dev):
        st = _lib.current_stream(dev)
        r = int(valid_border_margin) * 2
        mask = torch.empty((B, 1, h, w), dtype=torch.uint8, device=dev)
        tmp = torch.empty_like(mask) if r > 0 else None
        _lib.call("xp_ha_valid_mask", ptr(Hd), ptr(mask), ptr(tmp), B, h, w, r, 1 if mask_border else 0, st)
        out = torch.empty_like(src)
        _lib.call("xp_aug_warp", ptr(src), ptr(out), ptr(Hd), ptr(flags), ptr(mask), B, h, w, 1 if border_reflect else 0, st)
        kp_out = None
        if keypoint_maps is not None:
            kin = keypoint_maps.to(torch.uint8).contiguous() if keypoint_maps.dtype != torch.uint8 else keypoint_maps.contiguous()
            kp8 = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
            _lib.call("xp_aug_scatter_labels", ptr(kin), ptr(kp8), ptr(Hd), ptr(flags), B, h, w, st)
            kp_out = kp8.view(torch.bool)
    return out, kp_out, mask.view(torch.bool)


# ------------------------------------------------------------------------------------------------ photometric: host side
def motion_blur_kernel(mode, ksize):
    """the reference's motion-blur kernel (photometric_augmentation.py:62-76), float64 ksize x ksize"""
    center = int((ksize - 1) / 2)
    kernel = np.zeros((ksize, ksize))
    if mode == 'h':
        kernel[center, :] = 1.
    elif mode == 'v':
        kernel[:, center] = 1.
    elif mode == 'diag_down':
        kernel = np.eye(ksize)
    elif mode == 'diag_up':
        kernel = np.flip(np.eye(ksize), 0)
    else:
        raise ValueError(f"motion_blur: unknown mode {mode!r}")
    var = ksize * ksize / 16.0
    grid = np.repeat(np.arange(ksize)[:, np.newaxis], ksize, axis=-1)
    gaussian = np.exp(-(np.square(grid - center) + np.square(grid.T - center)) / (2.0 * var))
    kernel = kernel * gaussian
    return kernel / np.sum(kernel)


def gaussian_kernel(ksize):
    """cv2.getGaussianKernel(ksize, 0): sigma = 0.3 ((ksize - 1) 0.5 - 1) + 0.8, normalised in double"""
    sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    k = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return k / k.sum()


def parse_primitives(names):
    p = PRIMITIVES if names == 'all' else (list(names) if isinstance(names, (list, tuple)) else [names])
    if not set(p) <= set(PRIMITIVES):
        raise ValueError(f"unknown photometric primitives {sorted(set(p) - set(PRIMITIVES))}")
    if len(set(p)) != len(p):
        raise ValueError("a photometric primitive may appear once")
    return p


def make_programs(ops, params, ellipses=None, shade_ksize=None, motion_kernels=None):
    """The per-sample program tables from explicit values (what `sample_photometric_params` fills by drawing): ops (B, S) opcodes =
    indices into PRIMITIVES, every row a permutation of one set; params (B, S) the scalar of each step (stddev, prob, delta, strength,
    transparency, motion ksize); ellipses (B, n, 5) rows (cx, cy, ax, ay, angle in degrees) and shade_ksize (B) odd, for additive_shade;
    motion_kernels: B float64 ksize x ksize arrays, for motion_blur."""
    ops = np.ascontiguousarray(ops, np.int32)
    B, S = ops.shape
    if any(sorted(row) != sorted(ops[0]) for row in ops.tolist()) or len(set(ops[0].tolist())) != S or ops.min() < 0 or ops.max() >= len(PRIMITIVES):
        raise ValueError("make_programs: every sample's order must be a permutation of the same primitives")
    prog = {'ops': ops, 'params': np.ascontiguousarray(params, np.float32).reshape(B, S)}
    if _OP['additive_shade'] in ops[0]:
        e = np.asarray(ellipses, np.float64).reshape(B, -1, 5)
        ang = np.deg2rad(e[..., 4])
        prog['ellipses'] = np.ascontiguousarray(np.stack([e[..., 0], e[..., 1], np.maximum(e[..., 2], 0.5), np.maximum(e[..., 3], 0.5),
                                                          np.cos(ang), np.sin(ang)], -1))
        ks = np.ascontiguousarray(shade_ksize, np.int32).reshape(B)
        if (ks < 1).any() or (ks % 2 == 0).any():
            raise ValueError("make_programs: additive_shade kernel sizes must be odd and positive")
        prog['shade_ksize'] = ks
        wts = np.zeros((B, int(ks.max())), np.float32)
        for i in range(B):
            wts[i, :ks[i]] = gaussian_kernel(int(ks[i]))
        prog['shade_weights'] = wts
    if _OP['motion_blur'] in ops[0]:
        mk = np.zeros((B, _MOTION_MAX * _MOTION_MAX), np.float32)
        for i in range(B):
            k = np.asarray(motion_kernels[i], np.float64)
            ks = k.shape[0]
            step = int(np.nonzero(ops[i] == _OP['motion_blur'])[0][0])
            if k.shape != (ks, ks) or ks % 2 == 0 or ks > _MOTION_MAX or int(prog['params'][i, step]) != ks:
                raise ValueError(f"make_programs: motion kernels are odd squares of at most {_MOTION_MAX}, with the size as the step's scalar")
            mk[i, :ks * ks] = k.reshape(-1)
        prog['motion_kernel'] = mk
    return prog


def sample_photometric_params(config, B, shape, rng):
    """Draw the reference's photometric scalars for B samples of `shape` = (h, w) on the host and emit the per-sample program tables
    (`make_programs`).  config = the reference's config['augmentation']['photometric'] ({'primitives', 'params', 'random_order'}).
    Per sample, in the reference's order and from the reference's distributions: the order of the primitives (random_order), then for
    every primitive AS IT RUNS its scalars: stddev / prob / delta / strength (uniform); per ellipse (rand ax, rand ay, integer x, integer
    y, rand angle), then transparency (uniform) and kernel_size (integer, made odd); the blur mode (one of four) and ksize.
    rng is a numpy.random.Generator.  The reference draws from the legacy global np.random (and the order from Python's random): the
    distributions and the order are the same, the streams are not, and no stream parity is claimed."""
    h, w = int(shape[0]), int(shape[1])
    prims = parse_primitives(config['primitives'])
    pcfg = [dict(config.get('params', {}).get(p, {})) for p in prims]
    S = len(prims)
    ops, params = np.zeros((B, S), np.int32), np.zeros((B, S), np.float32)
    nb = int(dict(zip(prims, pcfg)).get('additive_shade', {}).get('nb_ellipses', 20))
    ellipses, shade_ksize, motion = np.zeros((B, nb, 5)), np.ones(B, np.int32), [np.ones((1, 1))] * B
    for i in range(B):
        order = rng.permutation(S) if config.get('random_order', True) else np.arange(S)
        for s, idx in enumerate(order):
            name, c = prims[idx], pcfg[idx]
            ops[i, s] = _OP[name]
            if name == 'additive_gaussian_noise':
                params[i, s] = rng.uniform(*c.get('stddev_range', [0.0, 0.06]))
            elif name == 'additive_speckle_noise':
                params[i, s] = rng.uniform(*c.get('prob_range', [0.0, 0.005]))
            elif name == 'random_brightness':
                m = c.get('max_abs_change', 0.2)
                params[i, s] = rng.uniform(-m, m)
            elif name == 'random_contrast':
                params[i, s] = rng.uniform(*c.get('strength_range', [0.5, 1.5]))
            elif name == 'additive_shade':
                min_dim = min(h, w) / 4
                for e in range(nb):
                    ax = int(max(rng.random() * min_dim, min_dim / 5))
                    ay = int(max(rng.random() * min_dim, min_dim / 5))
                    max_rad = max(ax, ay)
                    x = int(rng.integers(max_rad, w - max_rad))
                    y = int(rng.integers(max_rad, h - max_rad))
                    ellipses[i, e] = (x, y, ax, ay, rng.random() * 90)
                params[i, s] = rng.uniform(*c.get('transparency_range', [-0.5, 0.8]))
                ks = int(rng.integers(*c.get('kernel_size_range', [250, 350])))
                shade_ksize[i] = ks + 1 if ks % 2 == 0 else ks
            else:
                mode = ['h', 'v', 'diag_down', 'diag_up'][int(rng.integers(0, 4))]
                ks = int(rng.integers(0, int((c.get('max_kernel_size', 10) + 1) / 2))) * 2 + 1
                if ks > _MOTION_MAX:
                    raise ValueError(f"motion_blur: max_kernel_size gives a kernel of {ks} > {_MOTION_MAX}")
                motion[i] = motion_blur_kernel(mode, ks)
                params[i, s] = ks
    return make_programs(ops, params, ellipses, shade_ksize, motion)


# ------------------------------------------------------------------------------------------------ photometric: device side
def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _field(fields, name, B, h, w, dev):
    if fields is None or fields.get(name) is None:
        return None
    f = fields[name]
    f = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32))
    f = f.to(device=dev, dtype=torch.float32).contiguous()
    if f.numel() != B * h * w:
        raise ValueError(f"photometric_augmentation: the {name} field must hold {(B, h, w)} elements")
    return f


def _sample_ids(sample_ids, B, dev):
    ids = torch.arange(B, dtype=torch.int32) if sample_ids is None else torch.as_tensor(sample_ids).to(torch.int64).reshape(-1).cpu()
    if ids.shape[0] != B or int(ids.min()) < 0 or int(ids.max()) >= 1 << 29:
        raise ValueError(f"photometric_augmentation: {B} sample ids in [0, 2^29) are needed")
    return ids.to(device=dev, dtype=torch.int32).contiguous()


def photometric_augmentation(images, programs, seed, sample_ids=None, fields=None):
    """Run every sample's program (`sample_photometric_params` / `make_programs`) on images (B, 1, h, w) f32 device; returns the
    augmented images.  seed (int, 64 bits) and sample_ids (B, default arange(B)) key the noise generator: sample i's noise is a function
    of (seed, sample_ids[i], primitive, pixel) alone.  fields = {'additive_gaussian_noise': standard-normal (B, h, w), 'additive_speckle_noise':
    uniform (B, h, w)} replaces the generated fields (parity tests).  Launches: 1 prologue (+ 2 blur passes with additive_shade) + one
    per primitive, whatever B and whatever the orders."""
    _need_device(images, "photometric_augmentation")
    if images.dim() != 4 or images.shape[1] != 1 or images.dtype != torch.float32:
        raise ValueError(f"photometric_augmentation: images must be (B, 1, h, w) float32, got {tuple(images.shape)} {images.dtype}")
    B, _, h, w = images.shape
    dev = images.device
    ops_h = np.asarray(programs['ops'])
    if ops_h.shape[0] != B:
        raise ValueError(f"photometric_augmentation: programs for {ops_h.shape[0]} samples, {B} images")
    S = ops_h.shape[1]
    has_shade, has_motion = 'ellipses' in programs, 'motion_kernel' in programs
    if (_OP['additive_shade'] in ops_h) != has_shade or (_OP['motion_blur'] in ops_h) != has_motion:
        raise ValueError("photometric_augmentation: the program tables do not match the opcodes (build them with make_programs)")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    with torch.cuda.device(dev):
        st = _lib.current_stream(dev)
        ids = _sample_ids(sample_ids, B, dev)
        ops, params = _dev(programs['ops'], dev), _dev(programs['params'], dev)
        nblk = _lib.load().xp_aug_partials_per_sample(h, w)
        if nblk <= 0:
            raise _lib.XPointHipError(f"photometric_augmentation: bad image size {h} x {w}")
        partials = torch.empty((2, B, nblk), dtype=torch.float64, device=dev)
        ping, pong = images.contiguous(), torch.empty_like(images)
        shade = motion = ell = None
        if has_shade:
            ell = _dev(programs['ellipses'], dev)
            shade, shade_tmp = torch.empty((B, h, w), dtype=torch.float32, device=dev), torch.empty((B, h, w), dtype=torch.float32, device=dev)
            wts, ksz = _dev(programs['shade_weights'], dev), _dev(programs['shade_ksize'], dev)
        if has_motion:
            motion = _dev(programs['motion_kernel'], dev)
        fg, fs = _field(fields, 'additive_gaussian_noise', B, h, w, dev), _field(fields, 'additive_speckle_noise', B, h, w, dev)
        _lib.call("xp_aug_photo_prologue", ptr(ping), ptr(partials[0]), ptr(ell), ptr(shade), ell.shape[1] if has_shade else 0, B, h, w, st)
        if has_shade:
            _lib.call("xp_aug_blur", ptr(shade), ptr(shade_tmp), ptr(wts), ptr(ksz), wts.shape[1], B, h, w, 0, st)
            _lib.call("xp_aug_blur", ptr(shade_tmp), ptr(shade), ptr(wts), ptr(ksz), wts.shape[1], B, h, w, 1, st)
        for s in range(S):
            _lib.call("xp_aug_photo_step", ptr(ping), ptr(pong), ptr(ops), ptr(params), s, S, ptr(partials[s & 1]), ptr(partials[(s + 1) & 1]),
                      ptr(shade), ptr(motion), ptr(fg), ptr(fs), ctypes.c_uint64(seed), ptr(ids), B, h, w, st)
            if s == 0:
                ping, pong = pong, torch.empty_like(images)          # the caller's images are never written
            else:
                ping, pong = pong, ping
    return ping


def random_field(seed, sample_ids, primitive, shape, kind, device="cuda:0"):
    """The generator on its own: (B, h, w) f32 fields, kind 'uniform' ((x >> 8) * 2^-24) or 'normal' (Box-Muller), keyed as
    photometric_augmentation keys the primitive's field.  primitive: a name of PRIMITIVES or an opcode."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.XPointHipError("random_field needs a GPU device: xpoint_amd has no CPU fallback")
    h, w = int(shape[0]), int(shape[1])
    B = len(sample_ids)
    op = _OP[primitive] if isinstance(primitive, str) else int(primitive)
    with torch.cuda.device(dev):
        ids = _sample_ids(sample_ids, B, dev)
        out = torch.empty((B, h, w), dtype=torch.float32, device=dev)
        _lib.call("xp_aug_random_field", ptr(out), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ptr(ids), op, {'uniform': 0, 'normal': 1}[kind],
                  B, h * w, _lib.current_stream(dev))
    return out


# ------------------------------------------------------------------------------------------------ batch assembly
def hm_regression_points(optical_H, thermal_H, h, w, patch=128):
    """prep_hm_regression_input's four-point target (ImagePairDataset.py:439-456) for one sample, host f64, with its quirks: the corner
    (h // 2 - 64, w // 2 - 64) is used as (x, y); the perturbed points are optical_H @ thermal_H @ p WITHOUT the projective division,
    truncated by int().  Returns ((4, 2) int64 differences, the crop's (y0, y1, x0, x1))."""
    tl = np.array([h // 2 - 64, w // 2 - 64])
    four = [tl, tl + [patch, 0], tl + [patch, patch], tl + [0, patch]]
    M = np.asarray(optical_H, np.float64).reshape(3, 3) @ np.asarray(thermal_H, np.float64).reshape(3, 3)
    pert = []
    for p in four:
        q = M @ np.array([[p[0]], [p[1]], [1]], np.float64)
        pert.append([int(q[0, 0]), int(q[1, 0])])
    xs, ys = [int(p[0]) for p in four], [int(p[1]) for p in four]
    return np.subtract(np.array(pert), np.array(four)).astype(np.int64), (min(ys), max(ys), min(xs), max(xs))


def augment_pair_batch(batch, config, rng, seed, labels_follow_warp=True, homographies=None, warp_optical=None, hm_input=True):
    """ImagePairDataset.__getitem__ :349-430 for the batched device dict `batch` of `ImagePairDataset.load_batch`; config = the
    reference's config['augmentation'] ({'photometric': {...}, 'homographic': {...}}).  Photometric runs on both images when enabled
    (one call over the 2B images; sample ids 0 .. B-1 optical, B .. 2B-1 thermal), then homographic: one coin per sample decides which
    image is warped (Python's `random`, as the reference; homographies by np.random / random as `sample_homography` /
    `sample_homography_corner` draw them).  rng: the numpy Generator of the photometric scalars; seed: the noise generator's.
    homographies (B, 3, 3) / warp_optical (B) bool override the draws.

    Returns {'optical': {'image' (B,1,h,w) f32, 'keypoints' (B,h,w) bool (when the batch has labels), 'valid_mask' (B,1,h,w) bool,
    'homography' (B,3,3) f32 (identity on the unwarped side), 'is_optical'}, 'thermal': {...}, 'name'} and, with homographic.enable,
    'hm_input' (B,2,128,128) f32 and 'hfour_points' (B,4,2) int64 (prep_hm_regression_input, quirks kept: see hm_regression_points).
    hm_input=False (a model without the homography head) leaves these two out, and with them the demand that the 128 x 128 crop fits.

    labels_follow_warp=True labels the warped image with the warped points (geometrically consistent); False reproduces the reference,
    whose pair branch discards the warped points and labels the warped image with the unwarped ones (:407-415)."""
    opt, th = batch['optical'], batch['thermal']
    _need_device(opt['image'], "augment_pair_batch")
    _need_device(th['image'], "augment_pair_batch")
    B, _, h, w = opt['image'].shape
    dev = opt['image'].device
    img_o, img_t = opt['image'], th['image']
    pcfg, hcfg = config.get('photometric', {}), config.get('homographic', {})
    if pcfg.get('enable', False):
        prog = sample_photometric_params(pcfg, 2 * B, (h, w), rng)
        both = photometric_augmentation(torch.cat([img_o, img_t], 0), prog, seed)
        img_o, img_t = both[:B], both[B:]
    out = {'optical': {}, 'thermal': {}}
    kp = {'optical': opt.get('keypoints'), 'thermal': th.get('keypoints')}
    if hcfg.get('enable', False):
        if hm_input and (h // 2 < 64 or w // 2 < 64 or h // 2 + 64 > w or w // 2 + 64 > h):      # the corner (h // 2 - 64, w // 2 - 64) is used as (x, y)
            raise ValueError(f"augment_pair_batch: the 128 x 128 homography-head crop does not fit a {h} x {w} image")
        params = hcfg.get('params', {})
        corner = params.get('corner_homography', {})
        pick = np.zeros(B, bool)
        Hs = np.zeros((B, 3, 3))
        for i in range(B):
            pick[i] = bool(_random.randint(0, 1)) if warp_optical is None else bool(warp_optical[i])
            if homographies is not None:
                Hs[i] = np.asarray(homographies[i], np.float64)
            elif corner.get('enable', False):
                Hs[i] = _hom.sample_homography_corner((h, w), corner['params'])
            else:
                Hs[i] = _hom.sample_homography((h, w), **{k: v for k, v in params.items() if k != 'corner_homography'})
        kw = dict(border_reflect=hcfg.get('border_reflect', True), valid_border_margin=hcfg.get('valid_border_margin', 0),
                  mask_border=hcfg.get('mask_border', True))
        # one batch of 2B: the optical images warp where the coin says so, the thermal ones where it does not
        flags = np.concatenate([pick, ~pick])
        kmaps = None if kp['optical'] is None or kp['thermal'] is None else torch.cat([kp['optical'], kp['thermal']], 0).to(torch.bool)
        img, kw_maps, mask = homographic_augmentation(torch.cat([img_o, img_t], 0), kmaps, np.concatenate([Hs, Hs]), warp=flags, **kw)
        img_o, img_t = img[:B], img[B:]
        eye = np.broadcast_to(np.eye(3, dtype=np.float32), (B, 3, 3))
        H32 = Hs.astype(np.float32)
        Ho, Ht = np.where(pick[:, None, None], H32, eye), np.where(pick[:, None, None], eye, H32)
        out['optical']['homography'], out['thermal']['homography'] = _dev(Ho, dev), _dev(Ht, dev)
        out['optical']['valid_mask'], out['thermal']['valid_mask'] = mask[:B], mask[B:]
        if kmaps is not None:
            maps = kw_maps if labels_follow_warp else kmaps
            out['optical']['keypoints'], out['thermal']['keypoints'] = maps[:B], maps[B:]
        if hm_input:
            pts = np.zeros((B, 4, 2), np.int64)
            for i in range(B):
                pts[i], (y0, y1, x0, x1) = hm_regression_points(Ho[i], Ht[i], h, w)
            out['hm_input'] = torch.cat([img_o[:, :, y0:y1, x0:x1], img_t[:, :, y0:y1, x0:x1]], 1).contiguous()
            out['hfour_points'] = _dev(pts, dev)
    else:
        for key, src in (('optical', opt), ('thermal', th)):
            out[key]['valid_mask'] = torch.ones((B, 1, h, w), dtype=torch.bool, device=dev)
            if kp[key] is not None:
                out[key]['keypoints'] = kp[key].to(torch.bool)
    out['optical']['image'], out['thermal']['image'] = img_o.contiguous(), img_t.contiguous()
    for key, src in (('optical', opt), ('thermal', th)):
        if 'is_optical' in src:
            out[key]['is_optical'] = src['is_optical']
    if 'name' in batch:
        out['name'] = batch['name']
    return out


def profile_launches(fn):
    """Run fn() with the library's per-launch event timing on (xp_prof_*) and return its rows {tag: (launches, ms, algorithmic bytes)};
    one row counts the calls of one entry point (tools/augment_bench.py, the launch-count tests)."""
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.xp_prof_reset(); lib.xp_prof_filter(None); lib.xp_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.xp_prof_enable(0)
    rows = {}
    name = ctypes.create_string_buffer(64)
    ms, cnt, fl, by = ctypes.c_double(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    for i in range(lib.xp_prof_count()):
        lib.xp_prof_get(i, name, 64, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by))
        rows[name.value.decode()] = (cnt.value, ms.value, by.value)
    lib.xp_prof_reset()
    return rows
