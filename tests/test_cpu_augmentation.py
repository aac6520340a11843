"""CPU: the numpy restatement of the training-pair augmentation (tests/augmentation_f64.py) against the REAL reference
(tests/golden/g29_augmentation.npz, tools/make_golden_augmentation.py) and against scipy where it imports; the host side of
xpoint_amd/augmentation.py (scalar sampling, corner homographies); the C ABI's declarations; the refusal of CPU tensors."""
import os
import random

import numpy as np
import pytest
import torch

from tests import augmentation_f64 as A
from xpoint_amd import _lib, augmentation as aug, homographies as hom

G29 = "g29_augmentation.npz"
SYMBOLS = ["xp_aug_warp", "xp_aug_scatter_labels", "xp_aug_random_field", "xp_aug_photo_prologue", "xp_aug_blur", "xp_aug_photo_step",
           "xp_aug_partials_per_sample"]
LABEL_CASES = ["sampled0", "sampled1", "sampled2", "empty", "collision", "minus_one_to_zero", "lands_on_h", "one_pixel_wide"]
PHOTO_CONFIG = {
    'enable': True, 'random_order': True,
    'primitives': ['random_brightness', 'random_contrast', 'additive_speckle_noise', 'additive_gaussian_noise', 'additive_shade', 'motion_blur'],
    'params': {'random_brightness': {'max_abs_change': 0.15}, 'random_contrast': {'strength_range': [0.3, 1.8]},
               'additive_gaussian_noise': {'stddev_range': [0, 0.06]}, 'additive_speckle_noise': {'prob_range': [0, 0.0035]},
               'additive_shade': {'transparency_range': [-0.5, 0.8], 'kernel_size_range': [9, 15], 'nb_ellipses': 6},
               'motion_blur': {'max_kernel_size': 10}}}


def test_restated_primitives_equal_the_reference(golden):
    """the four numpy-only primitives: the f64 restatement, fed the scalar and the field the reference drew, gives the reference's bits"""
    g = golden(G29)
    fns = {'additive_gaussian_noise': A.additive_gaussian_noise, 'additive_speckle_noise': A.additive_speckle_noise}
    for name in ('additive_gaussian_noise', 'additive_speckle_noise', 'random_brightness', 'random_contrast'):
        x, s, f, want = g[f"photo/{name}/input"], float(g[f"photo/{name}/scalar"]), g[f"photo/{name}/field"], g[f"photo/{name}/output"]
        assert x.dtype == np.float32 and want.dtype == np.float64 and x.shape == (48, 64)
        if name in fns:
            got = fns[name](x, s, f)
        else:
            got = A.random_brightness(x, s) if name == 'random_brightness' else A.random_contrast(x, s)
        assert np.array_equal(got, want), name
        assert not np.array_equal(want, x.astype(np.float64)), name          # the primitive did something
    # the speckle positions survive the f32 cast of field and prob (asserted by the tool with a 1e-6 gap)
    s, f = float(g["photo/additive_speckle_noise/scalar"]), g["photo/additive_speckle_noise/field"]
    lo64, hi64 = A.speckle_positions(s, f)
    lo32, hi32 = A.speckle_positions(np.float32(s), f.astype(np.float32))
    assert np.array_equal(lo64, lo32) and np.array_equal(hi64, hi32) and lo64.sum() > 0 and hi64.sum() > 0


@pytest.mark.parametrize("case", LABEL_CASES)
def test_restated_label_warp_equals_the_reference(golden, case):
    g = golden(G29)
    m, Hm, want = g[f"labels/{case}/map"], g[f"labels/{case}/H"], g[f"labels/{case}/out"]
    got = A.warp_label_map(m, Hm)
    assert got.dtype == bool and got.shape == m.shape and np.array_equal(got, want)
    if case.startswith("sampled"):
        exact = A.warp_keypoints_exact(np.stack(np.nonzero(m), 1), Hm)
        assert np.abs(exact - np.rint(exact)).min() > 1e-6                   # what makes equality independent of the f64 operation order
        assert 0 < want.sum() < m.sum()                                       # some labels left the frame
    expected_counts = {"empty": 0, "collision": 1, "minus_one_to_zero": 1, "lands_on_h": 1, "one_pixel_wide": 2}
    if case in expected_counts:
        assert int(want.sum()) == expected_counts[case]
    if case == "minus_one_to_zero":
        assert want[4, 0]                                                     # x' = -0.75 truncates to 0 and is kept
    if case == "lands_on_h":
        assert want[m.shape[0] - 1, 7]


def test_border_interpolate_and_warp_borders():
    assert A.border_interpolate_101(np.array([-1, -2, 0, 4, 5, 6, 9, -9, 13, -300, 300]), 5).tolist() == [1, 2, 0, 4, 3, 2, 1, 1, 3, 4, 4]
    assert A.border_interpolate_101(np.array([-7, 0, 3]), 1).tolist() == [0, 0, 0]
    assert A.border_interpolate_101(np.array([-3, -2, -1, 0, 1, 2, 3]), 2).tolist() == [1, 0, 1, 0, 1, 0, 1]
    rng = np.random.default_rng(0)
    img = rng.random((20, 28), dtype=np.float32)
    shift = np.array([[1.0, 0.0, 3.0], [0.0, 1.0, -2.0], [0.0, 0.0, 1.0]])        # dst(x, y) = src(x - 3, y + 2)
    const, refl = A.warp_perspective_f32(img, shift, False), A.warp_perspective_f32(img, shift, True)
    assert np.array_equal(const[:-2, 3:], img[2:, :-3]) and np.array_equal(refl[:-2, 3:], img[2:, :-3])
    assert not const[:, :3].any() and not const[-2:].any()
    assert np.array_equal(refl[:-2, 0], img[2:, 3]) and np.array_equal(refl[-1, 3:], img[-3, :-3])       # x = -3 -> 3; y = 20 -> 18
    assert np.array_equal(A.warp_perspective_f32(img, np.eye(3), True), img)


def test_restated_valid_mask():
    m = A.compute_valid_mask((20, 28), np.eye(3), 0, True)
    assert m.all()
    m = A.compute_valid_mask((20, 28), np.eye(3), 2, True)
    assert m[2:-2, 2:-2].all() and m.sum() == 16 * 24                       # the zero frame eats r pixels
    assert A.compute_valid_mask((20, 28), np.eye(3), 2, False).all()          # cv2.erode's default border never erodes
    shift = np.array([[1.0, 0.0, 5.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    m = A.compute_valid_mask((20, 28), shift, 0, False)
    assert not m[:, :5].any() and m[:, 5:].all()


def test_filter2d_and_gaussian_blur_agree_with_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    img = rng.random((12, 8))
    for mode, ks in (('h', 11), ('v', 5), ('diag_down', 7), ('diag_up', 11), ('h', 1)):       # ksize 11 on an 8-pixel-wide image: two folds
        k = A.motion_blur_kernel(mode, ks)
        assert np.array_equal(k, aug.motion_blur_kernel(mode, ks)) and abs(k.sum() - 1) < 1e-15
        assert np.abs(A.filter2d(img, k) - ndi.correlate(img, k, mode='mirror')).max() <= 1e-12, (mode, ks)
    for ks in (9, 15, 31):                                                     # 31: the radius exceeds both dimensions
        k = A.gaussian_kernel(ks)
        assert np.array_equal(k, aug.gaussian_kernel(ks))
        want = ndi.correlate(ndi.correlate(img, k[None, :], mode='mirror'), k[:, None], mode='mirror')
        assert np.abs(A.gaussian_blur(img, ks) - want).max() <= 1e-12, ks


def test_ellipse_mask_is_the_analytic_inside_test():
    t = A.ellipse_table([[20, 12, 8, 4, 0.0], [5, 5, 0, 3, 90.0]])
    m = A.ellipse_mask((24, 40), t)
    assert m[12, 12] == 1 and m[12, 28] == 1 and m[12, 11] == 0 and m[8, 20] == 1 and m[7, 20] == 0          # the axis ends are inside
    assert m[5, 5] == 1 and set(np.unique(m)) == {0.0, 1.0}
    shaded = A.additive_shade(np.full((24, 40), 0.5), t, 0.8, 9)
    assert shaded.min() < 0.5 - 0.1 and shaded.max() == 0.5


def test_sample_photometric_params_ranges_and_reproducibility():
    B, h, w = 16, 24, 40
    p = aug.sample_photometric_params(PHOTO_CONFIG, B, (h, w), np.random.default_rng(7))
    q = aug.sample_photometric_params(PHOTO_CONFIG, B, (h, w), np.random.default_rng(7))
    assert sorted(p) == sorted(q) and all(np.array_equal(p[k], q[k]) for k in p)
    r = aug.sample_photometric_params(PHOTO_CONFIG, B, (h, w), np.random.default_rng(8))
    assert not np.array_equal(p['params'], r['params'])
    assert p['ops'].shape == (B, 6) and all(sorted(row) == list(range(6)) for row in p['ops'].tolist())
    assert len({tuple(row) for row in p['ops'].tolist()}) > 1                  # the orders differ between samples
    lo = {'additive_gaussian_noise': 0, 'additive_speckle_noise': 0, 'random_brightness': -0.15, 'random_contrast': 0.3, 'additive_shade': -0.5}
    hi = {'additive_gaussian_noise': 0.06, 'additive_speckle_noise': 0.0035, 'random_brightness': 0.15, 'random_contrast': 1.8, 'additive_shade': 0.8}
    for i in range(B):
        for s, op in enumerate(p['ops'][i]):
            name, v = aug.PRIMITIVES[op], float(p['params'][i, s])
            if name == 'motion_blur':
                ks = int(v)
                assert ks == v and ks % 2 == 1 and 1 <= ks <= 9                 # randint(0, (10 + 1) / 2) * 2 + 1
                k = p['motion_kernel'][i]
                assert abs(float(k[:ks * ks].sum()) - 1) < 1e-6 and not k[ks * ks:].any()
            else:
                assert np.float32(lo[name]) <= v <= np.float32(hi[name]), (name, v)
    ks = p['shade_ksize']
    assert ((ks % 2) == 1).all() and (ks >= 9).all() and (ks <= 15).all()
    assert np.allclose(p['shade_weights'].sum(1), 1, atol=1e-6)
    e = p['ellipses']
    assert e.shape == (B, 6, 6) and (e[..., 2] >= 0.5).all() and (e[..., 2] <= min(h, w) / 4).all() and np.allclose(e[..., 4] ** 2 + e[..., 5] ** 2, 1)
    assert (e[..., 0] >= 0).all() and (e[..., 0] < w).all() and (e[..., 1] >= 0).all() and (e[..., 1] < h).all()
    assert (e[..., 4] >= 0).all() and (e[..., 5] >= 0).all()                    # angles in [0, 90)
    fixed = aug.sample_photometric_params(dict(PHOTO_CONFIG, random_order=False), 3, (h, w), np.random.default_rng(0))
    assert all(row == [aug.PRIMITIVES.index(n) for n in PHOTO_CONFIG['primitives']] for row in fixed['ops'].tolist())
    with pytest.raises(ValueError):
        aug.sample_photometric_params(dict(PHOTO_CONFIG, primitives=['sharpen']), 1, (h, w), np.random.default_rng(0))
    with pytest.raises(ValueError):
        aug.sample_photometric_params(dict(PHOTO_CONFIG, params={'motion_blur': {'max_kernel_size': 30}}, primitives=['motion_blur']), 64, (h, w),
                                      np.random.default_rng(0))


def test_sample_homography_corner_maps_perturbed_corners_back():
    cfg = {'rho': 16, 'patch_size': 64}
    h, w = 160, 192
    for seed in range(5):
        random.seed(seed)
        Hm = hom.sample_homography_corner((h, w), cfg)
        random.seed(seed)                                                        # the reference's draw order
        px, py = random.randint(16, w - 16 - 64), random.randint(16, h - 16 - 64)
        four = [(px, py), (px + 64, py), (px + 64, py + 64), (px, py + 64)]
        pert = [(x + random.randint(-16, 16), y + random.randint(-16, 16)) for x, y in four]
        q = Hm @ np.array([[x, y, 1.0] for x, y in pert]).T
        assert np.abs((q[:2] / q[2]).T - np.array(four, np.float64)).max() < 1e-8
        assert Hm.dtype == np.float64 and Hm.shape == (3, 3)


def test_hm_regression_points_match_the_restatement():
    h, w = 160, 192
    np.random.seed(3)
    Hm = hom.sample_homography((h, w)).astype(np.float32)
    eye = np.eye(3, dtype=np.float32)
    img = np.arange(h * w, dtype=np.float32).reshape(h, w)
    for Ho, Ht in ((Hm, eye), (eye, Hm)):
        pts, (y0, y1, x0, x1) = aug.hm_regression_points(Ho, Ht, h, w)
        crop, want = A.prep_hm_regression_input(img, -img, Ho, Ht, h, w)
        assert np.array_equal(pts, want) and (y0, y1, x0, x1) == (w // 2 - 64, w // 2 + 64, h // 2 - 64, h // 2 + 64)
        assert crop.shape == (2, 128, 128) and np.array_equal(crop[0], img[y0:y1, x0:x1]) and np.array_equal(crop[1], -img[y0:y1, x0:x1])
        assert np.abs(pts).max() > 0
    # no projective division: the first point is int(M[0] . (x, y, 1)) - x
    p = np.array([h // 2 - 64, w // 2 - 64, 1.0])
    pts, _ = aug.hm_regression_points(Hm, eye, h, w)
    assert pts[0].tolist() == [int(Hm[0].astype(np.float64) @ p) - (h // 2 - 64), int(Hm[1].astype(np.float64) @ p) - (w // 2 - 64)]


def test_augmentation_symbols_declared_exported_and_bound():
    lib = _lib.load()
    declared = _lib.exported_symbols()
    bound = set(_lib._SIGNATURES) | set(_lib._SIZE_QUERIES)
    for n in SYMBOLS:
        assert n in declared and hasattr(lib, n) and n in bound, n
    assert lib.xp_aug_partials_per_sample(24, 40) == 4 and lib.xp_aug_partials_per_sample(256, 256) == 256
    assert lib.xp_aug_partials_per_sample(0, 5) == 0
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "..", "include", "xpoint_hip.h")).read()
    for i, n in enumerate(aug.PRIMITIVES):                                       # the opcodes are the reference's list order
        macro = {"additive_gaussian_noise": "GAUSSIAN_NOISE", "additive_speckle_noise": "SPECKLE_NOISE", "random_brightness": "BRIGHTNESS",
                 "random_contrast": "CONTRAST", "additive_shade": "SHADE", "motion_blur": "MOTION_BLUR"}[n]
        assert f"#define XP_AUG_{macro} {i}\n" in hdr
    assert aug.PRIMITIVES == A.PRIMITIVES
    # argument errors surface as return codes with a message
    assert lib.xp_aug_warp(None, None, None, None, None, 1, 4, 4, 1, None) < 0 and b"null" in lib.xp_last_error()
    assert lib.xp_aug_scatter_labels(None, None, None, None, 1, 4, 4, None) < 0
    assert lib.xp_aug_random_field(None, 0, None, 0, 0, 1, 4, None) < 0
    assert lib.xp_aug_photo_prologue(None, None, None, None, 0, 1, 4, 4, None) < 0
    assert lib.xp_aug_blur(None, None, None, None, 1, 1, 4, 4, 0, None) < 0
    assert lib.xp_aug_photo_step(None, None, None, None, 0, 1, None, None, None, None, None, None, 0, None, 1, 4, 4, None) < 0


def test_every_entry_point_raises_on_cpu_tensors():
    img = torch.rand(2, 1, 24, 40)
    kp = torch.zeros(2, 24, 40, dtype=torch.bool)
    Hs = np.stack([np.eye(3)] * 2)
    with pytest.raises(_lib.XPointHipError):
        aug.homographic_augmentation(img, kp, Hs)
    prog = aug.make_programs([[2], [2]], [[0.1], [0.1]])
    with pytest.raises(_lib.XPointHipError):
        aug.photometric_augmentation(img, prog, seed=1)
    with pytest.raises(_lib.XPointHipError):
        aug.random_field(1, [0, 1], 'additive_gaussian_noise', (24, 40), 'normal', device="cpu")
    batch = {k: {'image': img, 'valid_mask': torch.ones_like(img, dtype=torch.bool), 'keypoints': kp} for k in ('optical', 'thermal')}
    with pytest.raises(_lib.XPointHipError):
        aug.augment_pair_batch(batch, {'photometric': {'enable': False}, 'homographic': {'enable': False}}, np.random.default_rng(0), 0)


def test_image_pair_dataset_still_raises_for_the_augmentation_keys(tmp_path):
    from PIL import Image
    from xpoint_amd.datasets import ImagePairDataset
    for spec in ("optical", "thermal"):
        os.makedirs(tmp_path / spec)
        Image.fromarray(np.zeros((64, 64), np.uint8)).save(tmp_path / spec / "a.png")
    ImagePairDataset({"foldername": str(tmp_path)})
    for key in ("photometric", "homographic"):
        with pytest.raises(NotImplementedError):
            ImagePairDataset({"foldername": str(tmp_path), "augmentation": {key: {"enable": True}}})
