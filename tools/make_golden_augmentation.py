"""Generate tests/golden/g29_augmentation.npz by running the parts of the REAL reference augmentation that need no OpenCV image routine
(imported from the reference tree with the harness shims of oracle/refharness, which this tool imports and does not modify) on the CPU.
Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_augmentation.py

  seed
  photo/<primitive>/{input, scalar, field, output}   the four numpy-only primitives of photometric_augmentation.py (additive_gaussian_noise,
                                                     additive_speckle_noise, random_brightness, random_contrast) under np.random.seed: the
                                                     f32-valued 48 x 64 input, the scalar and the field the primitive drew (re-drawn from the
                                                     same seed: np.random.normal(0, s, shape) is 0 + s * standard_normal of one stream), and the
                                                     reference's f64 output
  labels/<case>/{map, H, out}                        generate_keypoint_map(filter_points(warp_keypoints(nonzero(map), H), shape), shape) with
                                                     warp_keypoints on the harness's perspectiveTransform: three sampled homographies on a
                                                     random map, and the edge cases of the GPU test (empty map, two labels on one pixel, a label
                                                     landing in (-1, 0), a label landing at exactly h, a 1-pixel-wide image)
Conditions asserted (the seed is re-drawn until they hold): no warped coordinate of a SAMPLED homography lies within 1e-6 of an integer
(so that no truncation depends on the order of the f64 operations; the edge cases use matrices whose products are exact in f64 in any
order, and land on integers on purpose); no speckle sample lies within 1e-6 of prob or 1 - prob (so the positions survive the f32 cast of
the field).  Fixed zip timestamps: a re-run is byte-identical.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.refharness import stubs  # noqa: E402
from oracle.refharness.make_golden import savez_deterministic  # noqa: E402
from xpoint_amd import homographies as hom  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g29_augmentation.npz")
H, W = 48, 64
HOM_CONFIG = dict(translation=True, rotation=True, scaling=True, perspective=True, scaling_amplitude=0.2, perspective_amplitude_x=0.2,
                  perspective_amplitude_y=0.2, patch_ratio=0.85, max_angle=1.57, allow_artifacts=True, translation_overflow=0.05)
PHOTO_PARAMS = {'additive_gaussian_noise': {'stddev_range': [0.02, 0.06]}, 'additive_speckle_noise': {'prob_range': [0.01, 0.03]},
                'random_brightness': {'max_abs_change': 0.15}, 'random_contrast': {'strength_range': [0.3, 1.8]}}


def edge_cases():
    """name -> (label map, H); every product below is exact in f64"""
    def shift(tx, ty):
        return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])
    cases = {}
    cases["empty"] = (np.zeros((H, W), bool), shift(3.0, 2.0))
    m = np.zeros((H, W), bool); m[10, 20] = m[11, 21] = True                      # x' = 0.5 x + .., y' = 0.5 y + ..: (10, 20) and (11, 21) share a pixel
    cases["collision"] = (m, np.array([[0.5, 0.0, 1.0], [0.0, 0.5, 2.0], [0.0, 0.0, 1.0]]))
    m = np.zeros((H, W), bool); m[5, 3] = m[0, 0] = True                          # (5, 3) -> y' = 4.25, x' = -0.75 -> 0: kept; (0, 0) -> y' = -0.75 -> 0, x' = -3.75 -> -3: dropped
    cases["minus_one_to_zero"] = (m, shift(-3.75, -0.75))
    m = np.zeros((H, W), bool); m[H - 4, 7] = m[H - 5, 7] = True                  # y' = H exactly: dropped; y' = H - 1: kept
    cases["lands_on_h"] = (m, shift(0.0, 4.0))
    m = np.zeros((H, 1), bool); m[3, 0] = m[20, 0] = True
    cases["one_pixel_wide"] = (m, shift(0.25, 5.5))
    return cases


def main():
    stubs.install()
    from xpoint.datasets.augmentation import photometric_augmentation as ref_photo
    from xpoint.utils import homographies as ref_hom
    from xpoint.utils.utils import generate_keypoint_map

    def ref_labels(m, Hm):
        kp = np.stack(np.nonzero(m), 1)
        if kp.size > 0:
            kp = ref_hom.filter_points(ref_hom.warp_keypoints(kp, Hm), m.shape)
        return generate_keypoint_map(kp, m.shape)

    for seed in range(4096):
        g = {"seed": np.int64(seed)}
        rs = np.random.RandomState(seed)
        ok = True
        for k, name in enumerate(PHOTO_PARAMS):
            image = rs.uniform(0.0, 1.0, (H, W)).astype(np.float32)
            np.random.seed(seed * 16 + k)
            out = getattr(ref_photo, name)(image.astype(np.float64), **PHOTO_PARAMS[name])      # a copy: two primitives write in place
            np.random.seed(seed * 16 + k)
            cfg = PHOTO_PARAMS[name]
            field = np.zeros((H, W))
            if name == 'additive_gaussian_noise':
                scalar = np.random.uniform(*cfg['stddev_range']); field = np.random.standard_normal((H, W))
                assert np.array_equal(np.clip(image.astype(np.float64) + (0.0 + scalar * field), 0.0, 1.0), out)
            elif name == 'additive_speckle_noise':
                scalar = np.random.uniform(*cfg['prob_range']); field = np.random.uniform(size=(H, W))
                ok = ok and min(np.abs(field - scalar).min(), np.abs(field - (1.0 - scalar)).min()) > 1e-6
                assert (field < scalar).sum() > 0 and (field > 1.0 - scalar).sum() > 0
            elif name == 'random_brightness':
                scalar = np.random.uniform(-cfg['max_abs_change'], cfg['max_abs_change'])
            else:
                scalar = np.random.uniform(*cfg['strength_range'])
            g[f"photo/{name}/input"], g[f"photo/{name}/scalar"] = image, np.float64(scalar)
            g[f"photo/{name}/field"], g[f"photo/{name}/output"] = field, np.asarray(out, np.float64)
        label_map = rs.uniform(size=(H, W)) < 0.04
        kp = np.stack(np.nonzero(label_map), 1)
        np.random.seed(seed)
        for k in range(3):
            Hm = hom.sample_homography(np.array([H, W]), **HOM_CONFIG)
            exact = ref_hom.warp_keypoints(kp, Hm, return_type=np.float64)
            ok = ok and np.abs(exact - np.rint(exact)).min() > 1e-6
            g[f"labels/sampled{k}/map"], g[f"labels/sampled{k}/H"], g[f"labels/sampled{k}/out"] = label_map, Hm, ref_labels(label_map, Hm)
        if ok:
            break
    else:
        raise RuntimeError("no seed satisfies the conditions")
    for name, (m, Hm) in edge_cases().items():
        g[f"labels/{name}/map"], g[f"labels/{name}/H"], g[f"labels/{name}/out"] = m, Hm, ref_labels(m, Hm)
        print(f"labels/{name}: {int(m.sum())} labels -> {int(g[f'labels/{name}/out'].sum())}")
    for k in range(3):
        print(f"labels/sampled{k}: {int(label_map.sum())} labels -> {int(g[f'labels/sampled{k}/out'].sum())}")
    savez_deterministic(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(g)} arrays, seed {seed})")


if __name__ == "__main__":
    main()
