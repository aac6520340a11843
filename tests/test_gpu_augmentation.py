"""GPU: the training-pair augmentation (xpoint_amd/augmentation.py, csrc/augment.hip) against the numpy restatement
(tests/augmentation_f64.py) and the REAL reference (tests/golden/g29_augmentation.npz): warps, valid masks and label maps for equality, the
photometric chain to the project's parity tolerance 1e-4, the generator bit for bit, determinism, batch invariance, launch counts and the
assembled training batch through XPointLoss."""
import numpy as np
import pytest
import torch

from tests import augmentation_f64 as A
from xpoint_amd import _lib, augmentation as aug, homographies as hom, utils

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G29 = "g29_augmentation.npz"
TOL = 1e-4                                  # the project's parity tolerance (README)
# normal field against the f64 Box-Muller of the same uniforms: 16 x the maximum of the first MI355X run, capped at 1e-4
NORMAL_BOUND = min(16 * 9.315e-07, 1e-4)
OP = {n: i for i, n in enumerate(aug.PRIMITIVES)}
ALL6 = ['additive_gaussian_noise', 'additive_speckle_noise', 'random_brightness', 'random_contrast', 'additive_shade', 'motion_blur']


def _images(B, h, w, seed):
    return np.random.default_rng(seed).random((B, 1, h, w), dtype=np.float32)


def _warp_homographies(h, w):
    np.random.seed(11)
    mild = hom.sample_homography(np.array([h, w]), perspective_amplitude_x=0.15, perspective_amplitude_y=0.15, max_angle=0.5)
    far = np.array([[1.0, 0.0, 3.6 * w], [0.0, 1.0, -3.3 * h], [0.0, 1e-4, 1.0]])          # every pre-image lies > 2 image sizes outside
    return np.stack([mild, far, np.array([[0.9, 0.2, 3.0], [-0.1, 1.1, 2.0], [1e-3, 0.0, 1.0]])])


@pytest.mark.parametrize("border_reflect", [True, False])
def test_warp_bit_equal_to_the_restatement(gpu_lib, border_reflect):
    B, h, w = 3, 40, 56
    img = _images(B, h, w, 0)
    Hs = _warp_homographies(h, w)
    flags = np.array([True, True, False])
    X, Y = A._fixed_point_source(Hs[1], h, w, 32.0)
    assert ((X >> 5) < -2 * w).all() and ((Y >> 5) >= 3 * h).all()                  # more than two image sizes outside: repeated folding at every tap
    d = torch.from_numpy(img).to(DEV)
    out, kp, mask = aug.homographic_augmentation(d, None, Hs, warp=flags, border_reflect=border_reflect)
    assert kp is None and out.shape == d.shape and mask.shape == d.shape and mask.dtype == torch.bool and out.dtype == torch.float32
    got = out.cpu().numpy()
    for i in range(2):
        want = A.warp_perspective_f32(img[i, 0], Hs[i], border_reflect)
        assert np.array_equal(got[i, 0].view(np.uint32), want.view(np.uint32)), (i, float(np.abs(got[i, 0] - want).max()))
    assert got[1].any() == border_reflect                                          # far outside: zeros without the reflection
    assert np.array_equal(got[2].view(np.uint32), img[2].view(np.uint32)) and bool(mask[2].all())           # warp=False: untouched, all-ones mask
    assert not bool(mask[1].any()) and 0 < int(mask[0].sum()) < h * w
    if not border_reflect:
        ref = utils.warp_perspective(d[:2], Hs[:2])
        assert ref.shape == (2, 1, h, w) and torch.equal(ref.contiguous().view(torch.int32), out[:2].contiguous().view(torch.int32))
    everything = aug.homographic_augmentation(d, None, Hs, border_reflect=border_reflect)[0]               # warp=None: all warped
    assert torch.equal(everything[:2], out[:2]) and not torch.equal(everything[2], d[2])


@pytest.mark.parametrize("margin,mask_border", [(0, True), (0, False), (4, True), (4, False)])
def test_valid_mask_equals_xp_ha_valid_mask_and_the_restatement(gpu_lib, margin, mask_border):
    B, h, w = 3, 40, 56
    Hs = _warp_homographies(h, w)
    Hs[1] = np.array([[1.0, 0.0, 9.5], [0.0, 1.0, -6.25], [0.0, 0.0, 1.0]])
    d = torch.from_numpy(_images(B, h, w, 1)).to(DEV)
    _, _, mask = aug.homographic_augmentation(d, None, Hs, warp=[True, True, False], valid_border_margin=margin, mask_border=mask_border)
    Hd = torch.from_numpy(Hs.reshape(B, 9)).to(DEV)
    direct, tmp = torch.empty((B, h, w), dtype=torch.uint8, device=DEV), torch.empty((B, h, w), dtype=torch.uint8, device=DEV)
    _lib.call("xp_ha_valid_mask", _lib.ptr(Hd), _lib.ptr(direct), _lib.ptr(tmp), B, h, w, 2 * margin, 1 if mask_border else 0, _lib.current_stream())
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(mask[i, 0], direct[i].bool()), i
        assert np.array_equal(mask[i, 0].cpu().numpy(), A.compute_valid_mask((h, w), Hs[i], 2 * margin, mask_border)), i
    assert bool(mask[2].all())
    assert 0 < int(mask[0].sum()) < h * w and 0 < int(mask[1].sum()) < h * w


def test_label_maps_equal_the_restatement_and_the_reference(gpu_lib, golden):
    g = golden(G29)
    cases = ["sampled0", "sampled1", "sampled2", "empty", "collision", "minus_one_to_zero", "lands_on_h"]
    maps = np.stack([g[f"labels/{c}/map"] for c in cases])
    Hs = np.stack([g[f"labels/{c}/H"] for c in cases])
    B, h, w = maps.shape
    img = torch.zeros((B, 1, h, w), device=DEV)
    for reflect in (True, False):
        _, kp, _ = aug.homographic_augmentation(img, torch.from_numpy(maps).to(DEV), Hs, border_reflect=reflect)
        assert kp.dtype == torch.bool and tuple(kp.shape) == (B, h, w)
        got = kp.cpu().numpy()
        for i, c in enumerate(cases):
            assert np.array_equal(got[i], A.warp_label_map(maps[i], Hs[i])), c
            assert np.array_equal(got[i], g[f"labels/{c}/out"]), c
    assert got[4].sum() == 1 and got[5, 4, 0] and got[5].sum() == 1 and got[6].sum() == 1 and got[6, h - 1, 7] and got[3].sum() == 0
    # uint8 maps are accepted; warp=False copies the map
    _, kp, _ = aug.homographic_augmentation(img, torch.from_numpy(maps.astype(np.uint8)).to(DEV), Hs, warp=[i != 0 for i in range(B)])
    assert np.array_equal(kp[0].cpu().numpy(), maps[0]) and np.array_equal(kp[1:].cpu().numpy(), got[1:])
    # a 1-pixel-wide image
    m, Hm = g["labels/one_pixel_wide/map"], g["labels/one_pixel_wide/H"]
    x = torch.from_numpy(_images(1, m.shape[0], 1, 2)).to(DEV)
    out, kp, mask = aug.homographic_augmentation(x, torch.from_numpy(m[None]).to(DEV), Hm[None])
    assert np.array_equal(kp[0].cpu().numpy(), g["labels/one_pixel_wide/out"]) and np.array_equal(kp[0].cpu().numpy(), A.warp_label_map(m, Hm))
    want = A.warp_perspective_f32(x[0, 0].cpu().numpy(), Hm, True)
    assert np.array_equal(out[0, 0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(mask[0, 0].cpu().numpy(), A.compute_valid_mask(m.shape, Hm, 0, True))


# Shapes (h, w) that drive the block structure of OpenCV's coordinate arithmetic (csrc/cv_geom.h): the row base is formed at the first
# column of the pixel's block.  24 x 200: 64-wide blocks, three full plus a ragged 8; 16 x 65: ragged 1; 9 x 130: a height under 16, 113-wide
# blocks, ragged 17; 3 x 700: 341-wide blocks, ragged 18; one pixel.  Matrices of tests/test_gpu_warp.py: the horizon comes near
# (projective) or crosses (strong) the image, or the inverse is the zero matrix (singular): W == 0, the clamp and the 16-bit saturation.
BLOCK_SHAPES = [(24, 200), (16, 65), (9, 130), (3, 700), (1, 1)]
BLOCK_KINDS = ["projective", "strong", "singular"]
_block_cache = {}


def _block_case(shape):
    """images, matrices and the restatement's results of one shape, computed once; no test writes to them"""
    if shape not in _block_cache:
        from tests.test_gpu_warp import _homography
        h, w = shape
        img = _images(len(BLOCK_KINDS), h, w, 100 * h + w)
        Hs = np.stack([_homography(k, h, w) for k in BLOCK_KINDS])
        case = {"img": img, "Hs": Hs}
        for reflect in (True, False):
            case[reflect] = np.stack([A.warp_perspective_f32(img[i, 0], Hs[i], reflect) for i in range(len(BLOCK_KINDS))])
        for r, frame in ((0, True), (2, True), (2, False)):
            case[r, frame] = np.stack([A.compute_valid_mask(shape, Hs[i], r, frame) for i in range(len(BLOCK_KINDS))])
        _block_cache[shape] = case
    return _block_cache[shape]


def _assert_masks_are_not_trivial(shape, mask):
    """where the restatement gives a mask that is neither empty nor full (fractions 0.81, 0.54, 0.54, 0.08 for projective, 0.20 for strong
    at 24 x 200; the strong masks of the smaller shapes are empty or nearly so and are not asserted)"""
    h, w = shape
    if shape != (1, 1):
        assert 0 < int(mask[BLOCK_KINDS.index("projective")].sum()) < h * w
    if shape == (24, 200):
        assert 0 < int(mask[BLOCK_KINDS.index("strong")].sum()) < h * w


@pytest.mark.parametrize("border_reflect", [True, False])
@pytest.mark.parametrize("shape", BLOCK_SHAPES)
def test_warp_through_the_block_structure(gpu_lib, shape, border_reflect):
    h, w = shape
    case = _block_case(shape)
    d = torch.from_numpy(case["img"]).to(DEV)
    out, _, mask = aug.homographic_augmentation(d, None, case["Hs"], border_reflect=border_reflect)
    got = out.cpu().numpy()
    assert got.shape == case["img"].shape and got.dtype == np.float32
    for i, kind in enumerate(BLOCK_KINDS):
        assert np.array_equal(got[i, 0].view(np.uint32), case[border_reflect][i].view(np.uint32)), kind
    assert np.array_equal(mask[:, 0].cpu().numpy(), case[0, True])
    _assert_masks_are_not_trivial(shape, mask[:, 0].cpu().numpy())
    if not border_reflect:
        ref = utils.warp_perspective(d, case["Hs"])
        assert ref.shape == out.shape and torch.equal(ref.contiguous().view(torch.int32), out.contiguous().view(torch.int32))


@pytest.mark.parametrize("radius,mask_border", [(0, True), (2, True), (2, False)])
@pytest.mark.parametrize("shape", BLOCK_SHAPES)
def test_valid_mask_through_the_block_structure(gpu_lib, shape, radius, mask_border):
    h, w = shape
    case = _block_case(shape)
    K = len(BLOCK_KINDS)
    Hd = torch.from_numpy(case["Hs"].reshape(K, 9)).to(DEV)
    direct, tmp = torch.empty((K, h, w), dtype=torch.uint8, device=DEV), torch.empty((K, h, w), dtype=torch.uint8, device=DEV)
    _lib.call("xp_ha_valid_mask", _lib.ptr(Hd), _lib.ptr(direct), _lib.ptr(tmp), K, h, w, radius, 1 if mask_border else 0, _lib.current_stream())
    torch.cuda.synchronize()
    want = case[radius, mask_border]
    for i, kind in enumerate(BLOCK_KINDS):
        assert np.array_equal(direct[i].cpu().numpy().astype(bool), want[i]), kind
    # the augmentation's mask is this entry point's (valid_border_margin = radius / 2)
    _, _, mask = aug.homographic_augmentation(torch.from_numpy(case["img"]).to(DEV), None, case["Hs"], valid_border_margin=radius // 2,
                                              mask_border=mask_border)
    assert np.array_equal(mask[:, 0].cpu().numpy(), want)
    if radius == 0:
        _assert_masks_are_not_trivial(shape, want)


# ----------------------------------------------------------------------------------------------- photometric
def _run(img, prog, fields=None, seed=0, sample_ids=None):
    out = aug.photometric_augmentation(torch.from_numpy(img).to(DEV), prog, seed, sample_ids=sample_ids, fields=fields)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(got, img, prog, fields, what):
    worst = 0.0
    for i in range(img.shape[0]):
        want = A.run_program(img[i, 0], prog, i, fields)
        worst = max(worst, float(np.abs(got[i, 0].astype(np.float64) - want).max()))
    print(f"{what}: max |device - f64 restatement| = {worst:.3e}")
    assert worst <= TOL, (what, worst)
    return worst


@pytest.mark.parametrize("name", ['additive_gaussian_noise', 'additive_speckle_noise', 'random_brightness', 'random_contrast'])
def test_numpy_only_primitives_against_the_reference(gpu_lib, golden, name):
    """each of the four primitives the reference runs without OpenCV, alone, with the reference's input, scalar and field"""
    g = golden(G29)
    x, s, f, want = g[f"photo/{name}/input"], float(g[f"photo/{name}/scalar"]), g[f"photo/{name}/field"], g[f"photo/{name}/output"]
    prog = aug.make_programs([[OP[name]]], [[s]])
    f32 = f.astype(np.float32)[None]
    got = _run(x[None, None], prog, fields={name: f32})
    err = float(np.abs(got[0, 0].astype(np.float64) - want).max())
    print(f"{name}: max |device - reference| = {err:.3e}")
    assert err <= TOL
    _check(got, x[None, None], prog, {name: f32}, name)
    if name == 'additive_speckle_noise':
        lo, hi = A.speckle_positions(s, f)                  # the reference's positions (f64 field, f64 prob)
        assert np.array_equal(got[0, 0] == 0.0, lo | (x == 0.0)) and np.array_equal(got[0, 0] == 1.0, hi | (x == 1.0)) and lo.sum() > 0 and hi.sum() > 0
        untouched = ~(lo | hi)
        assert np.array_equal(got[0, 0][untouched].view(np.uint32), x[untouched].view(np.uint32))


def _chain_programs(B, h, w, orders, shade_range, motion_ks, seed):
    rng = np.random.default_rng(seed)
    cfg = {'primitives': ALL6, 'random_order': False,
           'params': {'additive_gaussian_noise': {'stddev_range': [0.02, 0.06]}, 'additive_speckle_noise': {'prob_range': [0.01, 0.03]},
                      'random_brightness': {'max_abs_change': 0.15}, 'random_contrast': {'strength_range': [0.3, 1.8]},
                      'additive_shade': {'transparency_range': [-0.5, 0.8], 'kernel_size_range': shade_range, 'nb_ellipses': 5},
                      'motion_blur': {'max_kernel_size': 10}}}
    p = aug.sample_photometric_params(cfg, B, (h, w), rng)
    ops = np.array([[OP[n] for n in order] for order in orders], np.int32)
    params = np.zeros((B, 6), np.float32)
    for i in range(B):
        for s, op in enumerate(ops[i]):
            params[i, s] = p['params'][i, list(p['ops'][i]).index(op)]
    modes = ['h', 'diag_up', 'v', 'diag_down']
    kernels = []
    for i in range(B):
        params[i, list(ops[i]).index(OP['motion_blur'])] = motion_ks[i]
        kernels.append(aug.motion_blur_kernel(modes[i % 4], motion_ks[i]))
    ell = np.concatenate([p['ellipses'][..., :4], np.rad2deg(np.arctan2(p['ellipses'][..., 5], p['ellipses'][..., 4]))[..., None]], -1)
    return aug.make_programs(ops, params, ell, p['shade_ksize'], kernels)


ORDERS3 = [ALL6, ALL6[::-1], ['random_contrast', 'motion_blur', 'additive_gaussian_noise', 'additive_shade', 'additive_speckle_noise', 'random_brightness']]


def _golden_fields(golden, B, h, w):
    g = golden(G29)
    z, u = g["photo/additive_gaussian_noise/field"], g["photo/additive_speckle_noise/field"]
    assert h <= 24 and w <= 40
    return {'additive_gaussian_noise': np.stack([z[8 * i:8 * i + h, 8 * i:8 * i + w] for i in range(B)]).astype(np.float32),
            'additive_speckle_noise': np.stack([u[8 * i:8 * i + h, 8 * i:8 * i + w] for i in range(B)]).astype(np.float32)}


def test_photometric_chain_three_orders(gpu_lib, golden):
    B, h, w = 3, 24, 40
    img = _images(B, h, w, 3)
    prog = _chain_programs(B, h, w, ORDERS3, [9, 15], [5, 9, 3], 4)
    assert len({tuple(r) for r in prog['ops'].tolist()}) == 3 and ((prog['shade_ksize'] >= 9) & (prog['shade_ksize'] <= 15)).all()
    fields = _golden_fields(golden, B, h, w)
    got = _run(img, prog, fields)
    _check(got, img, prog, fields, "chain 3 x 24 x 40")
    # speckle as the LAST step, so that its positions show in the output: exactly the field's
    last = [ALL6[2:] + ['additive_gaussian_noise', 'additive_speckle_noise']] * B
    prog2 = _chain_programs(B, h, w, last, [9, 15], [5, 9, 3], 4)
    got2 = _run(img, prog2, fields)
    _check(got2, img, prog2, fields, "chain ending in speckle")
    for i in range(B):
        lo, hi = A.speckle_positions(prog2['params'][i, 5], fields['additive_speckle_noise'][i])
        assert lo.sum() + hi.sum() > 0 and (got2[i, 0][lo] == 0.0).all() and (got2[i, 0][hi] == 1.0).all()


def test_motion_blur_kernel_wider_than_the_image(gpu_lib):
    B, h, w = 4, 12, 8
    img = _images(B, h, w, 5)
    kernels = [aug.motion_blur_kernel(m, 11) for m in ('h', 'v', 'diag_down', 'diag_up')]
    prog = aug.make_programs([[OP['motion_blur']]] * B, [[11]] * B, motion_kernels=kernels)
    got = _run(img, prog)
    _check(got, img, prog, None, "motion blur 11 on 12 x 8")
    assert np.abs(got - img).max() > 0.05


@pytest.mark.parametrize("h,w,ksize", [(24, 40, 15), (12, 20, 31)])
def test_shade_blur_radius(gpu_lib, h, w, ksize):
    B = 2
    img = _images(B, h, w, 6)
    ell = np.array([[[w // 2, h // 2, w // 5, h // 4, 30.0], [3, 3, 2, 0, 75.0]], [[w // 3, h // 3, 3, 5, 0.0], [w - 4, h - 4, 3, 3, 89.0]]], np.float64)
    prog = aug.make_programs([[OP['additive_shade']]] * B, [[0.8], [-0.5]], ell, [ksize, 9])
    got = _run(img, prog)
    _check(got, img, prog, None, f"shade {ksize} on {h} x {w}")
    assert (got[0] <= img[0]).all() and (got[0] < img[0] - 0.01).any() and (got[1] >= img[1]).all()      # transparency 0.8 darkens, -0.5 brightens


# ----------------------------------------------------------------------------------------------- generator
def test_generator_uniform_bits_and_normal_field(gpu_lib):
    h, w, seed, ids = 24, 40, 0x1234_5678_9ABC_DEF1, [0, 7, 123456]
    for prim in ('additive_speckle_noise', 'additive_gaussian_noise'):
        u = aug.random_field(seed, ids, prim, (h, w), 'uniform').cpu().numpy()
        for i, sid in enumerate(ids):
            want = A.uniform_field(seed, sid, OP[prim], h * w).reshape(h, w)
            assert np.array_equal(u[i].view(np.uint32), want.view(np.uint32)), (prim, sid)
        assert len({u[i].tobytes() for i in range(3)}) == 3 and 0.0 <= u.min() and u.max() < 1.0
    n = aug.random_field(seed, ids, 'additive_gaussian_noise', (h, w), 'normal').cpu().numpy()
    worst = 0.0
    for i, sid in enumerate(ids):
        want = A.normal_field_f64(seed, sid, OP['additive_gaussian_noise'], h * w).reshape(h, w)
        worst = max(worst, float(np.abs(n[i].astype(np.float64) - want).max()))
    print(f"normal field: max |device - f64 Box-Muller| = {worst:.3e} (bound {NORMAL_BOUND:.3e})")
    assert worst <= NORMAL_BOUND
    assert abs(float(n.mean())) < 0.1 and abs(float(n.std()) - 1) < 0.1
    # the fields the steps generate are these fields: gaussian noise with stddev 1 on a mid-grey image without clipping range issues
    img = np.full((3, 1, h, w), 0.5, np.float32)
    prog = aug.make_programs([[OP['additive_gaussian_noise']]] * 3, [[0.01]] * 3)
    got = _run(img, prog, seed=seed, sample_ids=ids)
    assert np.array_equal(got[:, 0], np.clip(np.float32(0.5) + np.float32(0.01) * n, 0, 1).astype(np.float32))
    prog = aug.make_programs([[OP['additive_speckle_noise']]] * 3, [[0.05]] * 3)
    got = _run(img, prog, seed=seed, sample_ids=ids)
    us = aug.random_field(seed, ids, 'additive_speckle_noise', (h, w), 'uniform').cpu().numpy()
    assert np.array_equal(got[:, 0] == 0.0, us < np.float32(0.05)) and np.array_equal(got[:, 0] == 1.0, us > np.float32(1) - np.float32(0.05))


def _slice(prog, i):
    return {k: v[i:i + 1] for k, v in prog.items()}


def test_determinism_and_batch_invariance(gpu_lib):
    B, h, w, seed, ids = 3, 24, 40, 99, [5, 6, 7]
    img = _images(B, h, w, 8)
    prog = _chain_programs(B, h, w, ORDERS3, [9, 15], [5, 9, 3], 9)
    a, b = _run(img, prog, seed=seed, sample_ids=ids), _run(img, prog, seed=seed, sample_ids=ids)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a, _run(img, prog, seed=seed + 1, sample_ids=ids))
    for i in range(B):
        alone = _run(img[i:i + 1], _slice(prog, i), seed=seed, sample_ids=ids[i:i + 1])
        assert np.array_equal(alone[0].view(np.uint32), a[i].view(np.uint32)), i
    Hs = _warp_homographies(h, w)
    maps = torch.from_numpy(np.random.default_rng(1).random((B, h, w)) < 0.05).to(DEV)
    d = torch.from_numpy(img).to(DEV)
    r1, r2 = aug.homographic_augmentation(d, maps, Hs, valid_border_margin=1), aug.homographic_augmentation(d, maps, Hs, valid_border_margin=1)
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))
    for i in range(B):
        alone = aug.homographic_augmentation(d[i:i + 1], maps[i:i + 1], Hs[i:i + 1], valid_border_margin=1)
        assert all(torch.equal(x[0], y[i]) for x, y in zip(alone, r1)), i


def test_launch_counts_do_not_depend_on_batch_or_order(gpu_lib):
    h, w = 24, 40
    counts = []
    for B, orders in ((1, ORDERS3[:1]), (3, ORDERS3), (3, [ORDERS3[2], ORDERS3[0], ORDERS3[1]])):
        prog = _chain_programs(B, h, w, orders, [9, 15], [5] * B, 2)
        d = torch.from_numpy(_images(B, h, w, 0)).to(DEV)
        rows = aug.profile_launches(lambda: aug.photometric_augmentation(d, prog, 1))
        assert set(rows) == {"aug_photo_prologue", "aug_blur", "aug_photo_step"}, rows
        counts.append({k: v[0] for k, v in rows.items()})
    assert counts[0] == counts[1] == counts[2] == {"aug_photo_prologue": 1, "aug_blur": 2, "aug_photo_step": 6}
    assert sum(counts[0].values()) <= 10
    hcounts = []
    for B in (1, 3):
        d = torch.from_numpy(_images(B, h, w, 0)).to(DEV)
        maps = torch.zeros((B, h, w), dtype=torch.bool, device=DEV)
        rows = aug.profile_launches(lambda: aug.homographic_augmentation(d, maps, _warp_homographies(h, w)[:B], valid_border_margin=2))
        hcounts.append({k: v[0] for k, v in rows.items()})
    assert hcounts[0] == hcounts[1] == {"ha_valid_mask": 1, "aug_warp": 1, "aug_scatter_labels": 1}


# ----------------------------------------------------------------------------------------------- assembled batch
CMT_LOSS = {'detector_loss': True, 'detector_use_cross_entropy': True, 'descriptor_loss': True, 'descriptor_loss_threshold': 4.0,
            'descriptor_loss_use_mask': True, 'sparse_descriptor_loss': False, 'sparse_descriptor_loss_num_cell_divisor': 64,
            'positive_margin': 1.0, 'negative_margin': 0.2, 'lambda_d': 250, 'lambda': 1.0, 'use_encoder_similarity': False,
            'homography_regression_loss': {'check': True, 'gamma': 1.0}, 'detector_loss_function': 'cross_entropy',
            'detector_handle_multiple_keypoints': 'hard_assignment', 'detector_dustbin_loss_weight': 1,
            'detector_focal_loss': {'use': False, 'alpha': 0.25, 'gamma': 2.0, 'reduction': 'mean'}}
CMT_AUG = {'photometric': {'enable': True, 'primitives': ['random_brightness', 'random_contrast', 'additive_speckle_noise',
                                                          'additive_gaussian_noise', 'additive_shade', 'motion_blur'],
                           'random_order': True,
                           'params': {'random_brightness': {'max_abs_change': 0.15}, 'random_contrast': {'strength_range': [0.3, 1.8]},
                                      'additive_gaussian_noise': {'stddev_range': [0, 0.06]}, 'additive_speckle_noise': {'prob_range': [0, 0.0035]},
                                      'additive_shade': {'transparency_range': [-0.5, 0.8], 'kernel_size_range': [50, 100]},
                                      'motion_blur': {'max_kernel_size': 3}}},
           'homographic': {'enable': True, 'valid_border_margin': 0, 'border_reflect': True,
                           'params': {'corner_homography': {'enable': False, 'params': {'patch_size': 128, 'rho': 32}}, 'translation': True,
                                      'rotation': True, 'scaling': True, 'perspective': True, 'scaling_amplitude': 0.2,
                                      'perspective_amplitude_x': 0.2, 'perspective_amplitude_y': 0.2, 'patch_ratio': 0.85, 'max_angle': 1.57,
                                      'allow_artifacts': True, 'translation_overflow': 0.05}}}


@pytest.mark.parametrize("labels_follow_warp", [True, False])
def test_augment_pair_batch_end_to_end(gpu_lib, labels_follow_warp):
    import random
    from xpoint_amd import losses
    B, h, w = 2, 160, 192
    rng = np.random.default_rng(0)
    batch = {'name': ['a', 'b']}
    for k, flag in (('optical', True), ('thermal', False)):
        img = torch.from_numpy(rng.random((B, 1, h, w), dtype=np.float32)).to(DEV)
        batch[k] = {'image': img, 'valid_mask': torch.ones_like(img, dtype=torch.bool), 'is_optical': torch.full((B, 1), flag, device=DEV),
                    'keypoints': torch.from_numpy(rng.random((B, h, w)) < 0.01).to(DEV)}
    np.random.seed(5); random.seed(5)
    pick = [True, False]
    data = aug.augment_pair_batch(batch, CMT_AUG, np.random.default_rng(1), seed=7, labels_follow_warp=labels_follow_warp, warp_optical=pick)
    assert set(data) == {'optical', 'thermal', 'name', 'hm_input', 'hfour_points'} and data['name'] == ['a', 'b']
    for k in ('optical', 'thermal'):
        d = data[k]
        assert set(d) == {'image', 'keypoints', 'valid_mask', 'homography', 'is_optical'}
        assert d['image'].shape == (B, 1, h, w) and d['image'].dtype == torch.float32 and d['image'].is_contiguous()
        assert d['keypoints'].shape == (B, h, w) and d['keypoints'].dtype == torch.bool
        assert d['valid_mask'].shape == (B, 1, h, w) and d['valid_mask'].dtype == torch.bool
        assert d['homography'].shape == (B, 3, 3) and d['homography'].dtype == torch.float32
        assert torch.equal(d['is_optical'], batch[k]['is_optical'])
        assert float(d['image'].min()) >= 0.0 and float(d['image'].max()) <= 1.0
    assert data['hm_input'].shape == (B, 2, 128, 128) and data['hm_input'].dtype == torch.float32 and data['hfour_points'].shape == (B, 4, 2)
    eye = torch.eye(3, device=DEV)
    Ho, Ht = data['optical']['homography'], data['thermal']['homography']
    assert torch.equal(Ht[0], eye) and torch.equal(Ho[1], eye) and not torch.equal(Ho[0], eye) and not torch.equal(Ht[1], eye)
    assert bool(data['thermal']['valid_mask'][0].all()) and bool(data['optical']['valid_mask'][1].all())
    assert not bool(data['optical']['valid_mask'][0].all()) and not bool(data['thermal']['valid_mask'][1].all())
    for i in range(B):
        o, t = data['optical']['image'][i, 0].cpu().numpy(), data['thermal']['image'][i, 0].cpu().numpy()
        crop, pts = A.prep_hm_regression_input(o, t, Ho[i].cpu().numpy(), Ht[i].cpu().numpy(), h, w)
        assert np.array_equal(data['hm_input'][i].cpu().numpy(), crop) and np.array_equal(data['hfour_points'][i].cpu().numpy(), pts)
        warped, plain = ('optical', 'thermal') if pick[i] else ('thermal', 'optical')
        assert torch.equal(data[plain]['keypoints'][i], batch[plain]['keypoints'][i])
        Hm = (Ho if pick[i] else Ht)[i].cpu().numpy()
        before = batch[warped]['keypoints'][i].cpu().numpy()
        if labels_follow_warp:
            # the f32 matrix handed out is the f64 one rounded: the maps are compared through the mask frame (labels inside the valid region)
            assert int(data[warped]['keypoints'][i].sum()) <= int(before.sum()) and not np.array_equal(data[warped]['keypoints'][i].cpu().numpy(), before)
        else:
            assert np.array_equal(data[warped]['keypoints'][i].cpu().numpy(), before)
        assert np.abs(Hm - np.eye(3)).max() > 1e-3
    crit = losses.XPointLoss(CMT_LOSS)
    g = torch.Generator().manual_seed(0)
    pred = {s: {'logits': torch.randn(B, 65, h // 8, w // 8, generator=g).to(DEV).requires_grad_(True),
                'desc': torch.nn.functional.normalize(torch.randn(B, 256, h // 8, w // 8, generator=g), dim=1).to(DEV).requires_grad_(True)}
            for s in ('optical', 'thermal')}
    pred_hm = torch.randn(B, 8, generator=g).to(DEV).requires_grad_(True)
    loss, comp = crit({'data': data, 'pred': pred['optical'], 'pred2': pred['thermal'], 'pred_hm': pred_hm})
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0 and 'homography_regression_loss' in comp and 'descriptor_loss' in comp
    assert bool(torch.isfinite(pred['optical']['logits'].grad).all()) and bool(torch.isfinite(pred_hm.grad).all())


def test_augment_pair_batch_labels_follow_the_given_homography(gpu_lib):
    """with the homographies given, the warped side's labels and image are the restatement's"""
    B, h, w = 2, 160, 192
    rng = np.random.default_rng(2)
    batch = {}
    for k in ('optical', 'thermal'):
        img = torch.from_numpy(rng.random((B, 1, h, w), dtype=np.float32)).to(DEV)
        batch[k] = {'image': img, 'valid_mask': torch.ones_like(img, dtype=torch.bool), 'keypoints': torch.from_numpy(rng.random((B, h, w)) < 0.01).to(DEV)}
    np.random.seed(2)
    Hs = np.stack([hom.sample_homography(np.array([h, w]), **{k: v for k, v in CMT_AUG['homographic']['params'].items() if k != 'corner_homography'})
                   for _ in range(B)])
    cfg = {'photometric': {'enable': False}, 'homographic': dict(CMT_AUG['homographic'], valid_border_margin=1)}
    data = aug.augment_pair_batch(batch, cfg, np.random.default_rng(0), 0, homographies=Hs, warp_optical=[False, True])
    assert 'name' not in data and 'is_optical' not in data['optical']
    for i, side in enumerate(('thermal', 'optical')):
        src = batch[side]
        assert np.array_equal(data[side]['keypoints'][i].cpu().numpy(), A.warp_label_map(src['keypoints'][i].cpu().numpy(), Hs[i]))
        want = A.warp_perspective_f32(src['image'][i, 0].cpu().numpy(), Hs[i], True)
        assert np.array_equal(data[side]['image'][i, 0].cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(data[side]['valid_mask'][i, 0].cpu().numpy(), A.compute_valid_mask((h, w), Hs[i], 2, True))
        assert np.array_equal(data[side]['homography'][i].cpu().numpy(), Hs[i].astype(np.float32))
        other = 'optical' if side == 'thermal' else 'thermal'
        assert torch.equal(data[other]['image'][i], batch[other]['image'][i]) and torch.equal(data[other]['keypoints'][i], batch[other]['keypoints'][i])
    plain = aug.augment_pair_batch(batch, {'photometric': {'enable': False}, 'homographic': {'enable': False}}, np.random.default_rng(0), 0)
    assert set(plain) == {'optical', 'thermal'} and torch.equal(plain['optical']['image'], batch['optical']['image'])
    assert bool(plain['thermal']['valid_mask'].all()) and torch.equal(plain['thermal']['keypoints'], batch['thermal']['keypoints'])
