"""SyntheticShapes on the device against the numpy restatement (tests/synthetic_shapes_f64.py).

The frame before the Gaussian must EQUAL the restatement (coverage, painter's order, resolved colours rounded to f32; uncovered pixels are the
device's own background); the background, the frame after the Gaussian passes and the final image are within 1e-4 absolute of the f64
restatement on images in [0, 1] (the project's standing bar); the per-image background mean within 1e-6; the label map equals the host's
points.  Largest errors seen on an MI355X: background 5.3e-8, after the Gaussian passes 4.1e-7, final image 3.9e-7, background mean 7.3e-9, the
box blur alone (kernels up to 500, wider than the frame) 4.5e-8."""
import numpy as np
import pytest
import torch

from tests import synthetic_shapes_f64 as ref
from xpoint_amd import _lib
from xpoint_amd import augmentation as aug
from xpoint_amd import synthetic_shapes as ss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
SIZES = {'small': ([96, 128], [24, 32]), 'ragged': ([100, 136], [30, 52]), 'equal': ([96, 128], [96, 128])}


def config(primitives, size='small', **kw):
    gen, img = SIZES[size]
    c = {'primitives': primitives, 'generation_size': gen, 'image_size': img,
         'generation': {'generate_background': {'min_kernel_size': 9, 'max_kernel_size': 15}},
         'augmentation': {'photometric': {'enable': False}, 'homographic': {'enable': False}}}
    c.update(kw)
    return c


def one_per_primitive(size, seed=5):
    """indices (consecutive from 0) and forced primitives: a batch that mixes all the implemented primitives"""
    return [ss.sample_draw_lists(config([p], size), [i], seed)[0] for i, p in enumerate(ss.IMPLEMENTED)]


def render_lists(lists, size, seed, **kw):
    gen, img = SIZES[size]
    tables = ss.pack_draw_lists(lists, gen)
    tables['min_contrast'] = 0.1
    image, kmap, dbg = ss.render(tables, gen, img, seed, DEV, debug=True, **kw)
    torch.cuda.synchronize()
    return tables, image, kmap, dbg


def check_against_restatement(lists, size, seed, **kw):
    gen, img = SIZES[size]
    tables, image, kmap, dbg = render_lists(lists, size, seed, **kw)
    ids = [d['index'] for d in lists]
    bg_field = aug.random_field(seed, ids, ss.KEY_BACKGROUND, gen, 'uniform', DEV).cpu().numpy()
    noise = aug.random_field(seed, ids, ss.KEY_NOISE, gen, 'uniform', DEV).cpu().numpy()
    worst = {'background': 0.0, 'blurred': 0.0, 'image': 0.0, 'bg_mean': 0.0}
    for b in range(len(lists)):
        r = ref.render(tables, b, bg_field[b], noise[b], gen, img, 0.1, **kw)
        got_bg = dbg['background'][b].cpu().numpy()
        assert abs(float(dbg['field_mean'][b]) - r['field_mean']) < 1e-12
        worst['background'] = max(worst['background'], float(np.abs(got_bg - r['background']).max()))
        worst['bg_mean'] = max(worst['bg_mean'], abs(float(dbg['bg_mean'][b]) - r['bg_mean']))
        # the frame before the Gaussian: equal, pixel for pixel
        expect = ref.compose(tables, b, got_bg, r['cover'], r['colours'], noise[b]).astype(np.float32)
        got = dbg['frame'][b].cpu().numpy()
        assert np.array_equal(got, expect), f"{lists[b]['primitive']}: {int((got != expect).sum())} pixels of the pre-blur frame differ"
        assert np.array_equal(dbg['colours'][b].cpu().numpy()[:len(lists[b]['records'])], np.float32(r['colours'])[:len(lists[b]['records'])])
        worst['blurred'] = max(worst['blurred'], float(np.abs(dbg['blurred'][b].cpu().numpy() - r['blurred']).max()))
        worst['image'] = max(worst['image'], float(np.abs(image[b, 0].cpu().numpy() - r['image']).max()))
        assert np.array_equal(kmap[b].cpu().numpy(), r['keypoints'])
        assert int(kmap[b].sum()) == len({tuple(p) for p in lists[b]['keypoints'].tolist()})
    print(f"synthetic shapes {size} {sorted({d['primitive'] for d in lists})}: largest errors {worst}")
    assert worst['background'] < TOL and worst['blurred'] < TOL and worst['image'] < TOL and worst['bg_mean'] < 1e-6, worst
    assert image.shape == (len(lists), 1, *img) and image.dtype == torch.float32 and kmap.dtype == torch.bool
    return image, kmap, dbg


@pytest.mark.parametrize("primitive", ss.IMPLEMENTED)
def test_every_primitive_against_the_restatement(primitive):
    lists = ss.sample_draw_lists(config([primitive]), [3, 40, 7], seed=9)          # B = 3 images from different keys
    check_against_restatement(lists, 'small', 9)


@pytest.mark.parametrize("size", ['small', 'ragged', 'equal'])
def test_mixed_batch_at_every_size(size):
    check_against_restatement(one_per_primitive(size), size, 5)


def test_single_image():
    check_against_restatement(one_per_primitive('small')[5:6], 'small', 5)


def test_multiple_polygons_is_refused():
    with pytest.raises(NotImplementedError, match="draw_multiple_polygons"):
        ss.SyntheticShapes(config(['draw_multiple_polygons']))


def test_thermal_samples_take_the_second_gaussian():
    lists = one_per_primitive('small')[:4]
    for flag in (True, False):
        for d in lists:
            d['is_optical'] = flag
        _, _, dbg = check_against_restatement(lists, 'small', 5)
        _, _, _, plain = render_lists(lists, 'small', 5, additional_ir_blur=False)
        same = torch.equal(dbg['blurred'], plain['blurred'])
        assert same == flag          # optical: the size-1 pass copies bit for bit; thermal: the 51-tap pass ran
    # a batch without a thermal sample skips the second pair of passes; any other batch runs it, whatever its size
    gen, img = SIZES['small']
    for flags, calls in (([True] * 4, 2), ([False] * 4, 4), ([True, False, True, True], 4), ([False], 4), ([True], 2)):
        some = lists[:len(flags)]
        for d, f in zip(some, flags):
            d['is_optical'] = f
        tables = ss.pack_draw_lists(some, gen)
        assert aug.profile_launches(lambda: ss.render(tables, gen, img, 5, DEV))['aug_blur'][0] == calls, flags
    for d in lists:
        d['is_optical'] = False
    lists[1]['is_optical'] = True          # a batch that mixes both
    _, _, _, mixed = render_lists(lists, 'small', 5)
    assert torch.equal(mixed['blurred'][1], plain['blurred'][1]) and not torch.equal(mixed['blurred'][0], plain['blurred'][0])


@pytest.mark.parametrize("shape,ks", [((40, 70), [500, 150, 2]), ((96, 128), [151, 64, 1]), ((1, 300), [33, 8, 301]), ((130, 1), [7, 500, 2]),
                                      ((67, 2), [5, 4, 9])])
def test_box_blur_wide_kernels(shape, ks):
    """kernels wider than the frame (the reflected extension wraps several times), even sizes, one-pixel dimensions, more than one column
    segment (130 rows)"""
    H, W = shape
    g = torch.Generator().manual_seed(1)
    src = torch.rand((len(ks), H, W), generator=g, dtype=torch.float32)
    d_src, tmp, dst = src.to(DEV), torch.empty((len(ks), H, W), device=DEV), torch.empty((len(ks), H, W), device=DEV)
    kd = torch.tensor(ks, dtype=torch.int32, device=DEV)
    _lib.call("xp_synth_box_blur", _lib.ptr(d_src), _lib.ptr(tmp), _lib.ptr(dst), _lib.ptr(kd), len(ks), H, W, _lib.current_stream())
    torch.cuda.synchronize()
    err = max(float(np.abs(dst[i].cpu().numpy() - ref.box_blur(src[i].numpy(), k)).max()) for i, k in enumerate(ks))
    print(f"box blur {shape} {ks}: largest error {err:.3g}")
    assert err < TOL
    inplace = d_src.clone()
    _lib.call("xp_synth_box_blur", _lib.ptr(inplace), _lib.ptr(tmp), _lib.ptr(inplace), _lib.ptr(kd), len(ks), H, W, _lib.current_stream())
    assert torch.equal(inplace, dst)


def test_two_calls_and_batch_neighbours_change_no_bit():
    ds = ss.SyntheticShapes(config('all', 'ragged', augmentation={'photometric': {'enable': True}, 'homographic': {'enable': True}}))
    five = ds.load_batch([11, 2, 30, 4, 19], DEV, seed=3)
    again = ds.load_batch([11, 2, 30, 4, 19], DEV, seed=3)
    alone = ds.load_batch([30], DEV, seed=3)
    for k in ('image', 'keypoints', 'valid_mask', 'is_optical'):
        assert torch.equal(five[k], again[k]), k
        assert torch.equal(five[k][2:3], alone[k]), k
    r5 = ds.render_batch([11, 2, 30, 4, 19], DEV, seed=3)
    r1 = ds.render_batch([30], DEV, seed=3)
    assert torch.equal(r5[0][2:3], r1[0]) and torch.equal(r5[1][2:3], r1[1])
    assert not torch.equal(five['image'][2], ds.load_batch([30], DEV, seed=4)['image'][0])


def test_load_batch_end_to_end():
    cfg = config('all', 'small', augmentation={'photometric': {'enable': False}, 'homographic': {'enable': True, 'valid_border_margin': 1}})
    ds = ss.SyntheticShapes(cfg)
    idx = [6, 1, 13]
    out = ds.load_batch(idx, DEV, seed=21)
    image, kmap, lists = ds.render_batch(idx, DEV, seed=21)
    w_img, w_map, mask = aug.homographic_augmentation(image, kmap, ds.homographies(idx, 21), border_reflect=True, valid_border_margin=1, mask_border=True)
    assert torch.equal(out['image'], w_img) and torch.equal(out['keypoints'], w_map) and torch.equal(out['valid_mask'], mask)
    assert out['image'].shape == (3, 1, 24, 32) and out['image'].dtype == torch.float32
    assert out['keypoints'].shape == (3, 24, 32) and out['keypoints'].dtype == torch.bool
    assert out['valid_mask'].shape == (3, 1, 24, 32) and out['valid_mask'].dtype == torch.bool and not bool(out['valid_mask'].all())
    assert out['is_optical'].shape == (3, 1) and out['is_optical'].dtype == torch.bool
    assert out['is_optical'][:, 0].tolist() == [d['is_optical'] for d in lists]
    assert float(out['image'].min()) >= 0.0 and float(out['image'].max()) <= 1.0
    # the photometric stage changes the image only: labels and mask are those of the plain pipeline
    full = ss.SyntheticShapes(config('all', 'small', augmentation={'photometric': {'enable': True}, 'homographic': {'enable': True, 'valid_border_margin': 1}}))
    aug_out = full.load_batch(idx, DEV, seed=21)
    assert torch.equal(aug_out['keypoints'], out['keypoints']) and torch.equal(aug_out['valid_mask'], out['valid_mask'])
    assert not torch.equal(aug_out['image'], out['image'])
    forced = full.load_batch(idx, DEV, seed=21, is_optical=False)
    assert not bool(forced['is_optical'].any())
    plain = ss.SyntheticShapes(config('all', 'small')).load_batch(idx, DEV, seed=21)
    assert bool(plain['valid_mask'].all()) and torch.equal(plain['image'], image) and torch.equal(plain['keypoints'], kmap)


def test_cli_synth_writes_the_samples(tmp_path):
    import yaml
    from xpoint_amd import cli
    cfg = {'dataset': dict(config('all', 'small', augmentation={'photometric': {'enable': True}, 'homographic': {'enable': True}}), type='SyntheticShapes'),
           'training': {'batchsize': 3}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    out = tmp_path / "out" / "shapes.npz"
    cli.main(['synth', '-y', str(tmp_path / "cfg.yaml"), '-n', '5', '-i', '2', '-s', '3', '-o', str(out)])
    z = np.load(out)
    assert z['image'].shape == (5, 1, 24, 32) and z['image'].dtype == np.float32 and z['keypoints'].shape == (5, 24, 32) and z['keypoints'].dtype == bool
    assert z['valid_mask'].shape == (5, 1, 24, 32) and z['is_optical'].shape == (5, 1)
    ds_cfg = {k: v for k, v in cfg['dataset'].items() if k != 'type'}
    one = ss.SyntheticShapes(ds_cfg).load_batch([4], DEV, seed=3)          # sample 4 = row 2, whatever the batching
    assert np.array_equal(z['image'][2], one['image'][0].cpu().numpy()) and np.array_equal(z['keypoints'][2], one['keypoints'][0].cpu().numpy())
