"""draw_multiple_polygons (textured polygons) on the device against the numpy restatement (tests/textured_polygons_f64.py).

Per job the unblurred texture over its texture box must EQUAL the restatement's; a pixel that a textured record wins must hold, bit for bit,
the device's blurred value of that record's job, and every other pixel of the frame before the Gaussian must EQUAL the flat composition
(coverage, painter's order, colours rounded to f32, the device's own background): together they pin the set of textured pixels.  The blurred
boxes, the frame before the Gaussian inside the polygons, the frame after the Gaussian passes and the final image are within 1e-4 absolute of
the f64 restatement on images in [0, 1] (the project's standing bar); with ksize = 1 the whole frame before the Gaussian is EQUAL.  The label
map equals the host's points.  Largest errors seen on an MI355X: blurred boxes 5.6e-8, frame before the Gaussian inside the polygons 5.6e-8,
after the Gaussian passes 5.0e-7, final image 3.9e-7."""
import numpy as np
import pytest
import torch

from tests import synthetic_shapes_f64 as ref
from tests import textured_polygons_f64 as tex
from xpoint_amd import augmentation as aug
from xpoint_amd import synthetic_shapes as ss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
SIZES = {'small': ([96, 128], [24, 32]), 'ragged': ([100, 136], [30, 52])}
KB = (5, 9)
FLAT = {'synth_background': 1, 'synth_box_blur': 1, 'synth_resolve_colours': 1, 'synth_rasterise': 1, 'aug_blur': 2, 'synth_resize': 1,
        'synth_scatter_points': 1}          # the entry-point calls of an all-optical batch without a textured record


def config(primitives, size='small', **kw):
    gen, img = SIZES[size]
    c = {'primitives': primitives, 'textured_polygons': True, 'generation_size': gen, 'image_size': img,
         'generation': {'generate_background': {'min_kernel_size': 9, 'max_kernel_size': 15}, 'draw_multiple_polygons': {'kernel_boundaries': KB}},
         'augmentation': {'photometric': {'enable': False}, 'homographic': {'enable': False}}}
    c.update(kw)
    return c


def hand_list(records, index=0, points=()):
    return {'index': index, 'primitive': 'hand', 'is_optical': True, 'threshold': np.float32(0.5), 'blobs': [], 'blob_raw': [], 'bg_ksize': 1,
            'records': records, 'keypoints': np.asarray(points, np.int64).reshape(-1, 2)}


def textured(geom, ksize, ordinal, colour=0.3, nb_blobs=3000):
    rec = ss.make_record(ss.TEXTURED, geom, len(geom) // 2, ss.rule_abs(colour))
    rec.update(ksize=ksize, ordinal=ordinal, nb_blobs=nb_blobs)
    return rec


def render_lists(lists, size, seed, **kw):
    gen, img = SIZES[size]
    tables = ss.pack_draw_lists(lists, gen)
    tables['min_contrast'] = 0.1
    image, kmap, dbg = ss.render(tables, gen, img, seed, DEV, debug=True, **kw)
    torch.cuda.synchronize()
    return tables, image, kmap, dbg


def texture_uniforms(tables, lists, seed):
    """the (B, J, 4 NB) uniform draws of the batch's textures, from the generator on its own"""
    nb = int(tables.get('texture_blobs', 0))
    J = int(tables['records'][:, :, 23].max()) + 1
    if nb == 0:
        return np.zeros((len(lists), J, 0), np.float32)
    return aug.random_field(seed, [d['index'] for d in lists], ss.KEY_TEXTURE, (J, 4 * nb), 'uniform', DEV).cpu().numpy()


def check_against_restatement(lists, size, seed, whole_frame_equal=False):
    gen, img = SIZES[size]
    tables, image, kmap, dbg = render_lists(lists, size, seed)
    ids = [d['index'] for d in lists]
    bg_field = aug.random_field(seed, ids, ss.KEY_BACKGROUND, gen, 'uniform', DEV).cpu().numpy()
    noise = aug.random_field(seed, ids, ss.KEY_NOISE, gen, 'uniform', DEV).cpu().numpy()
    uni = texture_uniforms(tables, lists, seed)
    jobs = {(j['b'], j['r']): j for j in dbg.get('texture_jobs', [])}
    worst = {'texture_blur': 0.0, 'frame_inside': 0.0, 'blurred': 0.0, 'image': 0.0}
    n_textured = 0
    for b in range(len(lists)):
        r = tex.render(tables, b, bg_field[b], noise[b], uni[b], gen, img, 0.1, float(tables.get('texture_min_contrast', 0.13)))
        got_bg = dbg['background'][b].cpu().numpy()
        got = dbg['frame'][b].cpu().numpy()
        expect = ref.compose(tables, b, got_bg, r['cover'], r['colours'], noise[b]).astype(np.float32)          # flat: exact outside the textures
        for rec, ks, _ in tex.textured_records(tables, b):
            won = r['cover'] == rec
            if (b, rec) not in jobs:
                assert not won.any()          # a polygon outside the frame has no job and wins no pixel
                continue
            j = jobs[(b, rec)]
            (x0, y0, x1, y1), (tx0, ty0, tx1, ty1) = j['box'], j['texture_box']
            assert j['ksize'] == ks
            assert np.array_equal(j['texture'].cpu().numpy(), r['textures'][rec][ty0:ty1 + 1, tx0:tx1 + 1].astype(np.float32)), "the unblurred texture"
            dev_blur = j['blurred'].cpu().numpy()
            worst['texture_blur'] = max(worst['texture_blur'], float(np.abs(dev_blur - r['texture_blurs'][rec][y0:y1 + 1, x0:x1 + 1]).max()))
            full = np.zeros(gen, np.float32)
            full[y0:y1 + 1, x0:x1 + 1] = dev_blur
            assert not won[:y0].any() and not won[y1 + 1:].any() and not won[:, :x0].any() and not won[:, x1 + 1:].any()
            expect[won] = full[won]
            n_textured += int(won.sum())
        assert np.array_equal(got, expect), f"{lists[b]['primitive']}: {int((got != expect).sum())} pixels of the pre-blur frame differ"
        if r['textured'].any():
            worst['frame_inside'] = max(worst['frame_inside'], float(np.abs(got - r['frame'])[r['textured']].max()))
        if whole_frame_equal:
            assert np.array_equal(got, r['frame'].astype(np.float32))
        assert np.array_equal(dbg['colours'][b].cpu().numpy()[:len(lists[b]['records'])], np.float32(r['colours'])[:len(lists[b]['records'])])
        worst['blurred'] = max(worst['blurred'], float(np.abs(dbg['blurred'][b].cpu().numpy() - r['blurred']).max()))
        worst['image'] = max(worst['image'], float(np.abs(image[b, 0].cpu().numpy() - r['image']).max()))
        assert np.array_equal(kmap[b].cpu().numpy(), r['keypoints'])
        assert int(kmap[b].sum()) == len({tuple(p) for p in np.asarray(lists[b]['keypoints']).tolist()})
    print(f"textured polygons {size} {sorted({d['primitive'] for d in lists})}: {len(jobs)} jobs, {n_textured} textured pixels, largest errors {worst}")
    assert all(v < TOL for v in worst.values()), worst
    assert image.shape == (len(lists), 1, *img) and image.dtype == torch.float32 and kmap.dtype == torch.bool
    return n_textured, dbg


@pytest.mark.parametrize("size", ['small', 'ragged'])
def test_sampled_lists_against_the_restatement(size):
    lists = ss.sample_draw_lists(config(['draw_multiple_polygons'], size), [3, 40, 7], seed=9)          # three keys; every tile's list holds every blob
    assert sum(len(d['records']) for d in lists) >= 3
    n, _ = check_against_restatement(lists, size, 9)
    assert n > 0


W0, H0 = 128, 96
HAND = {
    'ksize 1': ([textured([20, 10, 100, 14, 90, 80, 30, 70], 1, 0)], True),
    'even and odd sizes': ([textured([5, 5, 60, 8, 50, 60, 8, 50], 4, 0), textured([70, 20, 120, 25, 110, 90, 75, 80], 7, 1), textured([64, 2, 69, 2, 66, 9], 2, 2)], False),
    'wider than the frame': ([textured([30, 20, 100, 30, 90, 70, 40, 75], 151, 0)], False),
    'touching the four borders': ([textured([0, 0, 30, 0, 0, 30], 9, 0), textured([W0 - 1, 0, W0 - 1, 40, W0 - 30, 0], 6, 1),
                                   textured([0, H0 - 1, 50, H0 - 1, 0, H0 - 20], 5, 2), textured([W0 - 1, H0 - 1, W0 - 1, H0 - 25, W0 - 40, H0 - 1], 8, 3),
                                   textured([-20, 40, 20, 30, 30, 60, -10, 70], 5, 4), textured([200, 200, 210, 200, 205, 210], 3, 5)], False),
    "painter's order": ([textured([10, 10, 90, 10, 90, 70, 10, 70], 5, 0), ss.make_record(ss.CIRCLE, [50, 40], 25, ss.rule_abs(0.9)),
                         textured([40, 20, 120, 30, 100, 90, 30, 80], 6, 1), ss.make_record(ss.SEGMENT, [0, 0, 127, 95], 7, ss.rule_abs(0.1)),
                         textured([60, 5, 80, 5, 80, 90, 60, 90], 3, 2)], False),
    'one-row sliver': ([textured([10, 50, 60, 50, 110, 50], 5, 0), textured([70, 10, 70, 40, 70, 25], 4, 1)], False),
}


@pytest.mark.parametrize("case", sorted(HAND))
def test_hand_made_lists(case):
    records, equal = HAND[case]
    n, _ = check_against_restatement([hand_list(records, index=12)], 'small', 4, whole_frame_equal=equal)
    assert n > 0


@pytest.mark.parametrize("nb_blobs", [0, 1, 4096])
def test_blob_counts(nb_blobs):
    recs = [textured([10, 10, 120, 20, 100, 90, 5, 80], 5, 0, nb_blobs=nb_blobs), textured([40, 30, 70, 30, 55, 60], 1, 1, colour=0.8, nb_blobs=nb_blobs)]
    n, dbg = check_against_restatement([hand_list(recs, index=5)], 'small', 2)
    assert n > 0
    if nb_blobs == 0:
        assert bool((dbg['texture_jobs'][0]['texture'] == np.float32(0.3)).all()) and bool((dbg['texture_jobs'][1]['blurred'] == np.float32(0.8)).all())


def one_per_primitive(size, seed=5):
    return [ss.sample_draw_lists(config([p], size), [i], seed)[0] for i, p in enumerate(ss.ALL_PRIMITIVES)]


@pytest.mark.parametrize("size", ['small', 'ragged'])
def test_mixed_batch_of_the_nine(size):
    lists = one_per_primitive(size)
    assert [d['primitive'] for d in lists] == ss.ALL_PRIMITIVES
    check_against_restatement(lists, size, 5)


def calls(fn):
    return {tag: row[0] for tag, row in aug.profile_launches(fn).items()}


def test_bits_batches_and_launch_counts():
    gen, img = SIZES['ragged']
    idx = [11, 2, 30, 4]
    prims = ['draw_multiple_polygons', 'draw_star', 'draw_multiple_polygons', 'draw_multiple_polygons']
    lists = [ss.sample_draw_lists(config([p], 'ragged'), [k], 3, is_optical=True)[0] for k, p in zip(idx, prims)]
    t4 = ss.pack_draw_lists(lists, gen)
    assert len(ss.texture_jobs(t4, gen)['jobs']) > 3
    four, again = ss.render(t4, gen, img, 3, DEV), ss.render(t4, gen, img, 3, DEV)
    assert torch.equal(four[0], again[0]) and torch.equal(four[1], again[1])
    for i in range(4):
        alone = ss.render(ss.pack_draw_lists(lists[i:i + 1], gen), gen, img, 3, DEV)
        assert torch.equal(four[0][i:i + 1], alone[0]) and torch.equal(four[1][i:i + 1], alone[1]), idx[i]
    # launches: a constant more, whatever the batch and the number of polygons
    t1 = ss.pack_draw_lists([hand_list([textured([10, 10, 90, 10, 50, 70], 5, 0)])], gen)
    with_textures = {**{k: v for k, v in FLAT.items() if k != 'synth_rasterise'}, 'synth_texture': 1, 'synth_rasterise_textured': 1}
    assert calls(lambda: ss.render(t1, gen, img, 3, DEV)) == with_textures
    assert calls(lambda: ss.render(t4, gen, img, 3, DEV)) == with_textures
    # a batch without a textured record launches the existing sequence, with the key set or not
    stars = ss.sample_draw_lists(config(['draw_star'], 'ragged'), idx, 3, is_optical=True)
    assert calls(lambda: ss.render(ss.pack_draw_lists(stars, gen), gen, img, 3, DEV)) == FLAT


def test_generation_size():
    """960 x 1280, the reference's kernels (50 .. 99) and 3 000 blobs: properties only"""
    cfg = {'primitives': ['draw_multiple_polygons'], 'textured_polygons': True}
    ds = ss.SyntheticShapes(cfg)
    image, kmap, lists = ds.render_batch([5, 8], DEV, seed=1)
    assert image.shape == (2, 1, 240, 320) and bool(torch.isfinite(image).all()) and float(image.min()) >= 0.0 and float(image.max()) <= 1.0
    assert all(len(d['records']) > 0 for d in lists) and int(kmap.sum()) > 0
    again, kmap2, _ = ds.render_batch([5, 8], DEV, seed=1)
    alone, kmap1, _ = ds.render_batch([8], DEV, seed=1)
    assert torch.equal(image, again) and torch.equal(kmap, kmap2)
    assert torch.equal(image[1:2], alone) and torch.equal(kmap[1:2], kmap1)
    tables = ss.pack_draw_lists(lists, [960, 1280])
    jobs = ss.texture_jobs(tables, [960, 1280])
    print(f"generation size: {len(jobs['jobs'])} jobs, arena {jobs['arena_floats'] * 4 / 2 ** 20:.1f} MiB = {jobs['arena_floats'] / (2 * 960 * 1280):.2f} frames per image")
    assert jobs['arena_floats'] < 3 * 960 * 1280 * len(jobs['jobs'])


def test_load_batch_end_to_end():
    cfg = config('all', 'small', augmentation={'photometric': {'enable': True}, 'homographic': {'enable': True, 'valid_border_margin': 1}})
    ds = ss.SyntheticShapes(cfg)
    idx = list(range(12))
    out = ds.load_batch(idx, DEV, seed=21)
    _, _, lists = ds.render_batch(idx, DEV, seed=21)
    assert 'draw_multiple_polygons' in {d['primitive'] for d in lists}
    assert out['image'].shape == (12, 1, 24, 32) and out['image'].dtype == torch.float32
    assert out['keypoints'].shape == (12, 24, 32) and out['keypoints'].dtype == torch.bool
    assert out['valid_mask'].shape == (12, 1, 24, 32) and out['valid_mask'].dtype == torch.bool
    assert out['is_optical'].shape == (12, 1) and out['is_optical'][:, 0].tolist() == [d['is_optical'] for d in lists]
    assert bool(torch.isfinite(out['image']).all()) and float(out['image'].min()) >= 0.0 and float(out['image'].max()) <= 1.0
    i = [d['primitive'] for d in lists].index('draw_multiple_polygons')
    alone = ds.load_batch([idx[i]], DEV, seed=21)
    for k in ('image', 'keypoints', 'valid_mask', 'is_optical'):
        assert torch.equal(out[k][i:i + 1], alone[k]), k


def test_cli_synth_textured_polygons(tmp_path):
    import yaml
    from xpoint_amd import cli
    ds_cfg = {k: v for k, v in config(['draw_multiple_polygons'], 'small').items() if k != 'textured_polygons'}
    ds_cfg['generation']['draw_multiple_polygons']['kernel_boundaries'] = list(KB)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump({'dataset': dict(ds_cfg, type='SyntheticShapes'), 'training': {'batchsize': 2}}))
    out = tmp_path / "shapes.npz"
    with pytest.raises(NotImplementedError, match="draw_multiple_polygons"):
        cli.main(['synth', '-y', str(tmp_path / "cfg.yaml"), '-n', '3', '-s', '3', '-o', str(out)])
    cli.main(['synth', '-y', str(tmp_path / "cfg.yaml"), '-n', '3', '-i', '2', '-s', '3', '-o', str(out), '--textured-polygons'])
    z = np.load(out)
    assert z['image'].shape == (3, 1, 24, 32) and z['image'].dtype == np.float32 and z['keypoints'].shape == (3, 24, 32) and z['keypoints'].dtype == bool
    one = ss.SyntheticShapes(dict(ds_cfg, textured_polygons=True)).load_batch([4], DEV, seed=3)          # sample 4 = row 2, whatever the batching
    assert np.array_equal(z['image'][2], one['image'][0].cpu().numpy()) and np.array_equal(z['keypoints'][2], one['keypoints'][0].cpu().numpy())
