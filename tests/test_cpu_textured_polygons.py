"""draw_multiple_polygons (textured polygons, opt-in by the dataset key `textured_polygons`) on the host: the default behaviour without the
key, the nine primitives with it, the sampler's invariants over 200 (seed, index) keys, determinism and batch independence, the numpy
restatement (tests/textured_polygons_f64.py) on hand-made uniform tables, the job tables of `texture_jobs`, the C ABI's declarations and
argument checks."""
import ctypes

import numpy as np
import pytest

from tests import synthetic_shapes_f64 as ref
from tests import textured_polygons_f64 as tex
from xpoint_amd import _lib
from xpoint_amd import synthetic_shapes as ss

GEN, IMG = [96, 128], [24, 32]
H, W = GEN
KB = (5, 9)
N_KEYS = 200
SYMBOLS = ["xp_synth_texture", "xp_synth_rasterise_textured"]


def config(primitives='all', textured=True, **kw):
    c = {'primitives': primitives, 'generation_size': GEN, 'image_size': IMG,
         'generation': {'generate_background': {'min_kernel_size': 9, 'max_kernel_size': 15}, 'draw_multiple_polygons': {'kernel_boundaries': KB}}}
    if textured is not None:
        c['textured_polygons'] = textured
    c.update(kw)
    return c


_CACHE = {}


def polygon_lists():
    if 'l' not in _CACHE:
        _CACHE['l'] = [d for seed in (0, 7) for d in ss.sample_draw_lists(config(['draw_multiple_polygons']), range(N_KEYS // 2), seed)]
    return _CACHE['l']


def test_without_the_key_nothing_changes():
    assert ss.DEFAULT_CONFIG['textured_polygons'] is False and len(ss.IMPLEMENTED) == 8 and 'draw_multiple_polygons' not in ss.IMPLEMENTED
    for c in (config('all', textured=None), config('all', textured=False)):
        assert ss.SyntheticShapes(c).primitives == ss.IMPLEMENTED
        assert {d['primitive'] for d in ss.sample_draw_lists(c, range(120), 3)} == set(ss.IMPLEMENTED)
    for c in (config(['draw_multiple_polygons'], textured=None), config(['draw_lines', 'draw_multiple_polygons'], textured=False)):
        with pytest.raises(NotImplementedError, match="draw_multiple_polygons"):
            ss.sample_draw_lists(c, [0], 0)
        with pytest.raises(NotImplementedError, match="draw_multiple_polygons"):
            ss.SyntheticShapes(c)
    # the key changes no draw of a sample of another primitive
    a = ss.sample_draw_lists(config(['draw_star'], textured=None), [4], 2)[0]
    b = ss.sample_draw_lists(config(['draw_star'], textured=True), [4], 2)[0]
    assert a['records'] == b['records'] and a['blobs'] == b['blobs'] and np.array_equal(a['points'], b['points'])


def test_with_the_key_all_means_the_nine():
    ds = ss.SyntheticShapes(config('all'))
    assert ds.primitives == ss.ALL_PRIMITIVES and len(ds.primitives) == 9
    assert ss.SyntheticShapes(config(['draw_lines', 'draw_multiple_polygons'])).primitives == ['draw_lines', 'draw_multiple_polygons']
    # the primitive of sample i is one uniform draw among nine: over 400 samples a given one is missing with probability (8 / 9)^400 < 1e-20
    seen = {d['primitive'] for d in ss.sample_draw_lists(config('all'), range(400), 3)}
    assert seen == set(ss.ALL_PRIMITIVES)
    assert ss.KEY_TEXTURE == 8 and ss.TEXTURED == 6 and ss.RECORD_INTS == 24


def test_sampler_invariants():
    counts = []
    for d in polygon_lists():
        recs = d['records']
        counts.append(len(recs))
        assert d['primitive'] == 'draw_multiple_polygons' and 0 <= len(recs) <= 30 and len(recs) <= ss.MAX_RECORDS
        assert all(r['kind'] == ss.TEXTURED for r in recs)
        assert [r['ordinal'] for r in recs] == list(range(len(recs)))
        polys = []
        for r in recs:
            assert 3 <= r['n'] <= 8 and len(r['geom']) == 2 * r['n'] and KB[0] <= r['ksize'] < KB[1]
            assert r['rule'][0] == ss.RULE_ABS and 0.0 <= r['rule'][1] < 1.0 and not r['rule'][1] < 0.13      # get_random_color(0, 0.13)
            assert r['nb_blobs'] == 3000 and r['min_contrast'] == 0.13
            polys.append(np.array(r['geom'], np.int64).reshape(-1, 2))
        for i, p in enumerate(polys):
            for q in polys[:i]:
                for a in range(len(q)):
                    for c in range(len(p)):
                        assert not ss.segments_intersect(tuple(q[a]), tuple(q[(a + 1) % len(q)]), tuple(p[c]), tuple(p[(c + 1) % len(p)]))
        circles = [r['circle'] for r in recs]
        for i, (x, y, rad) in enumerate(circles):
            assert rad >= min(H, W) / 10 and int(rad) <= x < max(int(W - rad), int(rad) + 1)
            for (x2, y2, rad2) in circles[:i]:
                assert not np.hypot(x - x2, y - y2) + min(rad, rad2) < max(rad, rad2)
        pts = np.concatenate(polys) if polys else np.zeros((0, 2), np.int64)
        assert np.array_equal(d['points'], pts) and d['keypoints'].shape == (len(pts), 2)
        t = ss.pack_draw_lists([d], GEN)
        rec = t['records'][0]
        for r, q in enumerate(recs):
            assert rec[r, 0] == ss.TEXTURED and rec[r, 5] == q['n'] and rec[r, 22] == q['ksize'] and rec[r, 23] == r
            assert rec[r, 6:6 + 2 * q['n']].tolist() == q['geom']
        if recs:
            assert t['texture_blobs'] == 3000 and t['texture_min_contrast'] == 0.13
    assert max(counts) > 1 and min(counts) >= 0


def test_determinism_independence_and_forced_flag():
    c = config(['draw_multiple_polygons'])
    one = ss.sample_draw_lists(c, [3], 11)[0]
    again = ss.sample_draw_lists(c, [3], 11)[0]
    inside = ss.sample_draw_lists(c, [0, 9, 3, 4, 1], 11)[2]
    for other in (again, inside):
        assert other['records'] == one['records'] and np.array_equal(other['points'], one['points']) and other['blobs'] == one['blobs']
    assert ss.sample_draw_lists(c, [3], 12)[0]['records'] != one['records']
    forced = ss.sample_draw_lists(c, [3], 11, is_optical=not one['is_optical'])[0]
    assert forced['records'] == one['records'] and forced['is_optical'] != one['is_optical']
    with pytest.raises(ValueError, match="max_sides"):
        ss.sample_draw_lists(config(['draw_multiple_polygons'], generation={'draw_multiple_polygons': {'max_sides': 9}}), [0], 0)
    with pytest.raises(ValueError, match="nb_blobs"):
        ss.sample_draw_lists(config(['draw_multiple_polygons'], generation={'draw_multiple_polygons': {'nb_blobs': 4097}}), [0], 0)


def uniforms(blobs, H, W):
    """the uniform row that decodes to the blobs [(cx, cy, r, u3)]: cell centres, so floor() gives the integers back"""
    return np.array([[(cx + 0.5) / W, (cy + 0.5) / H, (r + 0.5) / 20, u3] for cx, cy, r, u3 in blobs], np.float32).reshape(-1)


def test_restatement_texture_by_hand():
    h, w = 9, 12
    u = uniforms([(3, 3, 2, 0.5), (4, 3, 1, 0.05), (10, 7, 0, 0.9)], h, w)
    cx, cy, r, col = tex.blobs(u, h, w, 0.13)
    assert cx.tolist() == [3, 4, 10] and cy.tolist() == [3, 3, 7] and r.tolist() == [2, 1, 0]
    assert col.tolist() == [np.float32(0.5), np.float32((float(np.float32(0.05)) + 0.5) % 1.0), np.float32(0.9)]          # 0.05 < 0.13: shifted
    t = tex.texture(u, 0.25, h, w, 0.13)
    assert t[3, 1] == np.float32(0.5) and t[3, 2] == np.float32(0.5) and t[1, 3] == np.float32(0.5)          # blob 0 alone
    assert t[3, 3] == col[1] and t[3, 4] == col[1] and t[3, 5] == col[1] and t[2, 4] == col[1]             # the highest index wins
    assert (t == col[2]).sum() == 1 and t[7, 10] == col[2]                                                 # radius 0 covers one pixel
    assert t[0, 0] == np.float32(0.25) and (t == np.float32(0.25)).sum() == h * w - 13 - 1                   # 13 = the disc of radius 2
    assert np.array_equal(tex.blurred(t, 1), t)                                                            # k = 1 returns the texture
    assert np.array_equal(tex.texture(np.zeros(0, np.float32), 0.25, h, w, 0.13), np.full((h, w), np.float64(np.float32(0.25))))
    # reflection at a border against a direct sum: k = 5 at the corner (0, 0) and k = 4 (anchor 2) at the last column
    b5, b4 = tex.blurred(t, 5), tex.blurred(t, 4)
    idx = [2, 1, 0, 1, 2]
    assert abs(b5[0, 0] - t[np.ix_(idx, idx)].sum() / 25) < 1e-14
    cols, rows = [w - 3, w - 2, w - 1, w - 2], [5, 6, 7, 8]
    assert abs(b4[7, w - 1] - t[np.ix_(rows, cols)].sum() / 16) < 1e-14


def hand_list(records, index=0):
    return {'index': index, 'primitive': 'hand', 'is_optical': True, 'threshold': np.float32(0.5), 'blobs': [], 'blob_raw': [], 'bg_ksize': 1,
            'records': records, 'keypoints': np.zeros((0, 2), np.int64)}


def textured(geom, ksize, ordinal, colour=0.3, **kw):
    rec = ss.make_record(ss.TEXTURED, geom, len(geom) // 2, ss.rule_abs(colour))
    rec.update(ksize=ksize, ordinal=ordinal, **kw)
    return rec


def test_job_tables():
    recs = [textured([10, 10, 30, 10, 30, 20, 10, 20], 5, 0), ss.make_record(ss.CIRCLE, [5, 5], 3), textured([0, 90, 127, 90, 127, 95, 0, 95], 151, 1),
            textured([200, 200, 210, 200, 205, 210], 3, 2)]
    t = ss.pack_draw_lists([hand_list(recs)], GEN)
    assert ss.texture_jobs(ss.pack_draw_lists([hand_list(recs[1:2])], GEN), GEN) is None
    j = ss.texture_jobs(t, GEN)
    assert j['jobs'].shape == (2, ss.JOB_INTS) and j['ksize'] == (5, 151)          # the third polygon lies outside the frame: no job
    assert j['jobs'][0, :12].tolist() == [0, 0, 0, 5, 10, 10, 30, 20, 8, 8, 32, 22]
    assert j['jobs'][1, :12].tolist() == [0, 2, 1, 151, 0, 90, 127, 95, 0, 15, 127, 95]          # wider than the frame: every column; rows 15 .. 170 fold onto 15 .. 95
    sizes = [25 * 15 + 21 * 15 + 21 * 11, 128 * 81 + 128 * 81 + 128 * 6]
    assert j['arena_floats'] == sum(sizes) and j['offsets'].tolist() == [[0, 375, 690], [sizes[0], sizes[0] + 128 * 81, sizes[0] + 2 * 128 * 81]]
    assert j['units'].tolist() == [[0, 1, 13], [0, 15, 96], [0, 1, 3]]
    assert j['tex_offsets'][0].tolist()[:4] == [690, -1, sizes[0] + 2 * 128 * 81, -1]
    # even k: anchor k // 2, the window of x is [x - 2, x + 1]; at the frame's border the reflection folds back inside
    e = ss.texture_jobs(ss.pack_draw_lists([hand_list([textured([0, 0, 6, 0, 6, 4, 0, 4], 4, 0)])], GEN), GEN)
    assert e['jobs'][0, 4:12].tolist() == [0, 0, 6, 4, 0, 0, 7, 5]
    with pytest.raises(ValueError, match="ksize"):
        ss.pack_draw_lists([hand_list([textured([1, 1, 5, 1, 3, 5], 0, 0)])], GEN)
    with pytest.raises(ValueError, match="ksize"):
        ss.pack_draw_lists([hand_list([textured([1, 1, 5, 1, 3, 5], 501, 0)])], GEN)
    with pytest.raises(ValueError, match="nb_blobs"):
        ss.pack_draw_lists([hand_list([textured([1, 1, 5, 1, 3, 5], 3, 0, nb_blobs=4097)])], GEN)
    with pytest.raises(ValueError, match="share"):
        ss.pack_draw_lists([hand_list([textured([1, 1, 5, 1, 3, 5], 3, 0, nb_blobs=10), textured([1, 1, 5, 1, 3, 5], 3, 1, nb_blobs=11)])], GEN)


def test_symbols_declared_exported_and_bound():
    lib = _lib.load()
    declared = _lib.exported_symbols()
    for n in SYMBOLS:
        assert n in declared and n in _lib._SIGNATURES and hasattr(lib, n), n
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "xpoint_hip.h")).read()
    for line in ("#define XP_SYNTH_KEY_TEXTURE 8", "#define XP_SYNTH_TEXTURED 6", "#define XP_SYNTH_MAX_TEXTURE_BLOBS 4096", "#define XP_SYNTH_RECORD_INTS 24",
                 f"#define XP_SYNTH_JOB_INTS {ss.JOB_INTS}", f"#define XP_SYNTH_MAX_KSIZE {ss.MAX_KSIZE}"):
        assert line in hdr, line


def test_argument_errors_name_the_argument():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))           # never dereferenced: every call below fails its checks before any launch
    odd = ctypes.c_void_p(p.value + 4)

    def err(rc):
        assert rc != 0
        return lib.xp_last_error().decode()

    def texture(**kw):
        a = dict(arena=p, arena_floats=100, jobs=p, offsets=p, units=p, n_jobs=1, colours=p, n_records=4, seed=0, sample_ids=p, nb_blobs=3000,
                 min_contrast=0.13, min_ksize=5, max_ksize=9, n_tiles=1, n_rows=1, n_col_blocks=1, B=1, H=8, W=8, stream=None)
        assert set(kw) <= set(a)
        a.update(kw)
        return err(lib.xp_synth_texture(*a.values()))
    assert "nb_blobs" in texture(nb_blobs=4097) and "nb_blobs" in texture(nb_blobs=-1)
    assert "ksize" in texture(min_ksize=0) and "ksize" in texture(max_ksize=501) and "ksize" in texture(min_ksize=9, max_ksize=5)
    assert "B must" in texture(B=0) and "H must" in texture(H=0) and "W must" in texture(W=4097)
    assert "n_jobs" in texture(n_jobs=0) and "n_jobs" in texture(n_jobs=129) and "n_records" in texture(n_records=129)
    assert "min_contrast" in texture(min_contrast=1.5) and "arena_floats" in texture(arena_floats=0)
    assert "n_tiles" in texture(n_tiles=0) and "n_rows" in texture(n_rows=0) and "n_col_blocks" in texture(n_col_blocks=0)
    for name in ("arena", "jobs", "offsets", "units", "colours", "sample_ids"):
        msg = texture(**{name: None})
        assert "null pointer" in msg and msg.rstrip().endswith(name), msg
    msg = texture(offsets=odd)
    assert "misaligned" in msg and msg.rstrip().endswith("offsets"), msg

    def raster(**kw):
        a = dict(frame=p, records=p, colours=p, seed=0, sample_ids=p, arena=p, tex_offsets=p, n_records=4, B=1, H=8, W=8, stream=None)
        assert set(kw) <= set(a)
        a.update(kw)
        return err(lib.xp_synth_rasterise_textured(*a.values()))
    assert "n_records" in raster(n_records=0) and "B must" in raster(B=70000) and "W must" in raster(W=0)
    for name in ("frame", "records", "colours", "sample_ids", "arena", "tex_offsets"):
        msg = raster(**{name: None})
        assert "null pointer" in msg and msg.rstrip().endswith(name), msg
    for name in ("records", "tex_offsets"):
        msg = raster(**{name: odd})
        assert "misaligned" in msg and msg.rstrip().endswith(name), msg
    # the generator accepts the new slot and nothing beyond it
    assert "primitive" in err(lib.xp_aug_random_field(p, 0, p, 9, 0, 1, 8, None))
    # without a device the renderer refuses, as before
    with pytest.raises(_lib.XPointHipError, match="GPU"):
        ss.SyntheticShapes(config(['draw_multiple_polygons'])).load_batch([0], "cpu")
