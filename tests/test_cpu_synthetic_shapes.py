"""SyntheticShapes on the host: the sampler's invariants over many (seed, index) keys, determinism and batch independence, the numpy
restatement (tests/synthetic_shapes_f64.py) on hand-made draw lists, the C ABI's declarations and argument checks, the dataset's refusals."""
import ctypes
import math

import numpy as np
import pytest

from tests import synthetic_shapes_f64 as ref
from xpoint_amd import _lib
from xpoint_amd import synthetic_shapes as ss

GEN, IMG = [96, 128], [24, 32]
H, W = GEN
SYMBOLS = ["xp_synth_background", "xp_synth_box_blur", "xp_synth_resolve_colours", "xp_synth_rasterise", "xp_synth_resize", "xp_synth_scatter_points"]
N_KEYS = 200


def config(primitives='all', **kw):
    c = {'primitives': primitives, 'generation_size': GEN, 'image_size': IMG,
         'generation': {'generate_background': {'min_kernel_size': 9, 'max_kernel_size': 15},
                        'draw_multiple_polygons': {'kernel_boundaries': (5, 9)}}}
    c.update(kw)
    return c


_CACHE = {}


def lists_of(primitive):
    if primitive not in _CACHE:
        _CACHE[primitive] = [d for seed in (0, 7) for d in ss.sample_draw_lists(config([primitive]), range(N_KEYS // 2), seed)]
    return _CACHE[primitive]


def records(d, kind):
    return [r for r in d['records'] if r['kind'] == kind]


@pytest.mark.parametrize("primitive", ss.IMPLEMENTED)
def test_background_and_final_keypoints(primitive):
    for d in lists_of(primitive):
        assert d['primitive'] == primitive and 0.0 <= d['threshold'] < 1.0
        assert len(d['blobs']) == 100 and len(d['blob_raw']) == 100 and 9 <= d['bg_ksize'] <= 15
        for cx, cy, r in d['blobs']:
            assert 0 <= cx < W and 0 <= cy < H and int(128 * 0.02) <= r <= int(128 * 0.031)
        assert len(d['records']) <= ss.MAX_RECORDS
        kp = d['keypoints']
        assert kp.shape == (len(d['points']), 2)
        assert (kp >= 0).all() and (kp[:, 0] < IMG[0]).all() and (kp[:, 1] < IMG[1]).all()
        expect = np.flip(d['points'], 1) * 0.25
        assert (np.minimum(expect.round().astype(int), np.array(IMG) - 1) == kp).all()


def test_draw_lines_counts_and_no_intersection():
    for d in lists_of('draw_lines'):
        segs = records(d, ss.SEGMENT)
        assert 1 <= len(segs) <= 10 and len(segs) == len(d['records']) and len(d['points']) == 2 * len(segs)
        for i, r in enumerate(segs):
            g = r['geom']
            assert r['n'] == 1 and r['rule'][0] == ss.RULE_CONTRAST          # ceil(96 * 0.01) .. int(96 * 0.02)
            assert 0 <= g[0] < W and 0 <= g[2] < W and 0 <= g[1] < H and 0 <= g[3] < H
            for q in segs[:i]:
                assert not ss.segments_intersect(q['geom'][0:2], q['geom'][2:4], g[0:2], g[2:4])


def corner_filter_by_hand(pre):
    """The reference's one-pass filter written out independently of ss.filter_corners: (kept corners, the angle of every corner that survives the
    distance filter, taken with its neighbours in that distance-filtered list)."""
    pre = [tuple(q) for q in pre]
    n = len(pre)
    far = [pre[i] for i in range(n) if math.hypot(pre[i - 1][0] - pre[i][0], pre[i - 1][1] - pre[i][1]) > 0.01]
    kept, angles = [], []
    for i, q in enumerate(far):
        a, b = far[i - 1], far[(i + 1) % len(far)]
        v1, v2 = (a[0] - q[0], a[1] - q[1]), (b[0] - q[0], b[1] - q[1])
        n1, n2 = math.hypot(*v1), math.hypot(*v2)
        if n1 == 0 or n2 == 0:
            angle = float('nan')          # coincident neighbours: the reference's arccos of a NaN, which fails the comparison
        else:
            angle = math.acos(min(1.0, max(-1.0, (v1[0] / n1) * (v2[0] / n2) + (v1[1] / n1) * (v2[1] / n2))))
        angles.append(angle)
        if angle < 2 * math.pi / 3:
            kept.append(q)
    return kept, angles


def test_draw_polygon_corner_filter():
    redraws = removed = 0
    for d in lists_of('draw_polygon'):
        (r,) = d['records']
        p = np.array(r['geom'], np.int64).reshape(-1, 2)
        n = len(p)
        assert r['kind'] == ss.POLYGON and 3 <= n <= 8 and r['n'] == n and (d['points'] == p).all()
        assert (p[:, 0] >= 0).all() and (p[:, 0] < W).all() and (p[:, 1] >= 0).all() and (p[:, 1] < H).all()
        # the corners before the filter, every draw of this key: the emitted polygon is the filter of the LAST draw, in one pass (the
        # reference's), every earlier draw was thrown away because fewer than 3 corners remained, and the last one kept at least 3
        attempts = r['attempts']
        assert len(attempts) >= 1 and all(3 <= len(a) <= 8 for a in attempts)
        for a in attempts[:-1]:
            assert len(corner_filter_by_hand(a)[0]) < 3
        kept, angles = corner_filter_by_hand(attempts[-1])
        assert [list(q) for q in kept] == p.tolist() and len(kept) >= 3
        assert sum(ang < 2 * math.pi / 3 for ang in angles) == n          # every kept corner's angle with its pre-filter neighbours is below 2 pi / 3 ...
        removed += len(attempts[-1]) - n                                  # ... and the others went (distance or angle)
        assert np.array_equal(ss.filter_corners(np.array(attempts[-1], np.int64)), p)
        redraws += len(attempts) - 1
    assert redraws > 0 and removed > 0          # both branches ran on these keys: a sampler that stopped filtering or re-drawing fails above
    print(f"draw_polygon: {redraws} re-draws and {removed} removed corners over {N_KEYS} keys")
    # the filter itself, on corners written out: a repeated corner and a flat one go
    sq = np.array([[0, 0], [10, 0], [10, 0], [10, 10], [5, 10], [0, 10]], np.int64)
    assert ss.filter_corners(sq).tolist() == [[0, 0], [10, 0], [10, 10], [0, 10]]          # the repeated (10, 0) is too close, (5, 10) is flat
    kept = ss.filter_corners(np.array([[0, 0], [10, 0], [10, 10], [0, 10]], np.int64))
    assert len(kept) == 4


def test_draw_ellipses_separation_and_no_keypoints():
    for d in lists_of('draw_ellipses'):
        assert len(d['points']) == 0 and len(d['keypoints']) == 0
        es = records(d, ss.ELLIPSE)
        assert 1 <= len(es) <= 20 and len(es) == len(d['records'])
        centres, rads = [], []
        for r in es:
            cx, cy, ax, ay = r['geom']
            mr = max(ax, ay)
            assert int(24 / 5) <= ax <= 24 and int(24 / 5) <= ay <= 24 and mr <= cx <= W - mr and mr <= cy <= H - mr
            for c, q in zip(centres, rads):
                assert not mr > math.hypot(c[0] - cx, c[1] - cy) - q          # the reference's inequality
            centres.append((cx, cy)); rads.append(mr)
            co, si = r['cs']
            assert abs(co * co + si * si - 1) < 1e-12 and co >= 0 and si >= 0          # angle in [0, 90)


def test_draw_star():
    for d in lists_of('draw_star'):
        segs = records(d, ss.SEGMENT)
        assert 3 <= len(segs) <= 6 and len(d['points']) == len(segs) + 1
        assert all(r['geom'][0:2] == segs[0]['geom'][0:2] and r['n'] == segs[0]['n'] == 1 for r in segs)


def test_checkerboard_and_stripes_keypoints_inside():
    for d in lists_of('draw_checkerboard'):
        cells, lines = records(d, ss.POLYGON), records(d, ss.SEGMENT)
        assert 9 <= len(cells) <= 49 and 4 <= len(lines) <= 18 and all(c['n'] == 4 for c in cells)
        assert cells[0]['rule'][0] == ss.RULE_CONTRAST and all(c['rule'][0] == ss.RULE_DIFFERENT and len(c['rule'][5]) == 21 for c in cells[1:])
        p = d['points']
        assert len(p) <= 64 and (p[:, 0] >= 0).all() and (p[:, 0] < W).all() and (p[:, 1] >= 0).all() and (p[:, 1] < H).all()
    for d in lists_of('draw_stripes'):
        assert d['records'][0]['kind'] == ss.NOP and d['records'][0]['rule'][0] == ss.RULE_CONTRAST
        stripes, lines = records(d, ss.POLYGON), records(d, ss.SEGMENT)
        assert 1 <= len(stripes) <= 13 and 4 <= len(lines) <= 5 + len(stripes) + 2
        for i, s in enumerate(stripes):
            kind, _, delta, r0, _, _ = s['rule']
            assert kind == ss.RULE_REL and r0 == i and 0.4 <= delta < 0.6
        p = d['points']
        assert (p[:, 0] >= 0).all() and (p[:, 0] < W).all() and (p[:, 1] >= 0).all() and (p[:, 1] < H).all()


def test_cube_and_noise():
    for d in lists_of('draw_cube'):
        assert len(d['points']) <= 7 and len(records(d, ss.POLYGON)) == 3 and len(records(d, ss.SEGMENT)) == 12
        for r in d['records'][3:]:
            assert r['rule'][0] == ss.RULE_REL and r['rule'][3] == 0 and 0.25 <= r['rule'][2] < 0.75
    for d in lists_of('gaussian_noise'):
        assert len(d['points']) == 0 and len(d['keypoints']) == 0 and [r['kind'] for r in d['records']] == [ss.NOISE]


def test_all_means_the_eight_and_multiple_polygons_is_refused():
    seen = {d['primitive'] for d in ss.sample_draw_lists(config('all'), range(120), 3)}
    assert seen == set(ss.IMPLEMENTED)
    with pytest.raises(NotImplementedError, match="draw_multiple_polygons"):
        ss.sample_draw_lists(config(['draw_multiple_polygons']), [0], 0)
    with pytest.raises(NotImplementedError, match="draw_multiple_polygons"):
        ss.SyntheticShapes(config(['draw_lines', 'draw_multiple_polygons']))


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == 'records':
            assert len(a[k]) == len(b[k])
            for x, y in zip(a[k], b[k]):
                assert x == y
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_determinism_independence_and_forced_flag():
    c = config('all')
    one = ss.sample_draw_lists(c, [3], 11)[0]
    _same(one, ss.sample_draw_lists(c, [3], 11)[0])
    _same(one, ss.sample_draw_lists(c, [0, 9, 3, 4, 1], 11)[2])
    other = ss.sample_draw_lists(c, [3], 12)[0]
    assert other['threshold'] != one['threshold']
    flags = [d['is_optical'] for d in ss.sample_draw_lists(c, range(40), 0)]
    assert any(flags) and not all(flags)
    assert not any(d['is_optical'] for d in ss.sample_draw_lists(c, range(40), 0, is_optical=False))
    assert all(d['is_optical'] for d in ss.sample_draw_lists(c, range(40), 0, is_optical=True))
    forced = ss.sample_draw_lists(c, [3], 11, is_optical=not one['is_optical'])[0]
    assert forced['records'] == one['records']          # forcing the flag changes nothing else


def hand_list(records, points=()):
    return {'index': 0, 'primitive': 'hand', 'is_optical': True, 'threshold': np.float32(0.5), 'blobs': [], 'blob_raw': [], 'bg_ksize': 1,
            'records': records, 'keypoints': np.asarray(points, np.int64).reshape(-1, 2)}


def mask_of(rows):
    return np.array([[ch == '#' for ch in row] for row in rows])


def test_restatement_masks_written_out():
    t = ss.pack_draw_lists([hand_list([ss.make_record(ss.POLYGON, [1, 1, 5, 1, 1, 5], 3)])], (7, 7))
    assert np.array_equal(ref.coverage(t, 0, 7, 7) == 0, mask_of([".......",
                                                                  ".#####.",
                                                                  ".####..",
                                                                  ".###...",
                                                                  ".##....",
                                                                  ".#.....",
                                                                  "......."]))
    t = ss.pack_draw_lists([hand_list([ss.make_record(ss.CIRCLE, [3, 2], 0)])], (5, 6))
    assert np.argwhere(ref.coverage(t, 0, 5, 6) == 0).tolist() == [[2, 3]]
    t = ss.pack_draw_lists([hand_list([ss.make_record(ss.SEGMENT, [1, 3, 5, 3], 3)])], (7, 8))
    assert np.array_equal(ref.coverage(t, 0, 7, 8) == 0, mask_of(["........",
                                                                  "........",
                                                                  "#######.",
                                                                  "#######.",
                                                                  "#######.",
                                                                  "........",
                                                                  "........"]))
    t = ss.pack_draw_lists([hand_list([ss.make_record(ss.ELLIPSE, [4, 3, 3, 1], 0, angle_cos_sin=(1.0, 0.0))])], (7, 9))
    assert np.array_equal(ref.coverage(t, 0, 7, 9) == 0, mask_of([".........",
                                                                  ".........",
                                                                  "....#....",
                                                                  ".#######.",
                                                                  "....#....",
                                                                  ".........",
                                                                  "........."]))
    # painter's order: the later record wins where both cover
    t = ss.pack_draw_lists([hand_list([ss.make_record(ss.CIRCLE, [2, 2], 2), ss.make_record(ss.CIRCLE, [2, 2], 1)])], (5, 5))
    cov = ref.coverage(t, 0, 5, 5)
    assert (cov == 1).sum() == 5 and (cov == 0).sum() == 8 and cov[2, 2] == 1 and cov[0, 2] == 0 and cov[0, 0] == -1


def test_restatement_colour_chains_by_hand():
    diff1 = [0.9, 0.99, 0.3] + [0.5] * 18
    diff2 = [0.35, 0.15] + [0.5] * 19
    diff3 = [0.95] * 20 + [0.96]
    recs = [ss.make_record(ss.NOP, rule=ss.rule_contrast(0.45, 0.1)),                  # |0.45 - 0.5| < 0.1: (0.45 + 0.5) % 1
            ss.make_record(ss.NOP, rule=ss.rule_different(diff1, 0.1, 0)),             # 0.9 and 0.99 are near 0.95
            ss.make_record(ss.NOP, rule=ss.rule_different(diff2, 0.1, 0, 1)),          # 0.35 is near 0.3
            ss.make_record(ss.NOP, rule=ss.rule_different(diff3, 0.1, 0)),             # nothing contrasts: the last drawn
            ss.make_record(ss.NOP, rule=ss.rule_rel(1, 0.8)),
            ss.make_record(ss.NOP, rule=ss.rule_rel(4, 0.45)),
            ss.make_record(ss.NOP, rule=ss.rule_contrast(0.7, 0.1)),
            ss.make_record(ss.NOP, rule=ss.rule_abs(0.25))]
    t = ss.pack_draw_lists([hand_list(recs)], (4, 4))
    c = ref.resolve_colours(t, 0, 0.5)
    assert c.tolist() == [(0.45 + 0.5) % 1.0, 0.3, 0.15, 0.96, (0.3 + 0.8) % 1.0, ((0.3 + 0.8) % 1.0 + 0.45) % 1.0, 0.7, 0.25]
    assert abs(c[4] - 0.1) < 1e-12 and abs(c[5] - 0.55) < 1e-12
    with pytest.raises(ValueError, match="earlier"):
        ss.pack_draw_lists([hand_list([ss.make_record(ss.NOP, rule=ss.rule_rel(0, 0.1))])], (4, 4))


def test_restatement_filters():
    assert ref.reflect101(np.arange(-5, 9), 4).tolist() == [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    img = np.arange(12, dtype=np.float64).reshape(3, 4)
    b = ref.box_blur(img, 3)
    assert abs(b[1, 1] - img[0:3, 0:3].mean()) < 1e-12 and abs(b[0, 0] - img[[1, 0, 1]][:, [1, 0, 1]].mean()) < 1e-12
    e = ref.box_blur(img, 2)          # even: anchor 1, the window is [x - 1, x]
    assert abs(e[1, 2] - img[0:2, 1:3].mean()) < 1e-12
    assert np.allclose(ref.box_blur(np.full((5, 6), 0.3), 15), 0.3, atol=1e-15)          # a window wider than the frame
    assert np.allclose(ref.gaussian_blur(np.full((6, 5), 0.7), 21), 0.7, atol=1e-15)
    r = ref.resize_linear(np.arange(8, dtype=np.float64)[None].repeat(2, 0), 1, 2)      # 4:1, taps 1.5 and 5.5
    assert np.allclose(r, [[1.5, 5.5]])


def test_synth_symbols_declared_and_exported():
    lib = _lib.load()
    declared = _lib.exported_symbols()
    for n in SYMBOLS:
        assert n in declared and n in _lib._SIGNATURES and hasattr(lib, n), n


def test_synth_argument_errors_name_the_argument():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))           # never dereferenced: every call below fails its checks before any launch

    def err(rc):
        assert rc != 0
        return lib.xp_last_error().decode()
    assert "n_blobs" in err(lib.xp_synth_background(p, 0, p, p, p, p, 257, 0.1, p, p, 1, 8, 8, None))
    assert "min_contrast" in err(lib.xp_synth_background(p, 0, p, p, p, p, 4, -0.1, p, p, 1, 8, 8, None))
    assert "W must" in err(lib.xp_synth_background(p, 0, p, p, p, p, 4, 0.1, p, p, 1, 8, 4097, None))
    assert "H must" in err(lib.xp_synth_background(p, 0, p, p, p, p, 4, 0.1, p, p, 1, 0, 8, None))
    assert "B must" in err(lib.xp_synth_background(p, 0, p, p, p, p, 4, 0.1, p, p, 0, 8, 8, None))
    names = {0: "frame", 2: "sample_ids", 3: "thresholds", 4: "blob_geom", 5: "blob_raw", 8: "count_ws", 9: "field_mean"}
    for i, name in names.items():
        a = [p, 0, p, p, p, p, 4, 0.1, p, p, 1, 8, 8, None]
        a[i] = None
        msg = err(lib.xp_synth_background(*a))
        assert "null pointer" in msg and msg.rstrip().endswith(name), msg
    for i, name in enumerate(("src", "tmp", "dst", "ksizes")):
        a = [p, ctypes.c_void_p(p.value + 8), ctypes.c_void_p(p.value + 16), p, 1, 8, 8, None]
        a[i] = None
        msg = err(lib.xp_synth_box_blur(*a))
        assert msg.rstrip().endswith(name), msg
    assert "tmp" in err(lib.xp_synth_box_blur(p, p, p, p, 1, 8, 8, None))
    assert "n_records" in err(lib.xp_synth_resolve_colours(p, p, p, p, 129, 0, p, p, p, 1, 8, 8, None))
    assert "n_candidates" in err(lib.xp_synth_resolve_colours(p, p, p, p, 4, -1, p, p, p, 1, 8, 8, None))
    assert err(lib.xp_synth_resolve_colours(p, p, p, None, 4, 21, p, p, p, 1, 8, 8, None)).rstrip().endswith("candidates")
    assert err(lib.xp_synth_resolve_colours(p, None, p, p, 4, 21, p, p, p, 1, 8, 8, None)).rstrip().endswith("rules")
    assert "n_records" in err(lib.xp_synth_rasterise(p, p, p, 0, p, 0, 1, 8, 8, None))
    assert err(lib.xp_synth_rasterise(p, None, p, 0, p, 4, 1, 8, 8, None)).rstrip().endswith("records")
    assert "h must" in err(lib.xp_synth_resize(p, ctypes.c_void_p(p.value + 8), 1, 8, 8, 0, 4, None))
    assert "w must" in err(lib.xp_synth_resize(p, ctypes.c_void_p(p.value + 8), 1, 8, 8, 4, 5000, None))
    assert "in-place" in err(lib.xp_synth_resize(p, p, 1, 8, 8, 4, 4, None))
    assert err(lib.xp_synth_resize(p, None, 1, 8, 8, 4, 4, None)).rstrip().endswith("dst")
    odd = ctypes.c_void_p(p.value + 4)                  # 4 mod 8
    assert err(lib.xp_synth_background(p, 0, p, p, p, odd, 4, 0.1, p, p, 1, 8, 8, None)).rstrip().endswith("blob_raw")
    for i, name in ((2, "rule_values"), (3, "candidates"), (6, "partial_ws"), (8, "bg_mean")):
        a = [p, p, p, p, 4, 21, p, p, p, 1, 8, 8, None]
        a[i] = odd
        msg = err(lib.xp_synth_resolve_colours(*a))
        assert "misaligned" in msg and msg.rstrip().endswith(name), msg
    assert err(lib.xp_synth_rasterise(p, odd, p, 0, p, 4, 1, 8, 8, None)).rstrip().endswith("records")
    assert "h must" in err(lib.xp_synth_scatter_points(p, p, 4, p, 1, 0, 8, None))
    assert "w must" in err(lib.xp_synth_scatter_points(p, p, 4, p, 1, 8, 4097, None))
    assert "cap" in err(lib.xp_synth_scatter_points(p, p, 0, p, 1, 8, 8, None))
    assert err(lib.xp_synth_scatter_points(p, None, 4, p, 1, 8, 8, None)).rstrip().endswith("counts")


def test_dataset_refusals_and_config():
    with pytest.raises(NotImplementedError, match="on-the-fly"):
        ss.SyntheticShapes(config(**{'on-the-fly': False, 'hdf5-file': 'x.hdf5'}))
    with pytest.raises(NotImplementedError, match="keypoints_as_map"):
        ss.SyntheticShapes(config(keypoints_as_map=False))
    ds = ss.SyntheticShapes(config(length=17))
    assert len(ds) == 17 and ds.returns_pair() is False and ds.primitives == ss.IMPLEMENTED
    with pytest.raises(_lib.XPointHipError, match="GPU"):
        ds.load_batch([0, 1], "cpu")
    # Gaussian sizes: `processing` wins over the YAML's `preprocessing`, which wins over the defaults
    assert ss.SyntheticShapes(config()).config['processing'] == {'blur_size': 21, 'additional_ir_blur': True, 'additional_ir_blur_size': 51}
    c = ss.SyntheticShapes(config(preprocessing={'blur_size': 11, 'additional_ir_blur_size': 31})).config['processing']
    assert c['blur_size'] == 11 and c['additional_ir_blur_size'] == 31
    c = ss.SyntheticShapes(config(preprocessing={'blur_size': 11, 'additional_ir_blur_size': 31}, processing={'blur_size': 5})).config['processing']
    assert c['blur_size'] == 5 and c['additional_ir_blur_size'] == 31
    # the homographies are keyed like the draw lists and leave the process-wide generators alone
    state = np.random.get_state()[1].copy()
    h1 = ds.homographies([4, 5], seed=2)
    assert np.array_equal(np.random.get_state()[1], state)
    assert np.array_equal(h1[1], ds.homographies([5], seed=2)[0]) and not np.array_equal(h1[0], h1[1])
