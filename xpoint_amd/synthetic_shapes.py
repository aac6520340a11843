"""SyntheticShapes on the GPU: the detector's pretraining data (reference xpoint/datasets/SyntheticShapes.py,
xpoint/utils/draw_primitives.py, configs/config_synthetic_shapes.yaml).

The reference renders every sample on the host with OpenCV.  Here the host only SAMPLES: `sample_draw_lists` restates the sampling logic of
generate_background and of the primitives (counts, radii, thickness ranges, the polygon corner filter, the segment-intersection and ellipse
separation rejections, the affine + perspective warp of the checkerboard and stripe grids, the cube's transform and faces,
keep_points_inside) and emits, per image, the keypoints and a draw list of fixed-size records.  It draws nothing.  `render` executes the
lists on the device (csrc/synth_shapes.hip): background, box blur, colour resolve, rasteriser, Gaussian finish, resize, label scatter; a
batch is a fixed sequence of launches whatever its size; every table is uploaded before the first launch and nothing is read back, so the host
never waits for the batch's own kernels.

A record carries a colour RULE, not a colour, because the reference picks colours against np.mean(img), which exists only on the device:
  ABS(v); CONTRAST(raw, min_contrast) against the background's mean; DIFFERENT(21 candidates, up to two earlier records) =
  get_different_color; REL(earlier record, delta) = (c + delta) % 1 (the stripes' chain, the cube's edges).
The device resolves them in order, one thread per image.

Randomness: every draw of sample `index` comes from numpy.random.default_rng([seed, index]); the noise fields come from the Philox
generator of the augmentation kernels keyed by (seed, index).  A sample never depends on its batch neighbours, and the same (seed, index)
gives the same list on any machine.

Stated differences from the reference:
  * the draw order of the reference's two process-wide generators (random, np.random) is not reproduced: OpenCV is absent, so it could
    not be pinned against anything;
  * where the reference takes the running np.mean(img) between shapes (draw_lines, draw_polygon, draw_ellipses), the mean of the finished
    background is used;
  * a thick segment is the set of pixels within thickness / 2 of the segment; polygon fill is even-odd with the boundary included;
    ellipses are the analytic inside test (as additive_shade's); no pixel parity with OpenCV's rasterisers is claimed;
  * the checkerboard keeps its neighbours' colours in f64 (the reference rounds them to float16 before comparing);
  * warped grid points are clamped to +-16383 (the rasteriser's 64-bit tests are exact inside that range);
  * images are f32 from the first pixel (the reference carries float64 until the end);
  * `draw_multiple_polygons` (textured polygons) is opt-in: without the dataset key `textured_polygons: true` asking for it raises
    NotImplementedError and 'all' means the other eight primitives; with the key, 'all' means the nine.  Its polygons are filled with a
    procedural texture, 3 000 random discs under a box blur, that is never stored as a list: the device draws the discs from the Philox
    generator (slot KEY_TEXTURE) and blurs each texture only where its polygon needs it (`render`, `_multiple_polygons`);
  * the reference takes draw_multiple_polygons' background colour as int(np.mean(img)), which is 0 for an image in [0, 1): every colour of a
    texture is get_random_color(0, min_contrast), raw shifted by 0.5 where raw < min_contrast, whatever the image holds.  Kept: no texture
    colour depends on the device's mean.  The primitive reads its own min_contrast (0.13), not generation.min_contrast, as there.

Gaussian sizes: the reference reads config['processing'] only, while its shipped YAML writes `preprocessing`, which is therefore silently
ignored there.  Here both are accepted: a `processing` key given by the caller wins, then `preprocessing`, then the defaults (21, 51)."""
from __future__ import annotations

import copy
import ctypes
import math
import random as _random

import numpy as np

from . import _lib
from . import homographies as _hom
from .utils import dict_update

NOP, CIRCLE, SEGMENT, POLYGON, ELLIPSE, NOISE, TEXTURED = range(7)          # XP_SYNTH_* record kinds
RULE_ABS, RULE_CONTRAST, RULE_DIFFERENT, RULE_REL = range(4)      # XP_SYNTH_RULE_*
RECORD_INTS, MAX_RECORDS, CANDIDATES, COORD_MAX = 24, 128, 21, 16383
KEY_BACKGROUND, KEY_NOISE, KEY_TEXTURE = 6, 7, 8                  # Philox primitive slots (the photometric primitives hold 0..5)
MAX_TEXTURE_BLOBS, MAX_KSIZE, JOB_INTS = 4096, 500, 16            # XP_SYNTH_MAX_TEXTURE_BLOBS, _MAX_KSIZE, _JOB_INTS

ALL_PRIMITIVES = ['draw_lines', 'draw_polygon', 'draw_multiple_polygons', 'draw_ellipses', 'draw_star', 'draw_checkerboard', 'draw_stripes',
                  'draw_cube', 'gaussian_noise']
IMPLEMENTED = [p for p in ALL_PRIMITIVES if p != 'draw_multiple_polygons']

DEFAULT_CONFIG = {
    'length': 1000, 'primitives': 'all', 'textured_polygons': False, 'on-the-fly': True, 'hdf5-file': None,
    'generation_size': [960, 1280], 'image_size': [240, 320], 'keypoints_as_map': True,
    'generation': {
        'min_contrast': 0.1,
        'generate_background': {'min_kernel_size': 150, 'max_kernel_size': 500, 'min_rad_ratio': 0.02, 'max_rad_ratio': 0.031},
        'draw_lines': {'nb_lines': 10}, 'draw_polygons': {'max_sides': 8}, 'draw_stripes': {'transform_params': (0.1, 0.1)},
        'draw_multiple_polygons': {'kernel_boundaries': (50, 100)}},
    'processing': {'blur_size': 21, 'additional_ir_blur': True, 'additional_ir_blur_size': 51},
    'augmentation': {
        'photometric': {'enable': True, 'primitives': 'all', 'params': {}, 'random_order': True},
        'homographic': {'enable': True, 'params': {}, 'border_reflect': True, 'valid_border_margin': 0, 'mask_border': True}},
}


def merge_config(config):
    """The reference's defaults updated by `config`; `preprocessing` fills the Gaussian sizes that `processing` does not give."""
    cfg = dict_update(copy.deepcopy(DEFAULT_CONFIG), copy.deepcopy(dict(config or {})))
    given = dict((config or {}).get('processing', {}) or {})
    for k, v in dict((config or {}).get('preprocessing', {}) or {}).items():
        if k in DEFAULT_CONFIG['processing'] and k not in given:
            cfg['processing'][k] = v
    return cfg


def parse_primitives(names, textured_polygons=False):
    """'all' = the eight primitives of IMPLEMENTED, or the nine of ALL_PRIMITIVES with textured_polygons; a name or a list of names otherwise.
    Without textured_polygons the name draw_multiple_polygons raises NotImplementedError."""
    if names == 'all':
        return list(ALL_PRIMITIVES if textured_polygons else IMPLEMENTED)
    p = list(names) if isinstance(names, (list, tuple)) else [names]
    if 'draw_multiple_polygons' in p and not textured_polygons:
        raise NotImplementedError("SyntheticShapes: the primitive 'draw_multiple_polygons' (textured polygons) is not implemented; "
                                  "'all' selects the other eight (the dataset key textured_polygons: true turns it on)")
    if not p or not set(p) <= set(ALL_PRIMITIVES):
        raise ValueError(f"SyntheticShapes: unknown primitives {sorted(set(p) - set(ALL_PRIMITIVES))}")
    return p


# ------------------------------------------------------------------------------------------------ records and rules (host)
def rule_abs(v):
    return (RULE_ABS, float(v), 0.0, -1, -1, None)


def rule_contrast(raw, min_contrast):
    return (RULE_CONTRAST, float(raw), float(min_contrast), -1, -1, None)


def rule_different(candidates, min_contrast, ref0=-1, ref1=-1):
    c = [float(v) for v in candidates]
    if len(c) != CANDIDATES:
        raise ValueError(f"rule_different: {CANDIDATES} candidates are needed, got {len(c)}")
    return (RULE_DIFFERENT, 0.0, float(min_contrast), int(ref0), int(ref1), c)


def rule_rel(ref, delta):
    return (RULE_REL, 0.0, float(delta), int(ref), -1, None)


def _clampi(v):
    return int(min(max(int(v), -COORD_MAX), COORD_MAX))


def make_record(kind, geom=(), n=0, rule=None, angle_cos_sin=None):
    """One draw-list record: kind, integer geometry (circle cx cy; segment x1 y1 x2 y2; polygon x0 y0 x1 y1 ...; ellipse cx cy ax ay), n =
    radius / thickness / vertex count, the colour rule, and for an ellipse (cos, sin) of its angle as f64."""
    g = [_clampi(v) for v in geom]
    if kind in (POLYGON, TEXTURED) and (n != len(g) // 2 or not 1 <= n <= 8):
        raise ValueError(f"make_record: a polygon holds 1..8 vertices, got n = {n} with {len(g)} coordinates")
    return {'kind': int(kind), 'geom': g, 'n': int(n), 'rule': rule or rule_abs(0.0), 'cs': angle_cos_sin}


def _bbox(rec, H, W):
    k, g, n = rec['kind'], rec['geom'], rec['n']
    if k == CIRCLE:
        x0, y0, x1, y1 = g[0] - n, g[1] - n, g[0] + n, g[1] + n
    elif k == SEGMENT:
        pad = n // 2 + 1
        x0, y0, x1, y1 = min(g[0], g[2]) - pad, min(g[1], g[3]) - pad, max(g[0], g[2]) + pad, max(g[1], g[3]) + pad
    elif k in (POLYGON, TEXTURED):
        x0, y0, x1, y1 = min(g[0::2]), min(g[1::2]), max(g[0::2]), max(g[1::2])
    elif k == ELLIPSE:
        r = max(g[2], g[3]) + 1
        x0, y0, x1, y1 = g[0] - r, g[1] - r, g[0] + r, g[1] + r
    else:
        x0, y0, x1, y1 = 0, 0, W - 1, H - 1
    return max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)


def pack_draw_lists(lists, generation_size):
    """The device tables of B draw lists (`sample_draw_lists`, or hand-made dicts with 'records', 'keypoints', 'threshold', 'blobs',
    'blob_raw', 'bg_ksize', 'is_optical', 'index'): numpy arrays in the layouts of include/xpoint_hip.h (xp_synth_*).  An optional
    tables['min_contrast'] is the background blobs' (default 0.13, generate_background's own).  A TEXTURED record (a polygon record with
    'ksize', 'ordinal' and, optionally, 'nb_blobs' (3000) and 'min_contrast' (0.13)) puts its blur size and ordinal into words 22 and 23; the
    textures of one batch share nb_blobs and min_contrast: tables['texture_blobs'], tables['texture_min_contrast']."""
    H, W = int(generation_size[0]), int(generation_size[1])
    B = len(lists)
    R = max(1, max(len(d['records']) for d in lists))
    if R > MAX_RECORDS:
        raise ValueError(f"pack_draw_lists: a draw list holds at most {MAX_RECORDS} records, got {R}")
    nb = {len(d['blobs']) for d in lists}
    if len(nb) != 1:
        raise ValueError("pack_draw_lists: every image of a batch carries the same number of background blobs")
    NB = nb.pop()
    NC = max(1, max(sum(CANDIDATES for r in d['records'] if r['rule'][0] == RULE_DIFFERENT) for d in lists))
    P = max(1, max(len(d['keypoints']) for d in lists))
    t = {'records': np.zeros((B, R, RECORD_INTS), np.int32), 'rules': np.full((B, R, 4), -1, np.int32), 'rule_values': np.zeros((B, R, 2)),
         'candidates': np.zeros((B, NC)), 'points': np.zeros((B, P, 2), np.int32), 'counts': np.zeros(B, np.int32),
         'thresholds': np.zeros(B, np.float32), 'blob_geom': np.zeros((B, max(NB, 1), 4), np.int32), 'blob_raw': np.zeros((B, max(NB, 1))),
         'bg_ksize': np.zeros(B, np.int32), 'is_optical': np.zeros(B, bool), 'ids': np.zeros(B, np.int32), 'n_blobs': NB}
    t['rules'][:, :, 0] = RULE_ABS
    texture = set()
    for b, d in enumerate(lists):
        off = 0
        for r, rec in enumerate(d['records']):
            row = t['records'][b, r]
            row[0] = rec['kind']
            row[1:5] = _bbox(rec, H, W)
            row[5] = rec['n']
            g = rec['geom']
            row[6:6 + len(g)] = g
            if rec['kind'] == ELLIPSE:
                row[10:14] = np.array(rec['cs'], np.float64).view(np.int32)
            if rec['kind'] == TEXTURED:
                if not 1 <= int(rec['ksize']) <= MAX_KSIZE:
                    raise ValueError(f"pack_draw_lists: a textured polygon's ksize must be in [1, {MAX_KSIZE}], got {rec['ksize']}")
                row[22:24] = (rec['ksize'], rec['ordinal'])
                texture.add((int(rec.get('nb_blobs', 3000)), float(rec.get('min_contrast', 0.13))))
            kind, v, m, r0, r1, cands = rec['rule']
            if (r0 >= r) or (r1 >= r):
                raise ValueError("pack_draw_lists: a colour rule refers to earlier records only")
            t['rules'][b, r] = (kind, r0, r1, off if cands else -1)
            t['rule_values'][b, r] = (v, m)
            if cands:
                t['candidates'][b, off:off + CANDIDATES] = cands
                off += CANDIDATES
        kp = np.asarray(d['keypoints'], np.int64).reshape(-1, 2)
        t['points'][b, :len(kp)] = kp
        t['counts'][b] = len(kp)
        t['thresholds'][b] = d['threshold']
        if NB:
            t['blob_geom'][b, :, :3] = np.asarray(d['blobs'], np.int64).reshape(NB, 3)
            t['blob_raw'][b] = d['blob_raw']
        t['bg_ksize'][b] = d['bg_ksize']
        t['is_optical'][b] = d['is_optical']
        t['ids'][b] = d['index']
    if len(texture) > 1:
        raise ValueError(f"pack_draw_lists: the textured polygons of a batch share nb_blobs and min_contrast, got {sorted(texture)}")
    if texture:
        t['texture_blobs'], t['texture_min_contrast'] = texture.pop()
        if not 0 <= t['texture_blobs'] <= MAX_TEXTURE_BLOBS:
            raise ValueError(f"pack_draw_lists: nb_blobs must be in [0, {MAX_TEXTURE_BLOBS}], got {t['texture_blobs']}")
    return t


# ------------------------------------------------------------------------------------------------ the sampler
class _Draw:
    """The draws of one sample, from one numpy Generator."""

    def __init__(self, rng):
        self.rng = rng

    def u(self):
        return float(self.rng.random())

    def ri(self, lo, hi):          # random.randint: both ends included
        return int(self.rng.integers(int(lo), int(hi) + 1))

    def nr(self, lo, hi):          # np.random.randint: hi excluded
        lo, hi = int(lo), int(hi)
        return int(self.rng.integers(lo, max(hi, lo + 1)))


def _ccw(a, b, c):
    return (c[1] - a[1]) * (b[0] - a[0]) > (b[1] - a[1]) * (c[0] - a[0])


def segments_intersect(a, b, c, d):
    """draw_primitives.intersect for one pair of segments ab, cd (integer points)"""
    return _ccw(a, c, d) != _ccw(b, c, d) and _ccw(a, b, c) != _ccw(a, b, d)


def _angle(v1, v2):
    with np.errstate(all='ignore'):
        a, b = v1 / np.linalg.norm(v1), v2 / np.linalg.norm(v2)
        return np.arccos(np.clip(np.dot(a, b), -1.0, 1.0))


def filter_corners(points):
    """The polygon corner filter: drop corners closer than 0.01 to their predecessor, then corners flatter than 2 pi / 3."""
    n = len(points)
    norms = np.array([np.linalg.norm(points[(i - 1) % n] - points[i]) for i in range(n)])
    points = points[norms > 0.01]
    n = len(points)
    if n == 0:
        return points
    ang = np.array([_angle(points[(i - 1) % n] - points[i], points[(i + 1) % n] - points[i]) for i in range(n)])
    return points[ang < 2 * math.pi / 3]          # a NaN angle (coincident corners) fails the comparison, as in the reference


def _sample_background(d, H, W, gb):
    dim = max(H, W)
    nb = int(gb.get('nb_blobs', 100))
    thr = d.u()
    cx = [d.nr(0, W) for _ in range(nb)]
    cy = [d.nr(0, H) for _ in range(nb)]
    raw, blobs = [], []
    lo, hi = int(dim * gb.get('min_rad_ratio', 0.01)), int(dim * gb.get('max_rad_ratio', 0.05))
    for i in range(nb):
        raw.append(d.u())
        blobs.append((cx[i], cy[i], d.ri(lo, max(hi, lo))))
    ks = d.ri(gb.get('min_kernel_size', 50), gb.get('max_kernel_size', 300))
    return thr, blobs, raw, ks


def _thickness(d, min_dim, lo, hi):
    a = int(math.ceil(min_dim * lo))
    return d.ri(a, max(int(min_dim * hi), a))


def _lines(d, H, W, mc, nb_lines=10):
    recs, segs, pts = [], [], []
    for _ in range(d.ri(1, nb_lines)):
        p1, p2 = (d.nr(0, W), d.nr(0, H)), (d.nr(0, W), d.nr(0, H))
        if any(segments_intersect(s[0], s[1], p1, p2) for s in segs):
            continue
        segs.append((p1, p2))
        raw = d.u()
        recs.append(make_record(SEGMENT, p1 + p2, _thickness(d, min(H, W), 0.01, 0.02), rule_contrast(raw, mc)))
        pts += [p1, p2]
    return recs, np.array(pts, np.int64).reshape(-1, 2)


def _polygon_points(d, H, W, max_sides, min_rad_frac, lo_frac, centre=None):
    """corners on a circle (before the filter), its centre and its radius; centre: the draw of a centre coordinate, d.ri unless given"""
    centre = centre or d.ri
    n = d.ri(3, max_sides)
    min_dim = min(H, W)
    rad = max(d.u() * min_dim / 2, min_dim / min_rad_frac)
    x, y = centre(int(rad), int(W - rad)), centre(int(rad), int(H - rad))
    sl = np.linspace(0, 2 * math.pi, n + 1)
    ang = [sl[i] + d.u() * (sl[i + 1] - sl[i]) for i in range(n)]
    return np.array([[int(x + max(d.u(), lo_frac) * rad * math.cos(a)), int(y + max(d.u(), lo_frac) * rad * math.sin(a))] for a in ang], np.int64), (x, y, rad)


def _polygon(d, H, W, mc, max_sides=8):
    if max_sides > 8:
        raise ValueError(f"draw_polygon: max_sides must be at most 8 (a polygon record holds 8 vertices), got {max_sides}")
    attempts = []                                 # the corners of every draw before the filter: the last one is the polygon's
    while True:                                   # the reference draws again when fewer than 3 corners remain
        pts, _ = _polygon_points(d, H, W, max_sides, 10, 0.4)
        attempts.append(pts.tolist())
        pts = filter_corners(pts)
        if len(pts) >= 3:
            break
    rec = make_record(POLYGON, pts.reshape(-1).tolist(), len(pts), rule_contrast(d.u(), mc))
    rec['attempts'] = attempts                    # kept for inspection (tests); `pack_draw_lists` does not read it
    return [rec], pts


def circles_nested(centre, rad, centres, rads):
    """draw_primitives.overlap: an accepted circle that contains, or lies inside, the circle (centre, rad)"""
    return any(math.hypot(centre[0] - c[0], centre[1] - c[1]) + min(rad, r) < max(rad, r) for c, r in zip(centres, rads))


def _multiple_polygons(d, H, W, mc, max_sides=8, nb_polygons=30, nb_blobs=3000, min_contrast=0.13, kernel_boundaries=(50, 100)):
    """draw_multiple_polygons: nb_polygons attempts, each accepted polygon one TEXTURED record; the keypoints are all their vertices.  The
    draws of one attempt, in this order: the corner count, the radius, the centre x, y (upper end excluded), the corners' angles, then per
    corner its two radial factors; the corner filter draws nothing; an attempt with fewer than 3 corners left, with an edge that intersects
    an accepted polygon's edge, or whose circle nests with an accepted circle ends there (no redraw); an accepted one then draws its
    blur size in [kernel_boundaries) and its base colour.  `mc` (generation.min_contrast) is not read: the textures use `min_contrast`."""
    if max_sides > 8:
        raise ValueError(f"draw_multiple_polygons: max_sides must be at most 8 (a polygon record holds 8 vertices), got {max_sides}")
    if not 0 <= int(nb_blobs) <= MAX_TEXTURE_BLOBS:
        raise ValueError(f"draw_multiple_polygons: nb_blobs must be in [0, {MAX_TEXTURE_BLOBS}], got {nb_blobs}")
    recs, edges, centres, rads, pts_all = [], [], [], [], []
    for _ in range(nb_polygons):
        pts, (x, y, rad) = _polygon_points(d, H, W, max_sides, 10, 0.4, centre=d.nr)
        if circles_nested((x, y), rad, centres, rads):          # none of the three rejections draws: their order is free, the cheapest first
            continue
        pts = filter_corners(pts)
        n = len(pts)
        if n < 3:
            continue
        new = [(tuple(pts[i]), tuple(pts[(i + 1) % n])) for i in range(n)]
        if any(segments_intersect(a, b, p, q) for a, b in edges for p, q in new):
            continue
        centres.append((x, y)); rads.append(rad)
        edges += new
        ksize, raw = d.nr(kernel_boundaries[0], kernel_boundaries[1]), d.u()
        rec = make_record(TEXTURED, pts.reshape(-1).tolist(), n, rule_abs((raw + 0.5) % 1.0 if raw < min_contrast else raw))
        rec.update(ksize=ksize, ordinal=len(recs), nb_blobs=int(nb_blobs), min_contrast=float(min_contrast), circle=(x, y, rad))
        recs.append(rec)
        pts_all.append(pts)
    return recs, np.concatenate(pts_all).astype(np.int64) if pts_all else np.zeros((0, 2), np.int64)


def ellipses_separated(max_rad, centre, centres, rads):
    """draw_ellipses' acceptance: no earlier ellipse with max_rad > |centre - c| - rad"""
    return not any(max_rad > math.sqrt((c[0] - centre[0]) ** 2 + (c[1] - centre[1]) ** 2) - r for c, r in zip(centres, rads))


def _ellipses(d, H, W, mc, nb_ellipses=20):
    recs, centres, rads = [], [], []
    min_dim = min(H, W) / 4
    for _ in range(nb_ellipses):
        ax, ay = int(max(d.u() * min_dim, min_dim / 5)), int(max(d.u() * min_dim, min_dim / 5))
        mr = max(ax, ay)
        c = (d.ri(mr, max(W - mr, mr)), d.ri(mr, max(H - mr, mr)))
        if not ellipses_separated(mr, c, centres, rads):
            continue
        centres.append(c); rads.append(mr)
        raw, ang = d.u(), math.radians(d.u() * 90)
        recs.append(make_record(ELLIPSE, c + (ax, ay), 0, rule_contrast(raw, mc), (math.cos(ang), math.sin(ang))))
    return recs, np.zeros((0, 2), np.int64)


def _star(d, H, W, mc, nb_branches=6):
    n = d.ri(3, nb_branches)
    min_dim = min(H, W)
    t = _thickness(d, min_dim, 0.01, 0.02)
    rad = max(d.u() * min_dim / 2, min_dim / 5)
    x, y = d.nr(int(rad), int(W - rad)), d.nr(int(rad), int(H - rad))
    sl = np.linspace(0, 2 * math.pi, n + 1)
    ang = [sl[i] + d.u() * (sl[i + 1] - sl[i]) for i in range(n)]
    pts = [[x, y]] + [[int(x + max(d.u(), 0.3) * rad * math.cos(a)), int(y + max(d.u(), 0.3) * rad * math.sin(a))] for a in ang]
    recs = [make_record(SEGMENT, pts[0] + pts[i], t, rule_contrast(d.u(), mc)) for i in range(1, n + 1)]
    return recs, np.array(pts, np.int64)


def affine_transform(src, dst):
    """cv2.getAffineTransform: the 2 x 3 map of three points src -> dst, a 6 x 6 solve in f64"""
    a, b = np.zeros((6, 6)), np.zeros(6)
    for i in range(3):
        a[2 * i, 0:3] = (src[i][0], src[i][1], 1.0)
        a[2 * i + 1, 3:6] = (src[i][0], src[i][1], 1.0)
        b[2 * i], b[2 * i + 1] = dst[i][0], dst[i][1]
    return np.linalg.solve(a, b).reshape(2, 3)


def _warp_grid(d, H, W, points, transform_params):
    """The checkerboard's / stripes' affine + perspective warp of integer grid points (x, y); truncation toward zero, clamped."""
    alpha = max(H, W) * (transform_params[0] + d.u() * transform_params[1])
    centre = np.float16([H, W]) // 2                      # the reference's (row, column) centre, used as (x, y): kept
    sq = min(H, W) // 3
    pts1 = np.float32([centre + sq, [centre[0] + sq, centre[1] - sq], centre - sq, [centre[0] - sq, centre[1] + sq]])
    pts2 = pts1 + d.rng.uniform(-alpha, alpha, size=(4, 2)).astype(np.float32)
    A = affine_transform(pts1[:3].astype(np.float64), pts2[:3].astype(np.float64))
    pts2 = pts1 + d.rng.uniform(-alpha / 2, alpha / 2, size=(4, 2)).astype(np.float32)
    P = _hom.get_perspective_transform(pts1, pts2)
    hom = np.concatenate([np.asarray(points, np.float64), np.ones((len(points), 1))], 1)
    wp = hom @ A.T
    with np.errstate(all='ignore'):
        den = wp @ P[2, :2] + P[2, 2]
        out = np.stack([(wp @ P[0, :2] + P[0, 2]) / den, (wp @ P[1, :2] + P[1, 2]) / den], 1)
    out = np.nan_to_num(out, nan=0.0, posinf=COORD_MAX, neginf=-COORD_MAX)
    return np.clip(np.trunc(out), -COORD_MAX, COORD_MAX).astype(np.int64)


def keep_points_inside(points, H, W):
    m = (points[:, 0] >= 0) & (points[:, 0] < W) & (points[:, 1] >= 0) & (points[:, 1] < H)
    return points[m]


def _quad(wp, idx):
    return [int(v) for i in idx for v in wp[i]]


def _checkerboard(d, H, W, mc, max_rows=7, max_cols=7, transform_params=(0.05, 0.15)):
    rows, cols = d.ri(3, max_rows), d.ri(3, max_cols)
    s = min((W - 1) // cols, (H - 1) // rows)
    grid = s * np.array([[j, i] for i in range(rows + 1) for j in range(cols + 1)], np.int64)
    wp = _warp_grid(d, H, W, grid, transform_params)
    recs = []
    for i in range(rows):
        for j in range(cols):
            if i == 0 and j == 0:
                rule = rule_contrast(d.u(), mc)
            else:
                rule = rule_different([d.u() for _ in range(CANDIDATES)], mc, (i - 1) * cols + j if i else -1, i * cols + j - 1 if j else -1)
            k = i * (cols + 1) + j
            recs.append(make_record(POLYGON, _quad(wp, (k, k + 1, k + cols + 2, k + cols + 1)), 4, rule))
    nb_rows, nb_cols = d.ri(2, rows + 2), d.ri(2, cols + 2)
    t = _thickness(d, min(H, W), 0.01, 0.015)
    for _ in range(nb_rows):
        r, c1, c2 = d.nr(0, rows + 1), d.nr(0, cols + 1), d.nr(0, cols + 1)
        recs.append(make_record(SEGMENT, _quad(wp, (r * (cols + 1) + c1, r * (cols + 1) + c2)), t, rule_contrast(d.u(), mc)))
    for _ in range(nb_cols):
        c, r1, r2 = d.nr(0, cols + 1), d.nr(0, rows + 1), d.nr(0, rows + 1)
        recs.append(make_record(SEGMENT, _quad(wp, (r1 * (cols + 1) + c, r2 * (cols + 1) + c)), t, rule_contrast(d.u(), mc)))
    return recs, keep_points_inside(wp, H, W)


def _stripes(d, H, W, mc, max_nb_cols=13, min_width_ratio=0.04, transform_params=(0.05, 0.15)):
    board = (int(H * (1 + d.u())), int(W * (1 + d.u())))
    col = d.ri(5, max_nb_cols)
    cols = np.unique(np.concatenate([board[1] * d.rng.random(col - 1), [0, board[1] - 1]]).astype(np.int64))
    min_dim = min(H, W)
    min_width = min_dim * min_width_ratio
    cols = cols[(np.concatenate([cols[1:], [board[1] + min_width]]) - cols) >= min_width]
    col = len(cols) - 1
    grid = np.concatenate([np.stack([cols, np.zeros(col + 1, np.int64)], 1), np.stack([cols, np.full(col + 1, board[0] - 1, np.int64)], 1)])
    wp = _warp_grid(d, H, W, grid, transform_params)
    recs = [make_record(NOP, rule=rule_contrast(d.u(), mc))]          # the chain's start: a colour that is never drawn
    for i in range(col):
        recs.append(make_record(POLYGON, _quad(wp, (i, i + 1, i + col + 2, i + col + 1)), 4, rule_rel(len(recs) - 1, 0.4 + d.u() * 0.2)))
    nb_rows, nb_cols = d.ri(2, 5), d.ri(2, col + 2)
    t = _thickness(d, min_dim, 0.01, 0.015)
    for _ in range(nb_rows):
        r, c1, c2 = (0, col + 1)[d.nr(0, 2)], d.nr(0, col + 1), d.nr(0, col + 1)
        recs.append(make_record(SEGMENT, _quad(wp, (r + c1, r + c2)), t, rule_contrast(d.u(), mc)))
    for _ in range(nb_cols):
        c = d.nr(0, col + 1)
        recs.append(make_record(SEGMENT, _quad(wp, (c, c + col + 1)), t, rule_contrast(d.u(), mc)))
    return recs, keep_points_inside(wp, H, W)


def _cube(d, H, W, mc, min_size_ratio=0.2, min_angle_rot=math.pi / 10, scale_interval=(0.4, 0.6), trans_interval=(0.5, 0.2)):
    min_dim = min(H, W)
    lx, ly, lz = (min_dim * min_size_ratio + d.u() * 2 * min_dim / 3 for _ in range(3))
    cube = np.array([[0, 0, 0], [lx, 0, 0], [0, ly, 0], [lx, ly, 0], [0, 0, lz], [lx, 0, lz], [0, ly, lz], [lx, ly, lz]])
    a = d.rng.random(3) * 3 * math.pi / 10. + math.pi / 10.
    r1 = np.array([[math.cos(a[0]), -math.sin(a[0]), 0], [math.sin(a[0]), math.cos(a[0]), 0], [0, 0, 1]])
    r2 = np.array([[1, 0, 0], [0, math.cos(a[1]), -math.sin(a[1])], [0, math.sin(a[1]), math.cos(a[1])]])
    r3 = np.array([[math.cos(a[2]), 0, -math.sin(a[2])], [0, 1, 0], [math.sin(a[2]), 0, math.cos(a[2])]])
    scaling = np.diag([scale_interval[0] + d.u() * scale_interval[1] for _ in range(3)])
    trans = np.array([W * trans_interval[0] + d.ri(-int(W * trans_interval[1]), int(W * trans_interval[1])),
                      H * trans_interval[0] + d.ri(-int(H * trans_interval[1]), int(H * trans_interval[1])), 0])
    cube = (trans + (scaling @ (r1 @ (r2 @ (r3 @ cube.T)))).T)[:, :2].astype(np.int64)          # projected on z = 0; corner 0 is hidden
    faces = [[7, 3, 1, 5], [7, 5, 4, 6], [7, 6, 2, 3]]
    recs = [make_record(POLYGON, _quad(cube, faces[0]), 4, rule_contrast(d.u(), mc))]
    recs += [make_record(POLYGON, _quad(cube, f), 4, rule_rel(0, 0.0)) for f in faces[1:]]
    a0 = int(math.ceil(min_dim * 0.003))
    t = d.ri(a0, max(int(min_dim * 0.015), a0))
    for f in faces:
        for j in range(4):
            recs.append(make_record(SEGMENT, _quad(cube, (f[j], f[(j + 1) % 4])), t, rule_rel(0, 0.25 + d.u() * 0.5)))
    return recs, keep_points_inside(cube[1:], H, W)


def _noise(d, H, W, mc):
    return [make_record(NOISE)], np.zeros((0, 2), np.int64)


_SAMPLERS = {'draw_lines': _lines, 'draw_polygon': _polygon, 'draw_multiple_polygons': _multiple_polygons, 'draw_ellipses': _ellipses, 'draw_star': _star, 'draw_checkerboard': _checkerboard,
             'draw_stripes': _stripes, 'draw_cube': _cube, 'gaussian_noise': _noise}


def final_keypoints(points_xy, generation_size, image_size):
    """SyntheticShapes' own steps on the generation-frame points (x, y): flip to (y, x), scale by image_size / generation_size, np.round,
    astype(int), then apply_augmentation's clamp to the last row / column."""
    kp = np.flip(np.asarray(points_xy, np.int64).reshape(-1, 2), 1)
    if list(generation_size) != list(image_size):
        kp = (np.array(image_size).astype(np.float64) / np.array(generation_size) * kp).round().astype(np.int64)
    kp = kp.copy()
    kp[kp[:, 0] >= image_size[0], 0] = image_size[0] - 1
    kp[kp[:, 1] >= image_size[1], 1] = image_size[1] - 1
    return kp


def sample_draw_lists(config, indices, seed, is_optical=None):
    """One draw list per index: [{'index', 'primitive', 'is_optical', 'threshold', 'blobs' [(cx, cy, r)], 'blob_raw', 'bg_ksize', 'records',
    'points' (n, 2) generation-frame (x, y), 'keypoints' (n, 2) image-frame (y, x)}].  config: a merged config (`merge_config`) or the
    caller's partial one.  is_optical: None draws the flag per sample, a bool forces it for every sample."""
    cfg = merge_config(config)
    prims = parse_primitives(cfg['primitives'], bool(cfg.get('textured_polygons', False)))
    H, W = (int(v) for v in cfg['generation_size'])
    gen = cfg['generation']
    mc = float(gen.get('min_contrast', 0.1))
    out = []
    for index in indices:
        index = int(index)
        if not 0 <= index < 1 << 29:
            raise ValueError(f"sample_draw_lists: indices lie in [0, 2^29), got {index}")
        d = _Draw(np.random.default_rng([int(seed) & 0xFFFFFFFFFFFFFFFF, index]))
        flag = bool(d.ri(0, 1))
        thr, blobs, raw, ks = _sample_background(d, H, W, gen.get('generate_background', {}))
        prim = prims[d.nr(0, len(prims))]
        recs, pts = _SAMPLERS[prim](d, H, W, mc, **gen.get(prim, {}))
        out.append({'index': index, 'primitive': prim, 'is_optical': flag if is_optical is None else bool(is_optical), 'threshold': np.float32(thr),
                    'blobs': blobs, 'blob_raw': raw, 'bg_ksize': ks, 'records': recs, 'points': pts,
                    'keypoints': final_keypoints(pts, cfg['generation_size'], cfg['image_size'])})
    return out


# ------------------------------------------------------------------------------------------------ the device renderer
def _gauss_tables(sizes):
    from .augmentation import gaussian_kernel
    wts = np.zeros((len(sizes), int(max(sizes))), np.float32)
    for i, ks in enumerate(sizes):
        wts[i, :ks] = gaussian_kernel(int(ks)) if ks > 1 else 1.0
    return wts, np.asarray(sizes, np.int32)


def _reach(lo, hi, k, n):
    """(first, last) frame position that the box-blur windows (size k, anchor k // 2) of the positions lo .. hi reach after BORDER_REFLECT_101"""
    p = np.arange(lo - k // 2, hi - k // 2 + k)
    if n > 1:
        p = np.mod(p, 2 * (n - 1))
        p = np.where(p < n, p, 2 * (n - 1) - p)
    else:
        p = np.zeros_like(p)
    return int(p.min()), int(p.max())


def texture_jobs(tables, generation_size):
    """The work items of the TEXTURED records of packed draw lists, or None when there is none: {'jobs' (J, JOB_INTS) int32, 'offsets' (J, 3)
    int64, 'units' (3, J + 1) int32, 'tex_offsets' (B, R) int64, 'arena_floats', 'ksize' (min, max)} in the layouts of xp_synth_texture.  A job
    keeps, in floats of one arena: its texture over the texture box (th x tw: the record's box dilated by the blur window, the reflection at
    the frame's border folded back), the row pass (th x bw) and the blurred box (bh x bw).  The host knows every box, so the arena is sized
    exactly: the sum of those three products over the jobs, each at most H W (and far less for the sampler's lists, whose boxes lie in
    circles that do not nest); never a frame per polygon slot."""
    H, W = int(generation_size[0]), int(generation_size[1])
    rec = tables['records']
    B, R = rec.shape[:2]
    jobs, offs, units = [], [], [[0], [0], [0]]
    tex_offsets = np.full((B, R), -1, np.int64)
    arena = 0
    for b, r in zip(*np.nonzero(rec[:, :, 0] == TEXTURED)):
        row = rec[b, r]
        x0, y0, x1, y1, k, j = (int(v) for v in (*row[1:5], row[22], row[23]))
        if not 1 <= k <= MAX_KSIZE:
            raise ValueError(f"SyntheticShapes: a textured polygon's ksize must be in [1, {MAX_KSIZE}], got {k}")
        if not 0 <= j < MAX_RECORDS:
            raise ValueError(f"SyntheticShapes: a textured polygon's ordinal must be in [0, {MAX_RECORDS}), got {j}")
        if x0 > x1 or y0 > y1:
            continue                                      # the polygon lies outside the frame: it covers no pixel
        (tx0, tx1), (ty0, ty1) = _reach(x0, x1, k, W), _reach(y0, y1, k, H)
        bw, bh, tw, th = x1 - x0 + 1, y1 - y0 + 1, tx1 - tx0 + 1, ty1 - ty0 + 1
        jobs.append([b, r, j, k, x0, y0, x1, y1, tx0, ty0, tx1, ty1] + [0] * (JOB_INTS - 12))
        offs.append([arena, arena + tw * th, arena + tw * th + bw * th])
        tex_offsets[b, r] = offs[-1][2]
        arena += tw * th + bw * th + bw * bh
        for u, n in zip(units, (-(-tw // 32) * -(-th // 32), th, -(-bw // 64) * -(-bh // 256))):
            u.append(u[-1] + n)
    if not jobs:
        return None
    if max(u[-1] for u in units) >= 1 << 31:
        raise ValueError("SyntheticShapes: the textured polygons of one batch need more than 2^31 workgroups; render fewer images at a time")
    ks = [q[3] for q in jobs]
    return {'jobs': np.array(jobs, np.int32), 'offsets': np.array(offs, np.int64), 'units': np.array(units, np.int32), 'tex_offsets': tex_offsets,
            'arena_floats': arena, 'ksize': (min(ks), max(ks))}


def render(tables, generation_size, image_size, seed, device, blur_size=21, additional_ir_blur=True, additional_ir_blur_size=51, debug=False):
    """Execute packed draw lists (`pack_draw_lists`) on the device.  Returns (images (B, 1, h, w) f32, keypoint maps (B, h, w) bool), and with
    debug=True a third value: {'background', 'frame' (before the Gaussian), 'blurred' (before the resize), 'bg_mean', 'field_mean', 'colours'}.
    13 kernel launches for any B (11 with additional_ir_blur off or without a thermal sample in the batch, one fewer when the two sizes are
    equal) and one memset.  All tables are uploaded before the first launch and nothing is read back: the host never waits for the batch's own
    kernels.

    A batch that holds a TEXTURED record (draw_multiple_polygons) launches 3 kernels more, whatever B and the number of polygons: the textures,
    the row and the column pass of their box blur (xp_synth_texture, over the jobs of `texture_jobs`), and the rasteriser is the variant that
    reads the blurred boxes (xp_synth_rasterise_textured in place of xp_synth_rasterise).  The jobs share one arena of exactly
    `texture_jobs(...)['arena_floats']` floats (see there).  Any other batch launches what it always did.  debug=True then adds
    'texture_jobs': per job {'b', 'r', 'j', 'ksize', 'box', 'texture_box' (x0, y0, x1, y1 inclusive), 'texture' (th, tw) unblurred over the
    texture box, 'blurred' (bh, bw) over the record's box}."""
    import torch
    from ._lib import ptr
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.XPointHipError("SyntheticShapes renders on a GPU device: xpoint_amd has no CPU fallback")
    H, W = (int(v) for v in generation_size)
    h, w = (int(v) for v in image_size)
    for ks in (blur_size, additional_ir_blur_size):
        if ks < 1 or ks % 2 == 0:
            raise ValueError(f"SyntheticShapes: Gaussian sizes are odd and positive, got {ks}")
    B, R = tables['records'].shape[:2]
    seed = ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    with torch.cuda.device(dev):
        st = _lib.current_stream(dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ids, thr, geom, raw, bks = up(tables['ids']), up(tables['thresholds']), up(tables['blob_geom']), up(tables['blob_raw']), up(tables['bg_ksize'])
        recs, rules, vals, cands = up(tables['records']), up(tables['rules']), up(tables['rule_values']), up(tables['candidates'])
        pts, cnt = up(tables['points']), up(tables['counts'])
        # cv2.GaussianBlur's passes (xp_aug_blur): blur_size for every sample, then additional_ir_blur_size for the thermal ones; an optical sample of
        # a mixed batch gets a size-1 kernel of weight 1.0, which copies bit for bit, and a batch without a thermal sample skips the second pair.
        # Every table is uploaded HERE, before the first launch: a pageable upload makes the host wait for the stream, so none sits between launches.
        sizes = [[blur_size] * B]
        if additional_ir_blur and not all(bool(o) for o in tables['is_optical']):
            sizes.append([1 if o else additional_ir_blur_size for o in tables['is_optical']])
        gauss = [tuple(up(a) for a in _gauss_tables(sz)) for sz in sizes]
        tex = texture_jobs(tables, (H, W))
        if tex:
            nb, tex_mc = int(tables.get('texture_blobs', 3000)), float(tables.get('texture_min_contrast', 0.13))
            if not 0 <= nb <= MAX_TEXTURE_BLOBS:
                raise ValueError(f"SyntheticShapes: nb_blobs must be in [0, {MAX_TEXTURE_BLOBS}], got {nb}")
            jobs, offsets, units, tex_offsets = up(tex['jobs']), up(tex['offsets']), up(tex['units']), up(tex['tex_offsets'])
            arena = torch.empty(tex['arena_floats'], dtype=torch.float32, device=dev)
        frame, tmp = torch.empty((B, H, W), dtype=torch.float32, device=dev), torch.empty((B, H, W), dtype=torch.float32, device=dev)
        count_ws = torch.empty((B, 128), dtype=torch.int32, device=dev)
        part_ws = torch.empty((B, 128), dtype=torch.float64, device=dev)
        field_mean, bg_mean = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
        colours = torch.empty((B, R), dtype=torch.float32, device=dev)
        mc = float(tables.get('min_contrast', 0.13))          # generate_background's own default: the reference does not pass the config's
        _lib.call("xp_synth_background", ptr(frame), seed, ptr(ids), ptr(thr), ptr(geom), ptr(raw), int(tables['n_blobs']), mc, ptr(count_ws),
                  ptr(field_mean), B, H, W, st)
        _lib.call("xp_synth_box_blur", ptr(frame), ptr(tmp), ptr(frame), ptr(bks), B, H, W, st)
        _lib.call("xp_synth_resolve_colours", ptr(frame), ptr(rules), ptr(vals), ptr(cands), R, cands.shape[1], ptr(part_ws), ptr(colours),
                  ptr(bg_mean), B, H, W, st)
        dbg = {'background': frame.clone(), 'bg_mean': bg_mean, 'field_mean': field_mean, 'colours': colours} if debug else None
        if tex:
            _lib.call("xp_synth_texture", ptr(arena), tex['arena_floats'], ptr(jobs), ptr(offsets), ptr(units), len(tex['jobs']), ptr(colours), R, seed,
                      ptr(ids), nb, tex_mc, *tex['ksize'], *(int(u[-1]) for u in tex['units']), B, H, W, st)
            _lib.call("xp_synth_rasterise_textured", ptr(frame), ptr(recs), ptr(colours), seed, ptr(ids), ptr(arena), ptr(tex_offsets), R, B, H, W, st)
        else:
            _lib.call("xp_synth_rasterise", ptr(frame), ptr(recs), ptr(colours), seed, ptr(ids), R, B, H, W, st)
        if debug:
            dbg['frame'] = frame.clone()
            if tex:
                dbg['texture_jobs'] = []
                for q, o in zip(tex['jobs'].tolist(), tex['offsets'].tolist()):
                    bw, bh, tw, th = q[6] - q[4] + 1, q[7] - q[5] + 1, q[10] - q[8] + 1, q[11] - q[9] + 1
                    dbg['texture_jobs'].append({'b': q[0], 'r': q[1], 'j': q[2], 'ksize': q[3], 'box': tuple(q[4:8]), 'texture_box': tuple(q[8:12]),
                                                'texture': arena[o[0]:o[0] + tw * th].view(th, tw), 'blurred': arena[o[2]:o[2] + bw * bh].view(bh, bw)})
        for wts, ksz in gauss:
            _lib.call("xp_aug_blur", ptr(frame), ptr(tmp), ptr(wts), ptr(ksz), wts.shape[1], B, H, W, 0, st)
            _lib.call("xp_aug_blur", ptr(tmp), ptr(frame), ptr(wts), ptr(ksz), wts.shape[1], B, H, W, 1, st)
        if debug:
            dbg['blurred'] = frame.clone()
        if (H, W) != (h, w):
            image = torch.empty((B, h, w), dtype=torch.float32, device=dev)
            _lib.call("xp_synth_resize", ptr(frame), ptr(image), B, H, W, h, w, st)
        else:
            image = frame
        kmap = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
        _lib.call("xp_synth_scatter_points", ptr(pts), ptr(cnt), pts.shape[1], ptr(kmap), B, h, w, st)
    res = (image.view(B, 1, h, w), kmap.view(torch.bool))
    return res + (dbg,) if debug else res


# ------------------------------------------------------------------------------------------------ the dataset
def _merge_programs(progs):
    """Concatenate per-sample photometric program tables (each made for one sample) into one batch's."""
    out = {}
    for k in progs[0]:
        rows = [p[k] for p in progs]
        if k == 'shade_weights':
            width = max(r.shape[1] for r in rows)
            rows = [np.pad(r, ((0, 0), (0, width - r.shape[1]))) for r in rows]
        out[k] = np.ascontiguousarray(np.concatenate(rows, 0))
    return out


def _keyed_homography(seed, index, shape, params):
    """homographies.sample_homography with the process-wide generators keyed by (seed, index) for the call, and restored after it.  Not
    thread-safe: a thread that draws from np.random or random during the call gets keyed values (sample_homography takes no generator)."""
    s = np.random.SeedSequence([int(seed) & 0xFFFFFFFFFFFFFFFF, int(index), 2]).generate_state(2)
    np_state, py_state = np.random.get_state(), _random.getstate()
    try:
        np.random.seed(int(s[0]))
        _random.seed(int(s[1]))
        return _hom.sample_homography(shape, **{k: v for k, v in params.items() if k != 'corner_homography'})
    finally:
        np.random.set_state(np_state)
        _random.setstate(py_state)


class SyntheticShapes:
    """The reference's SyntheticShapes dataset with a batched device loader.  config: the reference's keys and defaults (`DEFAULT_CONFIG`);
    for the Gaussian sizes `processing.*` wins over the YAML's `preprocessing.*`, which wins over the defaults."""

    default_config = DEFAULT_CONFIG
    all_primitives = ALL_PRIMITIVES

    def __init__(self, config=None):
        self.config = merge_config(config)
        if self.config['on-the-fly'] is False:
            raise NotImplementedError("SyntheticShapes: 'on-the-fly': false reads an HDF5 set, and h5py is not available here; "
                                      "only on-the-fly generation is implemented")
        if not self.config['keypoints_as_map']:
            raise NotImplementedError("SyntheticShapes: 'keypoints_as_map': false (keypoint lists) is not implemented; the loss takes label maps")
        self.primitives = parse_primitives(self.config['primitives'], bool(self.config.get('textured_polygons', False)))

    def __len__(self):
        return int(self.config['length'])

    def returns_pair(self):
        return False

    def render_batch(self, indices, device, seed=0, is_optical=None, debug=False):
        """The rendered images and label maps before any augmentation (`render`), plus the draw lists."""
        lists = sample_draw_lists(self.config, indices, seed, is_optical)
        tables = pack_draw_lists(lists, self.config['generation_size'])
        tables['min_contrast'] = float(self.config['generation'].get('generate_background', {}).get('min_contrast', 0.13))
        p = self.config['processing']
        return render(tables, self.config['generation_size'], self.config['image_size'], seed, device, int(p['blur_size']),
                      bool(p['additional_ir_blur']), int(p['additional_ir_blur_size']), debug=debug) + (lists,)

    def homographies(self, indices, seed=0):
        h, w = (int(v) for v in self.config['image_size'])
        params = self.config['augmentation']['homographic'].get('params', {}) or {}
        return np.stack([_keyed_homography(seed, i, (h, w), params) for i in indices])

    def load_batch(self, indices, device, seed=0, is_optical=None):
        """{'image' (B, 1, h, w) f32, 'keypoints' (B, h, w) bool, 'valid_mask' (B, 1, h, w) bool, 'is_optical' (B, 1) bool} on `device`:
        rendered, then photometric_augmentation, then homographic_augmentation (the reference's order).  Every draw of sample i is keyed by
        (seed, indices[i]).  is_optical forces the flag of every sample (a multispectral model takes one spectrum per batch)."""
        import torch
        from . import augmentation as _aug
        indices = [int(i) for i in indices]
        image, kmap, lists = self.render_batch(indices, device, seed, is_optical)
        B, _, h, w = image.shape
        acfg = self.config['augmentation']
        if acfg['photometric'].get('enable', False):
            progs = [_aug.sample_photometric_params(acfg['photometric'], 1, (h, w), np.random.default_rng([int(seed) & 0xFFFFFFFFFFFFFFFF, i, 1]))
                     for i in indices]
            image = _aug.photometric_augmentation(image.contiguous(), _merge_programs(progs), seed, sample_ids=indices)
        hc = acfg['homographic']
        if hc.get('enable', False):
            image, kmap, mask = _aug.homographic_augmentation(image, kmap, self.homographies(indices, seed), border_reflect=hc.get('border_reflect', True),
                                                              valid_border_margin=hc.get('valid_border_margin', 0), mask_border=hc.get('mask_border', True))
        else:
            mask = torch.ones((B, 1, h, w), dtype=torch.bool, device=image.device)
        flags = torch.tensor([[bool(d['is_optical'])] for d in lists], dtype=torch.bool, device=image.device)
        return {'image': image.contiguous(), 'keypoints': kmap, 'valid_mask': mask, 'is_optical': flags}
