"""A plain numpy restatement of the SyntheticShapes renderer (csrc/synth_shapes.hip), in f64 and on exact integers: the oracle of
test_cpu_synthetic_shapes.py and test_gpu_synthetic_shapes.py.  It reads the packed tables of `synthetic_shapes.pack_draw_lists` (the
layouts of include/xpoint_hip.h) and imports nothing of the device renderer.  The uniform fields are inputs (the Philox generator has its own
tests): `background_field` / `noise_field` (H, W) arrays."""
import numpy as np

NOP, CIRCLE, SEGMENT, POLYGON, ELLIPSE, NOISE = range(6)
RULE_ABS, RULE_CONTRAST, RULE_DIFFERENT, RULE_REL = range(4)
CANDIDATES = 21


def reflect101(p, n):
    """cv::borderInterpolate BORDER_REFLECT_101 of integer positions p into [0, n)"""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    p = np.mod(p, period)
    return np.where(p < n, p, period - p)


def contrast(raw, mean, mc):
    return (raw + 0.5) % 1.0 if abs(raw - mean) < mc else raw


def background(tables, b, field, min_contrast):
    """(mean of the thresholded field, the painted frame before its box blur) of image b, f64"""
    H, W = field.shape
    img = (field > tables['thresholds'][b]).astype(np.float64)
    mean = float(img.sum()) / (H * W)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    for k in range(int(tables['n_blobs'])):
        cx, cy, r = (int(v) for v in tables['blob_geom'][b, k, :3])
        img[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = np.float32(contrast(float(tables['blob_raw'][b, k]), mean, min_contrast))
    return mean, img


def box_blur(img, k):
    """cv2.blur(img, (k, k)): normalised, anchor k // 2, BORDER_REFLECT_101; f64"""
    a = k // 2
    out = np.asarray(img, np.float64)
    for axis in (1, 0):
        n = out.shape[axis]
        ext = np.take(out, reflect101(np.arange(-a, n - a + k - 1), n), axis=axis)
        cs = np.cumsum(np.concatenate([np.zeros_like(np.take(ext, [0], axis=axis)), ext], axis=axis), axis=axis)
        out = (np.take(cs, np.arange(k, k + n), axis=axis) - np.take(cs, np.arange(0, n), axis=axis)) / k
    return out


def resolve_colours(tables, b, bg_mean):
    """the colour of every record of image b, f64, in order"""
    R = tables['rules'].shape[1]
    c = np.zeros(R)
    for r in range(R):
        kind, r0, r1, off = (int(v) for v in tables['rules'][b, r])
        v, m = (float(x) for x in tables['rule_values'][b, r])
        if kind == RULE_CONTRAST:
            c[r] = contrast(v, bg_mean, m)
        elif kind == RULE_DIFFERENT:
            cand = tables['candidates'][b, off:off + CANDIDATES]
            near = [c[i] for i in (r0, r1) if 0 <= i < r]
            c[r] = cand[-1]
            for t in cand[:-1]:
                if not any(abs(n - t) < m for n in near):
                    c[r] = t
                    break
        elif kind == RULE_REL:
            c[r] = (c[r0] + m) % 1.0
        else:
            c[r] = v
    return c


def in_circle(xx, yy, g, r):
    return (xx - g[0]) ** 2 + (yy - g[1]) ** 2 <= r * r


def in_segment(xx, yy, g, t):
    ax, ay, bx, by = (int(v) for v in g[:4])
    dx, dy, ux, uy = bx - ax, by - ay, xx - ax, yy - ay
    len2, proj, t2 = dx * dx + dy * dy, ux * dx + uy * dy, t * t
    cap_a = 4 * (ux * ux + uy * uy) <= t2
    cap_b = 4 * ((xx - bx) ** 2 + (yy - by) ** 2) <= t2
    cross = dx * uy - dy * ux
    band = cross * cross <= (t2 * len2) // 4
    if len2 == 0:
        return cap_a
    return np.where(proj < 0, cap_a, np.where(proj > len2, cap_b, band))


def in_polygon(xx, yy, g, n):
    odd = np.zeros(xx.shape, bool)
    edge = np.zeros(xx.shape, bool)
    for i in range(n):
        j = (i + 1) % n
        ax, ay, bx, by = int(g[2 * i]), int(g[2 * i + 1]), int(g[2 * j]), int(g[2 * j + 1])
        t = (bx - ax) * (yy - ay) - (xx - ax) * (by - ay)
        edge |= (t == 0) & (xx >= min(ax, bx)) & (xx <= max(ax, bx)) & (yy >= min(ay, by)) & (yy <= max(ay, by))
        cross = ((ay <= yy) != (by <= yy)) & ((t > 0) if by > ay else (t < 0))
        odd ^= cross
    return odd | edge


def in_ellipse(xx, yy, g, cs):
    dx, dy = (xx - int(g[0])).astype(np.float64), (yy - int(g[1])).astype(np.float64)
    ax, ay = max(float(g[2]), 0.5), max(float(g[3]), 0.5)
    u, w = (dx * cs[0] + dy * cs[1]) / ax, (dy * cs[0] - dx * cs[1]) / ay
    return u * u + w * w <= 1.0


def coverage(tables, b, H, W):
    """(H, W) int: the index of the last record that covers each pixel, -1 where none does (painter's order).  The analytic shapes alone: the
    records' bounding boxes are NOT read, so a packed box that cuts its shape shows as a mismatch against the device."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    cover = np.full((H, W), -1, np.int64)
    for r in range(tables['records'].shape[1]):
        rec = tables['records'][b, r]
        kind, n, g = int(rec[0]), int(rec[5]), rec[6:22].astype(np.int64)
        if kind == NOP:
            continue
        if kind == NOISE:
            cover[:] = r
            continue
        if kind == CIRCLE:
            m = in_circle(xx, yy, g, n)
        elif kind == SEGMENT:
            m = in_segment(xx, yy, g, n)
        elif kind == POLYGON:
            m = in_polygon(xx, yy, g, n)
        else:
            m = in_ellipse(xx, yy, g, rec[10:14].copy().view(np.float64))
        cover[m] = r
    return cover


def compose(tables, b, base, cover, colours, noise_field=None):
    """the frame: `base` where no record covers, the record's colour rounded to f32 where one does, the noise field under a NOISE record"""
    out = np.array(base, np.float64)
    hit = cover >= 0
    out[hit] = np.float32(colours)[cover[hit]].astype(np.float64)
    kinds = tables['records'][b, :, 0]
    for r in np.nonzero(kinds == NOISE)[0]:
        out[cover == r] = np.asarray(noise_field, np.float64)[cover == r]
    return out


def gaussian_kernel(ks):
    """cv2.getGaussianKernel(ks, 0) for ks > 7"""
    sigma = 0.3 * ((ks - 1) * 0.5 - 1) + 0.8
    x = np.arange(ks, dtype=np.float64) - (ks - 1) * 0.5
    k = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return k / k.sum()


def gaussian_blur(img, ks):
    """cv2.GaussianBlur(img, (ks, ks), 0): separable, BORDER_REFLECT_101; f64"""
    wt, r = gaussian_kernel(ks), ks // 2
    out = np.asarray(img, np.float64)
    for axis in (1, 0):
        n = out.shape[axis]
        acc = np.zeros_like(out)
        for d in range(ks):
            acc = acc + wt[d] * np.take(out, reflect101(np.arange(n) + d - r, n), axis=axis)
        out = acc
    return out


def resize_linear(img, h, w):
    """cv2.resize(img, (w, h), INTER_LINEAR): source coordinate (d + 0.5) scale - 0.5, clamped taps; f64"""
    H, W = img.shape

    def taps(n_dst, n_src):
        f = (np.arange(n_dst) + 0.5) * (n_src / n_dst) - 0.5
        i = np.floor(f).astype(np.int64)
        wgt = f - i
        wgt = np.where((i < 0) | (i >= n_src - 1), 0.0, wgt)
        i = np.clip(i, 0, n_src - 1)
        return i, np.minimum(i + 1, n_src - 1), wgt

    x0, x1, wx = taps(w, W)
    y0, y1, wy = taps(h, H)
    rows = img[:, x0] * (1 - wx) + img[:, x1] * wx
    return rows[y0] * (1 - wy)[:, None] + rows[y1] * wy[:, None]


def keypoint_map(tables, b, h, w):
    m = np.zeros((h, w), bool)
    for y, x in tables['points'][b, :int(tables['counts'][b])]:
        if 0 <= y < h and 0 <= x < w:
            m[y, x] = True
    return m


def render(tables, b, background_field, noise_field, generation_size, image_size, min_contrast, blur_size=21, additional_ir_blur=True,
           additional_ir_blur_size=51):
    """every stage of image b in f64: {'field_mean', 'background', 'bg_mean', 'colours', 'cover', 'frame', 'blurred', 'image', 'keypoints'}"""
    H, W = generation_size
    h, w = image_size
    field_mean, painted = background(tables, b, background_field, min_contrast)
    bg = box_blur(painted, int(tables['bg_ksize'][b]))
    bg_mean = float(bg.mean())
    colours = resolve_colours(tables, b, bg_mean)
    cover = coverage(tables, b, H, W)
    frame = compose(tables, b, bg, cover, colours, noise_field)
    blurred = gaussian_blur(frame, blur_size)
    if additional_ir_blur and not tables['is_optical'][b]:
        blurred = gaussian_blur(blurred, additional_ir_blur_size)
    image = resize_linear(blurred, h, w) if (H, W) != (h, w) else blurred
    return {'field_mean': field_mean, 'background': bg, 'bg_mean': bg_mean, 'colours': colours, 'cover': cover, 'frame': frame, 'blurred': blurred,
            'image': image, 'keypoints': keypoint_map(tables, b, h, w)}
