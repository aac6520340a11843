"""A plain numpy restatement of the textured polygons of the SyntheticShapes renderer (draw_multiple_polygons; csrc/synth_shapes.hip,
xp_synth_texture), in f64 and on exact integers: the oracle of test_cpu_textured_polygons.py and test_gpu_textured_polygons.py.  It reads the
packed tables of `synthetic_shapes.pack_draw_lists` and imports nothing of the device renderer.  The blobs' uniform draws are an input (the
Philox generator has its own tests): a (J, 4 NB) table, row j = the textured record of ordinal j, columns 4 i .. 4 i + 3 = blob i."""
import numpy as np

from tests import synthetic_shapes_f64 as ref

TEXTURED = 6


def blobs(u_row, H, W, min_contrast):
    """(cx, cy, r, colour) arrays of the NB blobs of one texture from its 4 NB uniforms; the products in f64, the colours rounded to f32"""
    u = np.asarray(u_row, np.float64).reshape(-1, 4)
    cx, cy, r = np.floor(u[:, 0] * W).astype(np.int64), np.floor(u[:, 1] * H).astype(np.int64), np.floor(u[:, 2] * 20).astype(np.int64)
    col = np.array([np.float32(ref.contrast(float(v), 0.0, min_contrast)) for v in u[:, 3]], np.float32)
    return cx, cy, r, col


def texture(u_row, base, H, W, min_contrast):
    """T_j over the whole frame: the colour of the highest-index blob with dx^2 + dy^2 <= r^2, else `base`; f32 values in an f64 array"""
    cx, cy, r, col = blobs(u_row, H, W, min_contrast)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    out = np.full((H, W), np.float64(np.float32(base)))
    for i in range(len(r)):                                          # ascending: a later blob overwrites
        x0, x1, y0, y1 = max(cx[i] - r[i], 0), min(cx[i] + r[i], W - 1), max(cy[i] - r[i], 0), min(cy[i] + r[i], H - 1)
        m = (xx[y0:y1 + 1, x0:x1 + 1] - cx[i]) ** 2 + (yy[y0:y1 + 1, x0:x1 + 1] - cy[i]) ** 2 <= r[i] * r[i]
        out[y0:y1 + 1, x0:x1 + 1][m] = np.float64(col[i])
    return out


def blurred(tex, k):
    """cv2.blur(T_j, (k, k)) over the whole frame, f64; k = 1 is the texture itself (no prefix sums in between)"""
    return np.array(tex, np.float64) if k == 1 else ref.box_blur(tex, k)


def coverage(tables, b, H, W):
    """synthetic_shapes_f64.coverage with a TEXTURED record covering what the POLYGON of the same vertices covers"""
    t = dict(tables)
    t['records'] = tables['records'].copy()
    t['records'][:, :, 0][tables['records'][:, :, 0] == TEXTURED] = ref.POLYGON
    return ref.coverage(t, b, H, W)


def textured_records(tables, b):
    """[(record index, ksize, ordinal)] of image b, in list order"""
    rec = tables['records'][b]
    return [(r, int(rec[r, 22]), int(rec[r, 23])) for r in range(rec.shape[0]) if rec[r, 0] == TEXTURED]


def render(tables, b, background_field, noise_field, uniforms, generation_size, image_size, min_contrast, texture_min_contrast=0.13, blur_size=21,
           additional_ir_blur=True, additional_ir_blur_size=51):
    """every stage of image b in f64, as synthetic_shapes_f64.render, plus 'textures' / 'texture_blurs' {record index: (H, W)} and 'textured'
    (H, W) bool = the pixels that a textured record wins.  uniforms: the (J, 4 NB) table of image b."""
    H, W = generation_size
    h, w = image_size
    field_mean, painted = ref.background(tables, b, background_field, min_contrast)
    bg = ref.box_blur(painted, int(tables['bg_ksize'][b]))
    bg_mean = float(bg.mean())
    colours = ref.resolve_colours(tables, b, bg_mean)
    cover = coverage(tables, b, H, W)
    frame = ref.compose(tables, b, bg, cover, colours, noise_field)
    textures, blurs, textured = {}, {}, np.zeros((H, W), bool)
    for r, k, j in textured_records(tables, b):
        textures[r] = texture(uniforms[j], colours[r], H, W, texture_min_contrast)
        blurs[r] = blurred(textures[r], k)
        frame[cover == r] = blurs[r][cover == r]
        textured |= cover == r
    out = ref.gaussian_blur(frame, blur_size)
    if additional_ir_blur and not tables['is_optical'][b]:
        out = ref.gaussian_blur(out, additional_ir_blur_size)
    image = ref.resize_linear(out, h, w) if (H, W) != (h, w) else out
    return {'field_mean': field_mean, 'background': bg, 'bg_mean': bg_mean, 'colours': colours, 'cover': cover, 'frame': frame, 'blurred': out,
            'image': image, 'keypoints': ref.keypoint_map(tables, b, h, w), 'textures': textures, 'texture_blurs': blurs, 'textured': textured}
