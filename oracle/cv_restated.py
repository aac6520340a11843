"""OpenCV's warpPerspective coordinate scheme restated in numpy (numpy only: it runs wherever the tests and the tools run).  The CPU
yardstick of the three kernels that share xpoint_amd/csrc/cv_geom.h, where the scheme is described: tests/augmentation_f64.py and the cv2
stand-in of tools/make_golden_ha.py call this module, tests/test_cpu_warp_oracle.py ties it to the independent second yardstick, the
plain-C oracle (oracle/csrc/oracle_kernels.c: xo_warp_perspective_*).

OpenCV is absent: the routines are restated from their published definitions (cv::invert of a 3 x 3 matrix, WarpPerspectiveInvoker's
block-structured fixed-point coordinates, borderInterpolate, remap's f32 bilinear combine, erode), with the device's operation order, so
every comparison against the kernels is equality."""
import numpy as np


def cv_invert3(S):
    """OpenCV's closed 3 x 3 inverse in double, in the operand order of csrc/cv_geom.h: xp_cv_invert3; a singular matrix gives zeros."""
    S = np.asarray(S, np.float64).reshape(9)
    d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
    if d == 0.0:
        return np.zeros(9)
    d = 1.0 / d
    return np.array([(S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
                     (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
                     (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d])


def fixed_point_source(Hm, h, w, scale):
    """WarpPerspectiveInvoker's integer source coordinates (X, Y) of every pixel of an h x w destination under the forward map Hm:
    scale = 32 (INTER_LINEAR, 1/32 pixel) or 1 (INTER_NEAREST).  The row base is formed at the first column of the pixel's block, the
    in-block offset added afterwards."""
    m = cv_invert3(Hm)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    bw = min(64, w) if h >= 16 else min(w, 1024 // h)
    xb = (x // bw * bw).astype(np.float64)
    x1 = x.astype(np.float64) - xb
    y = y.astype(np.float64)
    X0 = m[0] * xb + m[1] * y + m[2]
    Y0 = m[3] * xb + m[4] * y + m[5]
    W0 = m[6] * xb + m[7] * y + m[8]
    W = W0 + m[6] * x1
    with np.errstate(divide="ignore", invalid="ignore"):
        W = np.where(W != 0.0, scale / W, 0.0)
        fX = np.maximum(-2147483648.0, np.minimum(2147483647.0, (X0 + m[0] * x1) * W))
        fY = np.maximum(-2147483648.0, np.minimum(2147483647.0, (Y0 + m[3] * x1) * W))
    return np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)          # round half to even, as lrint


def border_interpolate_101(p, length):
    """cv::borderInterpolate(p, len, BORDER_REFLECT_101), the loop as OpenCV writes it (delta = 1), elementwise."""
    p = np.array(p, dtype=np.int64, copy=True)
    if length == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= length)
        if not bad.any():
            return p
        p = np.where(bad & (p < 0), -p - 1 + 1, np.where(bad, length - 1 - (p - length) - 1, p))


def warp_perspective_f32(image, Hm, border_reflect):
    """cv2.warpPerspective(image f32 (h, w), Hm, (w, h), INTER_LINEAR, BORDER_REFLECT_101 | BORDER_CONSTANT) in the f32 arithmetic of
    csrc/cv_geom.h: returns f32, to be compared for equality."""
    image = np.asarray(image, np.float32)
    h, w = image.shape
    X, Y = fixed_point_source(Hm, h, w, 32.0)
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = (X & 31).astype(np.float32) * np.float32(0.03125), (Y & 31).astype(np.float32) * np.float32(0.03125)
    one = np.float32(1)

    def tap(xx, yy):
        if border_reflect:
            return image[border_interpolate_101(yy, h), border_interpolate_101(xx, w)]
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(inside, image[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], np.float32(0))

    t0, t1, t2, t3 = tap(sx, sy), tap(sx + 1, sy), tap(sx, sy + 1), tap(sx + 1, sy + 1)
    w0, w1, w2, w3 = (one - fy) * (one - fx), (one - fy) * fx, fy * (one - fx), fy * fx
    out = ((t0 * w0 + t1 * w1) + t2 * w2) + t3 * w3
    assert out.dtype == np.float32
    return out


def warp_perspective_nearest(src, Hm, h, w):
    """cv2.warpPerspective(src (hs, ws), Hm, (w, h), flags=INTER_NEAREST): the source pixel itself, 0 outside."""
    src = np.asarray(src)
    X, Y = fixed_point_source(Hm, h, w, 1.0)
    ok = (X >= 0) & (X < src.shape[1]) & (Y >= 0) & (Y < src.shape[0])
    out = np.zeros((h, w), dtype=src.dtype)
    out[ok] = src[Y[ok], X[ok]]
    return out


def erode(src, radius, zero_frame=False):
    """cv2.erode with a (2r+1)^2 kernel of ones: a neighbour outside the image is ignored (OpenCV's default border never erodes), or
    reads 0 behind a zero frame."""
    src = np.asarray(src)
    h, w = src.shape
    r = int(radius)
    p = np.pad(src.astype(np.float64), r, constant_values=0.0 if zero_frame else np.inf)
    out = np.full((h, w), np.inf)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = np.minimum(out, p[dy:dy + h, dx:dx + w])
    return out.astype(src.dtype)


def compute_valid_mask(shape, Hm, erosion_radius=0, mask_border=False):
    """reference homographies.py: compute_valid_mask: the INTER_NEAREST warp of ones, then the (2r+1)^2 erosion behind a zero frame
    (mask_border) or cv2.erode's default border.  Without an erosion the frame is not applied, as in the reference."""
    h, w = shape
    mask = warp_perspective_nearest(np.ones((h, w), np.uint8), Hm, h, w)
    if int(erosion_radius) > 0:
        mask = erode(mask, erosion_radius, zero_frame=mask_border)
    return mask.astype(bool)
