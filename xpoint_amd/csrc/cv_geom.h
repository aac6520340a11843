// OpenCV's warpPerspective coordinate arithmetic, stated ONCE for every kernel that needs it: warp_perspective_kernel (warp.hip),
// aug_warp_kernel (augment.hip) and ha_mask_warp_kernel (homadapt.hip).  The claims "xp_aug_warp without reflection is bit-equal to
// xp_warp_perspective", "the augmentation's valid mask is xp_ha_valid_mask" and "HIP == oracle bit for bit" hold because these kernels
// share the definitions below.  The CPU yardsticks restate the same scheme independently: oracle/cv_restated.py (numpy) and
// oracle/csrc/oracle_kernels.c: xo_warp_perspective_* (plain C).
//
// OpenCV is not available to this project, so this is the DOCUMENTED scheme of its imgproc module (warpPerspective -> remap,
// INTER_BITS = 5, INTER_REMAP_COEF_BITS = 15) restated from the published source: "parity unpinned" (DESIGN.md section 4).
//   1. M^-1 by the closed 3 x 3 cofactor form in double (no LU): t = adj(M) * (1 / det), det == 0 -> the zero matrix (xp_cv_invert3).
//      Thread 0 of a workgroup inverts (or, with WARP_INVERSE_MAP, copies) into LDS (xp_cv_load_map).
//   2. per destination pixel (x, y), in double, with the block structure of OpenCV's WarpPerspectiveInvoker: the row base is formed at
//      the first column xb of the pixel's block, the in-block offset x1 is added afterwards.  The block is min(64, width) wide for a
//      height >= 16 and min(BLOCK_SZ * BLOCK_SZ / height, width) below that (BLOCK_SZ = 32).  scale = 32 (INTER_LINEAR: 1/32 pixel)
//      or 1 (INTER_NEAREST); scale / W with scale == 1 is the same operation as 1 / W (xp_cv_source):
//          X0 = m0 * xb + m1 * y + m2,  Y0 = m3 * xb + m4 * y + m5,  W0 = m6 * xb + m7 * y + m8
//          W = W0 + m6 * x1;  W = W ? scale / W : 0
//          fX = clamp((X0 + m0 * x1) * W, INT_MIN, INT_MAX),  fY likewise;   X = lrint(fX), Y = lrint(fY)        (round half to even)
//   3. INTER_LINEAR: sx = sat16(X >> 5), ax = X & 31 (xp_cv_split), likewise y; taps at (sx, sy), (sx + 1, sy), (sx, sy + 1),
//      (sx + 1, sy + 1).  A tap outside the source reads the border value 0 (BORDER_CONSTANT) or goes through borderInterpolate
//      (BORDER_REFLECT_101: xp_cv_reflect101).  f32 images (xp_cv_bilinear_f32): weights (1 - fy) * (1 - fx), (1 - fy) * fx,
//      fy * (1 - fx), fy * fx with fx = ax / 32 (exact in f32), out = ((t0 * w0 + t1 * w1) + t2 * w2) + t3 * w3: separate multiplies
//      and adds, left to right (every translation unit is built with -ffp-contract=off).  The u8 integer weights are warp.hip's.
//      INTER_NEAREST: the pixel (X, Y) itself, 0 outside.
// The kernels run one thread per destination pixel, 64 x 4 pixels per workgroup of 256 (xp_tile_x / xp_tile_y / xp_tile_grid):
// consecutive lanes on consecutive pixels.  The other per-pixel kernels of the three files use the same tile.
#pragma once
#include "xp_common.h"

__device__ __forceinline__ int xp_tile_x() { return blockIdx.x * 64 + (threadIdx.x & 63); }
__device__ __forceinline__ int xp_tile_y() { return blockIdx.y * 4 + (threadIdx.x >> 6); }
static inline dim3 xp_tile_grid(int W, int H, int n) { return dim3(xp_cdiv(W, 64), xp_cdiv(H, 4), n); }

// OpenCV cv::invert of a 3 x 3 double matrix (DECOMP_LU): det3 and the cofactors in this operand order; a singular matrix gives zeros.
__device__ __forceinline__ void xp_cv_invert3(const double* __restrict__ S, double (&t)[9]) {
    double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (d != 0.0) {
        d = 1.0 / d;
        t[0] = (S[4] * S[8] - S[5] * S[7]) * d;
        t[1] = (S[2] * S[7] - S[1] * S[8]) * d;
        t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
        t[3] = (S[5] * S[6] - S[3] * S[8]) * d;
        t[4] = (S[0] * S[8] - S[2] * S[6]) * d;
        t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
        t[6] = (S[3] * S[7] - S[4] * S[6]) * d;
        t[7] = (S[1] * S[6] - S[0] * S[7]) * d;
        t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
    } else {
        for (int k = 0; k < 9; ++k) t[k] = 0.0;
    }
}

// the workgroup's inverse map in LDS: thread 0 inverts M (the forward map) or copies it (inverse_map); `on` = false leaves s_m
// unwritten (a sample that is not warped).  Every thread of the workgroup calls it.
__device__ __forceinline__ void xp_cv_load_map(double (&s_m)[9], const double* __restrict__ M, bool inverse_map, bool on) {
    if (threadIdx.x == 0 && on) {
        double t[9];
        if (inverse_map) { for (int k = 0; k < 9; ++k) t[k] = M[k]; } else xp_cv_invert3(M, t);
        for (int k = 0; k < 9; ++k) s_m[k] = t[k];
    }
    __syncthreads();
}

// integer source coordinates (X, Y) of destination pixel (x, y) of an Hd x Wd image under the inverse map m, in units of 1 / SCALE pixel
template <int SCALE>
__device__ __forceinline__ void xp_cv_source(const double (&m)[9], int x, int y, int Hd, int Wd, int& X, int& Y) {
    static_assert(SCALE == 32 || SCALE == 1, "INTER_LINEAR (32) or INTER_NEAREST (1)");
    const int bw0 = Wd < 64 ? Wd : 64;
    const int bw = Hd >= 16 ? bw0 : (Wd < 1024 / Hd ? Wd : 1024 / Hd);
    const int xb = x / bw * bw, x1 = x - xb;
    const double X0 = m[0] * xb + m[1] * y + m[2];
    const double Y0 = m[3] * xb + m[4] * y + m[5];
    const double W0 = m[6] * xb + m[7] * y + m[8];
    double W = W0 + m[6] * x1;
    W = W != 0.0 ? (double)SCALE / W : 0.0;
    const double fX = fmax(-2147483648.0, fmin(2147483647.0, (X0 + m[0] * x1) * W));
    const double fY = fmax(-2147483648.0, fmin(2147483647.0, (Y0 + m[3] * x1) * W));
    X = __double2int_rn(fX); Y = __double2int_rn(fY);         // NaN (0 * inf) -> 0, as lrint's result is then unspecified in C
}

__device__ __forceinline__ int xp_cv_sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// a 1/32-pixel coordinate -> the 16-bit pixel of the first tap and the 5-bit fraction
__device__ __forceinline__ void xp_cv_split(int X, int& s, int& a) { s = xp_cv_sat16(X >> 5); a = X & 31; }

__device__ __forceinline__ float xp_cv_bilinear_f32(float t0, float t1, float t2, float t3, int ax, int ay) {
    const float fx = (float)ax * 0.03125f, fy = (float)ay * 0.03125f;
    const float w0 = (1.f - fy) * (1.f - fx), w1 = (1.f - fy) * fx, w2 = fy * (1.f - fx), w3 = fy * fx;
    return ((t0 * w0 + t1 * w1) + t2 * w2) + t3 * w3;
}

// cv::borderInterpolate(p, len, BORDER_REFLECT_101): the repeated fold p < 0 -> -p, p >= len -> 2 len - 2 - p in closed form (a triangle wave
// of period 2 (len - 1)), so that a coordinate many image sizes outside costs no loop
__device__ __forceinline__ int xp_cv_reflect101(int p, int len) {
    if (len == 1) return 0;
    const int period = 2 * (len - 1);
    p %= period;
    if (p < 0) p += period;
    return p < len ? p : period - p;
}
