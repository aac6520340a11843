// Homographic adaptation (reference xpoint/utils/homographies.py: homographic_adaptation_multispectral / homographic_adaptation,
// compute_valid_mask, warp_perspective_tensor): everything around the batched forwards, as four launches per chunk of homographies.
//
//   xp_ha_warp        kornia 0.1.4 warp_perspective_tensor of a whole chunk: n_dst images, image i = src[i % n_src] sampled with the
//                     normalised matrix M[i / n_src] (the matrix kornia hands to homography_warp: inverse(N_dst * H * N_src^-1)).
//                     Destination grid = torch.linspace(-1, 1, .) (two-sided, fused multiply-add: bit-equal to torch's CPU kernel),
//                     (X, Y, Z) = M * (gx, gy, 1) (separate multiplies and adds, left to right), (u, v) = (X / Z, Y / Z) with no epsilon
//                     guard (kornia 0.1.4 convert_points_from_homogeneous), then torch grid_sample with align_corners = False:
//                         ix = fma(u + 1, W / 2, -0.5)            (ATen's CPU unnormalise; equal to ((u + 1) W - 1) / 2)
//                         reflection: about -0.5 and W - 0.5, then clipped to [0, W - 1];  zeros: taps outside read 0
//                         bilinear: w = ix - floor(ix), e = 1 - w, n = iy - floor(iy), s = 1 - n,
//                                   out = fma(v_se, n w, fma(v_sw, n e, fma(v_ne, s w, v_nw * (s e))))   (ATen's CPU order)
//                         nearest:  rint (round half to even)
//                     The (w - 1) normalisation against align_corners = False sampling is the reference's half-pixel inconsistency,
//                     kept on purpose.
//   xp_ha_valid_mask  cv2.warpPerspective(ones, H, INTER_NEAREST) + cv2.erode((2r+1)^2) with the optional 1-pixel zero frame (mask_border):
//                     OpenCV's documented nearest scheme (csrc/cv_geom.h at scale 1, 0 outside), the erosion separable (row pass, column pass).
//                     Parity with OpenCV unpinned.
//   xp_ha_gaussian    utils.get_gaussian_filter behind nn.ReflectionPad2d: depthwise k x k on (n, H, W).
//   xp_ha_accumulate  per output pixel, the chunk's views IN ORDER: unwarp (bilinear, zeros) the forward outputs with the sampling matrix of
//                     inverse(H), combine (prod / sum per tap before interpolating; window: search_window over the unwarped maps, a tile
//                     plus halo in LDS), count_sample = the valid mask sampled by the nearest rule with the same matrix, and the running
//                     sums acc += value * count_sample, count += count_sample (f32, the reference's order).  A direct first view (the
//                     original images) initialises the sums unmasked with count = 1.  finalize: divide, sqrt (prod) / * 0.5 (sum),
//                     min_count.
// All four are memory-bound (DESIGN.md "Homographic adaptation"): one thread per output pixel, consecutive lanes on consecutive pixels.
#include "cv_geom.h"
#include "../../include/xpoint_hip.h"

namespace {

constexpr int HA_TX = 32, HA_TY = 8, HA_MAX_R = 15;

// torch.linspace(-1, 1, n)[i] as ATen's CPU kernel computes it: step = 2 / (n - 1), the lower half from -1, the upper half from 1, fused
__device__ __forceinline__ float ha_lin(int i, int n) {
    if (n == 1) return -1.f;
    const float step = 2.f / (float)(n - 1);
    return i < n / 2 ? fmaf(step, (float)i, -1.f) : fmaf(-step, (float)(n - i - 1), 1.f);
}

// the pixel coordinates (ix, iy) that grid_sample (align_corners = False) reads for destination pixel (x, y) under the normalised matrix m
__device__ __forceinline__ void ha_source(const float* __restrict__ m, int x, int y, int W, int H, int Ws, int Hs, float& ix, float& iy) {
    const float gx = ha_lin(x, W), gy = ha_lin(y, H);
    const float X = m[0] * gx + m[1] * gy + m[2];
    const float Y = m[3] * gx + m[4] * gy + m[5];
    const float Z = m[6] * gx + m[7] * gy + m[8];
    ix = fmaf(X / Z + 1.f, (float)Ws * 0.5f, -0.5f);
    iy = fmaf(Y / Z + 1.f, (float)Hs * 0.5f, -0.5f);
}

__device__ __forceinline__ float ha_reflect(float c, int S) {
    const float low = -0.5f, span2 = 2.f * (float)S;
    const float a = fabsf(c - low);
    const float flips = truncf(a / span2);
    const float extra = a - flips * span2;
    const float r = fminf(extra, span2 - extra) + low;
    return fminf((float)(S - 1), fmaxf(r, 0.f));
}

__device__ __forceinline__ float ha_tap(const float* __restrict__ p, int x, int y, int W, int H) {
    return ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) ? p[(size_t)y * W + x] : 0.f;
}

struct Bilinear { int x0, y0; float nw, ne, sw, se; };

__device__ __forceinline__ Bilinear ha_bilinear(float ix, float iy) {
    Bilinear b;
    const float fx = floorf(ix), fy = floorf(iy);
    const float w = ix - fx, e = 1.f - w, n = iy - fy, s = 1.f - n;
    b.x0 = (int)fx; b.y0 = (int)fy;
    b.nw = s * e; b.ne = s * w; b.sw = n * e; b.se = n * w;
    return b;
}

__device__ __forceinline__ float ha_interp(const Bilinear& b, float vnw, float vne, float vsw, float vse) {
    return fmaf(vse, b.se, fmaf(vsw, b.sw, fmaf(vne, b.ne, vnw * b.nw)));
}

// a coordinate far outside the image must not overflow the int conversion (those taps read 0 anyway)
__device__ __forceinline__ float ha_clamp_coord(float c) { return fminf(fmaxf(c, -16777216.f), 16777216.f); }

template <int BILINEAR, int REFLECT>
__global__ __launch_bounds__(256) void ha_warp_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ M,
                                                      int n_src, int Hs, int Ws, int Hd, int Wd) {
    const int i = blockIdx.z;
    const int x = xp_tile_x(), y = xp_tile_y();
    if (x >= Wd || y >= Hd) return;
    const float* m = M + (size_t)(i / n_src) * 9;
    const float* s = src + (size_t)(i % n_src) * Hs * Ws;
    float ix, iy;
    ha_source(m, x, y, Wd, Hd, Ws, Hs, ix, iy);
    if (REFLECT) { ix = ha_reflect(ix, Ws); iy = ha_reflect(iy, Hs); }
    ix = ha_clamp_coord(ix); iy = ha_clamp_coord(iy);
    float v;
    if (BILINEAR) {
        const Bilinear b = ha_bilinear(ix, iy);
        v = ha_interp(b, ha_tap(s, b.x0, b.y0, Ws, Hs), ha_tap(s, b.x0 + 1, b.y0, Ws, Hs), ha_tap(s, b.x0, b.y0 + 1, Ws, Hs),
                      ha_tap(s, b.x0 + 1, b.y0 + 1, Ws, Hs));
    } else {
        v = ha_tap(s, (int)rintf(ix), (int)rintf(iy), Ws, Hs);
    }
    dst[((size_t)i * Hd + y) * Wd + x] = v;
}

// cv2.warpPerspective(np.ones((H, W)), Hm, (W, H), flags=INTER_NEAREST) for K homographies (f64, the forward map)
__global__ __launch_bounds__(256) void ha_mask_warp_kernel(const double* __restrict__ Hm, uint8_t* __restrict__ out, int H, int W) {
    __shared__ double s_m[9];
    const int k = blockIdx.z;
    xp_cv_load_map(s_m, Hm + (size_t)k * 9, false, true);
    const int x = xp_tile_x(), y = xp_tile_y();
    if (x >= W || y >= H) return;
    int X, Y;
    xp_cv_source<1>(s_m, x, y, H, W, X, Y);
    out[((size_t)k * H + y) * W + x] = ((unsigned)X < (unsigned)W && (unsigned)Y < (unsigned)H) ? 1 : 0;
}

// one pass of the separable (2r+1) x (2r+1) erosion: minimum along x (VERTICAL = 0) or y (1).  A neighbour outside the image reads
// 0 with the zero frame (mask_border), and is ignored without it (cv2.erode's default border never erodes).
template <int VERTICAL>
__global__ __launch_bounds__(256) void ha_erode_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W, int r, int frame) {
    const int k = blockIdx.z;
    const int x = xp_tile_x(), y = xp_tile_y();
    if (x >= W || y >= H) return;
    const uint8_t* p = in + (size_t)k * H * W;
    int v = 1;
    for (int d = -r; d <= r; ++d) {
        const int xx = VERTICAL ? x : x + d, yy = VERTICAL ? y + d : y;
        if ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H) v = min(v, (int)p[(size_t)yy * W + xx]);
        else if (frame) v = 0;
    }
    out[((size_t)k * H + y) * W + x] = (uint8_t)v;
}

__device__ __forceinline__ int ha_reflect_index(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__global__ __launch_bounds__(256) void ha_gaussian_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ w,
                                                          int H, int W, int ks) {
    const int i = blockIdx.z;
    const int x = xp_tile_x(), y = xp_tile_y();
    if (x >= W || y >= H) return;
    const float* p = src + (size_t)i * H * W;
    const int r = ks / 2;
    float acc = 0.f;
    for (int dy = 0; dy < ks; ++dy) {
        const int yy = ha_reflect_index(y + dy - r, H);
        for (int dx = 0; dx < ks; ++dx) acc = fmaf(w[dy * ks + dx], p[(size_t)yy * W + ha_reflect_index(x + dx - r, W)], acc);
    }
    dst[((size_t)i * H + y) * W + x] = acc;
}

struct HaAccParams {
    const float* prob;        // (n_views, S, B, H, W) forward outputs of the chunk
    const float* M;           // (n_views - first_direct, 9) normalised sampling matrices of inverse(H)
    const uint8_t* mask;      // (n_views - first_direct, H, W) eroded valid masks
    float* acc0; float* acc1; float* count;    // (B, H, W)
    int B, n_views, first_direct, H, W, r, weighted, finalize;
    float min_count;
};

// unwarped value of map p at pixel (x, y) for the bilinear tap set b; COMB: the map is the product / sum of two maps, formed per tap
template <int MODE>
__device__ __forceinline__ float ha_unwarp(const float* __restrict__ p0, const float* __restrict__ p1, const Bilinear& b, int W, int H) {
    float t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int xx = b.x0 + (j & 1), yy = b.y0 + (j >> 1);
        if (MODE == XP_HA_PROD) t[j] = ha_tap(p0, xx, yy, W, H) * ha_tap(p1, xx, yy, W, H);
        else if (MODE == XP_HA_SUM) t[j] = ha_tap(p0, xx, yy, W, H) + ha_tap(p1, xx, yy, W, H);
        else t[j] = ha_tap(p0, xx, yy, W, H);
    }
    return ha_interp(b, t[0], t[1], t[2], t[3]);
}

template <int MODE>
__global__ __launch_bounds__(256) void ha_accumulate_kernel(HaAccParams p) {
    constexpr int S = MODE == XP_HA_SINGLE ? 1 : 2;
    constexpr int LD = HA_TX + 2 * HA_MAX_R;
    __shared__ float s_o[MODE == XP_HA_WINDOW ? (HA_TY + 2 * HA_MAX_R) * LD : 1];
    __shared__ float s_t[MODE == XP_HA_WINDOW ? (HA_TY + 2 * HA_MAX_R) * LD : 1];
    const int b = blockIdx.z, H = p.H, W = p.W, B = p.B;
    const int tx = threadIdx.x % HA_TX, ty = threadIdx.x / HA_TX;
    const int x0 = blockIdx.x * HA_TX, y0 = blockIdx.y * HA_TY;
    const int x = x0 + tx, y = y0 + ty;
    const bool in = x < W && y < H;
    const size_t HW = (size_t)H * W, pix = (size_t)y * W + x, out_off = (size_t)b * HW + pix;
    float a0 = 0.f, a1 = 0.f, cnt = 0.f;
    if (in && !p.first_direct) { a0 = p.acc0[out_off]; if (MODE == XP_HA_WINDOW) a1 = p.acc1[out_off]; cnt = p.count[out_off]; }
    const int r = p.r, tw = HA_TX + 2 * r, th = HA_TY + 2 * r;
    for (int v = 0; v < p.n_views; ++v) {
        const bool direct = p.first_direct && v == 0;
        const float* po = p.prob + ((size_t)v * S * B + b) * HW;        // optical (or the single map)
        const float* pt = po + (size_t)B * HW;                          // thermal (S == 2)
        const int j = v - p.first_direct;
        const float* m = p.M + (size_t)(direct ? 0 : j) * 9;
        float cs = 1.f;
        Bilinear bl{};
        if (!direct && in) {
            float ix, iy;
            ha_source(m, x, y, W, H, W, H, ix, iy);
            ix = ha_clamp_coord(ix); iy = ha_clamp_coord(iy);
            bl = ha_bilinear(ix, iy);
            const int nx = (int)rintf(ix), ny = (int)rintf(iy);
            cs = ((unsigned)nx < (unsigned)W && (unsigned)ny < (unsigned)H) ? (float)p.mask[(size_t)j * HW + (size_t)ny * W + nx] : 0.f;
        }
        if constexpr (MODE == XP_HA_WINDOW) {
            // the unwarped optical / thermal maps over the tile plus a radius-r halo (zero outside the image = search_window's ZeroPad2d)
            for (int e = threadIdx.x; e < tw * th; e += blockDim.x) {
                const int hx = x0 - r + e % tw, hy = y0 - r + e / tw;
                float vo = 0.f, vt = 0.f;
                if ((unsigned)hx < (unsigned)W && (unsigned)hy < (unsigned)H) {
                    if (direct) {
                        vo = po[(size_t)hy * W + hx]; vt = pt[(size_t)hy * W + hx];
                    } else {
                        float ix, iy;
                        ha_source(m, hx, hy, W, H, W, H, ix, iy);
                        const Bilinear bh = ha_bilinear(ha_clamp_coord(ix), ha_clamp_coord(iy));
                        vo = ha_unwarp<XP_HA_SINGLE>(po, nullptr, bh, W, H);
                        vt = ha_unwarp<XP_HA_SINGLE>(pt, nullptr, bh, W, H);
                    }
                }
                s_o[(e / tw) * LD + e % tw] = vo; s_t[(e / tw) * LD + e % tw] = vt;
            }
            __syncthreads();
            if (in) {
                float so = 0.f, st = 0.f;
                for (int dy = 0; dy <= 2 * r; ++dy)
                    for (int dx = 0; dx <= 2 * r; ++dx) {
                        so += s_o[(ty + dy) * LD + tx + dx];
                        st += s_t[(ty + dy) * LD + tx + dx];
                    }
                float f0 = st * s_o[(ty + r) * LD + tx + r], f1 = so * s_t[(ty + r) * LD + tx + r];
                if (!p.weighted) { f0 = f0 > 0.f ? 1.f : f0; f1 = f1 > 0.f ? 1.f : f1; }
                if (direct) { a0 = f0; a1 = f1; cnt = 1.f; }
                else { cnt += cs; a0 += f0 * cs; a1 += f1 * cs; }
            }
            __syncthreads();
        } else if (in) {
            if (direct) {
                const float vo = po[pix];
                a0 = MODE == XP_HA_PROD ? vo * pt[pix] : (MODE == XP_HA_SUM ? vo + pt[pix] : vo);
                cnt = 1.f;
            } else {
                cnt += cs;
                a0 += ha_unwarp<MODE>(po, pt, bl, W, H) * cs;
            }
        }
    }
    if (!in) return;
    if (p.finalize) {
        a0 = a0 / cnt;
        if (MODE == XP_HA_PROD) a0 = sqrtf(a0);
        else if (MODE == XP_HA_SUM) a0 = a0 * 0.5f;
        else if (MODE == XP_HA_WINDOW) a1 = a1 / cnt;
        if (p.min_count > 0.f && cnt < p.min_count) { a0 = 0.f; a1 = 0.f; }
    }
    p.acc0[out_off] = a0;
    if (MODE == XP_HA_WINDOW) p.acc1[out_off] = a1;
    p.count[out_off] = cnt;
}

}  // namespace

extern "C" int xp_ha_warp(const float* src, float* dst, const float* M, int n_src, int n_dst, int Hs, int Ws, int Hd, int Wd, int mode,
                          int padding, void* stream) {
    XP_CHECK_ARG(src && dst && M, "xp_ha_warp: null pointer");
    XP_CHECK_ARG(n_src > 0 && n_dst > 0 && n_dst <= 65535 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && Hd <= 4 * 65535,
                 "xp_ha_warp: bad shape (%d -> %d images, %d x %d -> %d x %d)", n_src, n_dst, Hs, Ws, Hd, Wd);
    XP_CHECK_ARG(mode == XP_HA_NEAREST || mode == XP_HA_BILINEAR, "xp_ha_warp: unknown mode %d", mode);
    XP_CHECK_ARG(padding == XP_HA_ZEROS || padding == XP_HA_REFLECTION, "xp_ha_warp: unknown padding %d", padding);
    XP_CHECK_ARG(src != dst, "xp_ha_warp: in-place warp is not supported");
    const dim3 grid = xp_tile_grid(Wd, Hd, n_dst), block(256);
    XpProfScope prof("ha_warp", (hipStream_t)stream, 0.0, 8.0 * n_dst * Hd * Wd);
    const bool bil = mode == XP_HA_BILINEAR, refl = padding == XP_HA_REFLECTION;
    if (bil && refl) hipLaunchKernelGGL((ha_warp_kernel<1, 1>), grid, block, 0, (hipStream_t)stream, src, dst, M, n_src, Hs, Ws, Hd, Wd);
    else if (bil) hipLaunchKernelGGL((ha_warp_kernel<1, 0>), grid, block, 0, (hipStream_t)stream, src, dst, M, n_src, Hs, Ws, Hd, Wd);
    else if (refl) hipLaunchKernelGGL((ha_warp_kernel<0, 1>), grid, block, 0, (hipStream_t)stream, src, dst, M, n_src, Hs, Ws, Hd, Wd);
    else hipLaunchKernelGGL((ha_warp_kernel<0, 0>), grid, block, 0, (hipStream_t)stream, src, dst, M, n_src, Hs, Ws, Hd, Wd);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_ha_valid_mask(const double* Hm, uint8_t* mask, uint8_t* tmp, int K, int H, int W, int erosion_radius, int mask_border, void* stream) {
    XP_CHECK_ARG(Hm && mask && (tmp || erosion_radius == 0), "xp_ha_valid_mask: null pointer");
    XP_CHECK_ARG(K > 0 && K <= 65535 && H > 0 && W > 0 && H < 32768 && W < 32768, "xp_ha_valid_mask: bad shape (%d masks of %d x %d)", K, H, W);
    XP_CHECK_ARG(erosion_radius >= 0 && erosion_radius < 4096, "xp_ha_valid_mask: bad erosion radius %d", erosion_radius);
    XP_CHECK_ARG(((uintptr_t)Hm & 7) == 0, "xp_ha_valid_mask: misaligned matrix pointer");
    const dim3 grid = xp_tile_grid(W, H, K), block(256);
    XpProfScope prof("ha_valid_mask", (hipStream_t)stream, 0.0, (erosion_radius > 0 ? 5.0 : 1.0) * K * H * W);
    hipLaunchKernelGGL(ha_mask_warp_kernel, grid, block, 0, (hipStream_t)stream, Hm, mask, H, W);
    if (erosion_radius > 0) {
        const int frame = mask_border ? 1 : 0;
        hipLaunchKernelGGL(ha_erode_kernel<0>, grid, block, 0, (hipStream_t)stream, mask, tmp, H, W, erosion_radius, frame);
        hipLaunchKernelGGL(ha_erode_kernel<1>, grid, block, 0, (hipStream_t)stream, tmp, mask, H, W, erosion_radius, frame);
    }
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_ha_gaussian(const float* src, float* dst, const float* weights, int n, int H, int W, int ksize, void* stream) {
    XP_CHECK_ARG(src && dst && weights, "xp_ha_gaussian: null pointer");
    XP_CHECK_ARG(n > 0 && n <= 65535 && H > 0 && W > 0 && H <= 4 * 65535, "xp_ha_gaussian: bad shape (%d x %d x %d)", n, H, W);
    XP_CHECK_ARG(ksize >= 1 && ksize % 2 == 1 && ksize / 2 < H && ksize / 2 < W, "xp_ha_gaussian: ksize %d must be odd with a reflection pad smaller than the image", ksize);
    XP_CHECK_ARG(src != dst, "xp_ha_gaussian: in-place filtering is not supported");
    const dim3 grid = xp_tile_grid(W, H, n), block(256);
    XpProfScope prof("ha_gaussian", (hipStream_t)stream, 2.0 * ksize * ksize * n * H * W, 8.0 * n * H * W);
    hipLaunchKernelGGL(ha_gaussian_kernel, grid, block, 0, (hipStream_t)stream, src, dst, weights, H, W, ksize);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_ha_accumulate(const float* prob, const float* M, const uint8_t* mask, float* acc0, float* acc1, float* count, int B, int n_views,
                                int first_direct, int H, int W, int mode, int window_size, int weighted, int finalize, float min_count, void* stream) {
    XP_CHECK_ARG(prob && acc0 && count && (mode != XP_HA_WINDOW || acc1), "xp_ha_accumulate: null pointer");
    XP_CHECK_ARG(n_views - (first_direct ? 1 : 0) == 0 || (M && mask), "xp_ha_accumulate: null matrix / mask pointer");
    XP_CHECK_ARG(B > 0 && B <= 65535 && n_views > 0 && H > 0 && W > 0, "xp_ha_accumulate: bad shape (B %d, %d views, %d x %d)", B, n_views, H, W);
    XP_CHECK_ARG(mode == XP_HA_SINGLE || mode == XP_HA_PROD || mode == XP_HA_SUM || mode == XP_HA_WINDOW, "xp_ha_accumulate: unknown mode %d", mode);
    XP_CHECK_ARG(mode != XP_HA_WINDOW || (window_size % 2 == 1 && window_size >= 1 && window_size <= 2 * HA_MAX_R + 1),
                 "xp_ha_accumulate: window_size must be odd and at most %d, got %d", 2 * HA_MAX_R + 1, window_size);
    HaAccParams p{prob, M, mask, acc0, acc1, count, B, n_views, first_direct ? 1 : 0, H, W, mode == XP_HA_WINDOW ? window_size / 2 : 0,
                  weighted ? 1 : 0, finalize ? 1 : 0, min_count};
    const dim3 grid(xp_cdiv(W, HA_TX), xp_cdiv(H, HA_TY), B), block(HA_TX * HA_TY);
    const double S = mode == XP_HA_SINGLE ? 1.0 : 2.0, px = (double)B * H * W;
    const int n_sampled = n_views - (first_direct ? 1 : 0);
    // forward outputs once per view, one mask byte per sampled view and pixel, the running sums read (unless initialised here) and written
    const double bytes = px * (4.0 * S * n_views + (double)n_sampled) + px * 4.0 * (mode == XP_HA_WINDOW ? 3.0 : 2.0) * (first_direct ? 1.0 : 2.0);
    XpProfScope prof("ha_accumulate", (hipStream_t)stream, 0.0, bytes);
    if (mode == XP_HA_SINGLE) hipLaunchKernelGGL(ha_accumulate_kernel<XP_HA_SINGLE>, grid, block, 0, (hipStream_t)stream, p);
    else if (mode == XP_HA_PROD) hipLaunchKernelGGL(ha_accumulate_kernel<XP_HA_PROD>, grid, block, 0, (hipStream_t)stream, p);
    else if (mode == XP_HA_SUM) hipLaunchKernelGGL(ha_accumulate_kernel<XP_HA_SUM>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(ha_accumulate_kernel<XP_HA_WINDOW>, grid, block, 0, (hipStream_t)stream, p);
    XP_LAUNCH_CHECK();
    return XP_OK;
}
