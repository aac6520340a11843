// Perspective warp of a batch of images: the last step of the reference's registration flow,
//     warped_image = cv2.warpPerspective(im_optical, H_est, im_optical.shape[:2][::-1], borderMode=cv2.BORDER_CONSTANT)
// (predict_align_image_pair.py:308; demo.py:225-249), i.e. flags = INTER_LINEAR, borderValue = 0, M = the FORWARD map src -> dst, which
// OpenCV inverts before the per-pixel inverse mapping.  SURVEY.md 8(f) rank 2.
//
// The coordinate arithmetic (the 3 x 3 inverse in double, the block-structured row base, the 1/32-pixel fixed point, the f32 bilinear combine)
// is OpenCV's documented scheme, stated once in csrc/cv_geom.h ("parity unpinned"); the oracle
// (oracle/csrc/oracle_kernels.c: xo_warp_perspective_*) states the same scheme in plain C and the GPU tests demand bit-equality with it.
// This file adds the taps (a tap outside the source reads the border value 0) and the u8 path:
//        u8 : weights w = 32768 * (1 - ay / 32 | ay / 32) * (1 - ax / 32 | ax / 32) = exact integers (32 - ay | ay) * (32 - ax | ax) * 32,
//             out = (sum w_i * tap_i + 16384) >> 15
// One thread per destination pixel (all channels), 64 x 4 pixels per workgroup: consecutive lanes write consecutive pixels; the four taps of
// neighbouring pixels share cache lines.  HBM-bound: a 480 x 640 u8 image is 0.3 MB in, 0.3 MB out.
#include "cv_geom.h"
#include "../../include/xpoint_hip.h"

namespace {

struct WarpParams {
    const void* src; void* dst; const double* M;
    const uint8_t* mask;                                    // MODE 2 only, may be null: (batch, Hs, Ws) valid mask, nonzero = valid
    int Hs, Ws, Hd, Wd, C, Cd, inverse_map;
};

// source element (channel c) at (sx, sy), 0 outside.  MODE 0: u8 source; 1: f32 source; 2: f32 source quantised on load as the reference
// does before warping: (np.clip(img, 0, 1) * 255.0).astype(np.uint8)  (predict_align_image_pair.py:271: f32 multiply, truncation), after
// `optical *= mask_optical` (:267) when a mask is given: an invalid pixel reads 0 (img * 0 = +-0 for every finite img, which clips to 0)
template <int MODE>
__device__ __forceinline__ auto warp_tap(const void* __restrict__ src, const uint8_t* __restrict__ mask, int Hs, int Ws, int C, int sx, int sy, int c) {
    const bool in = (unsigned)sx < (unsigned)Ws && (unsigned)sy < (unsigned)Hs;
    const size_t pix = (size_t)(in ? sy : 0) * Ws + (in ? sx : 0);
    const size_t off = pix * C + c;
    if constexpr (MODE == 0) {
        return in ? (int)reinterpret_cast<const uint8_t*>(src)[off] : 0;
    } else if constexpr (MODE == 1) {
        return in ? reinterpret_cast<const float*>(src)[off] : 0.f;
    } else {
        float v = reinterpret_cast<const float*>(src)[off];
        if (mask && !mask[pix]) v = 0.f;
        v = fminf(fmaxf(v, 0.f), 1.f) * 255.0f;        // NaN clips to 0 here (numpy would propagate it; a NaN pixel has no u8 value either way)
        return in ? (int)v : 0;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void warp_perspective_kernel(WarpParams p) {
    __shared__ double s_m[9];
    const int b = blockIdx.z;
    xp_cv_load_map(s_m, p.M + (size_t)b * 9, p.inverse_map, true);
    const int x = xp_tile_x(), y = xp_tile_y();
    if (x >= p.Wd || y >= p.Hd) return;
    int X, Y, sx, sy, ax, ay;
    xp_cv_source<32>(s_m, x, y, p.Hd, p.Wd, X, Y);
    xp_cv_split(X, sx, ax); xp_cv_split(Y, sy, ay);
    const size_t src_off = (size_t)b * p.Hs * p.Ws * p.C;
    const size_t dst_off = (((size_t)b * p.Hd + y) * p.Wd + x) * p.Cd;
    const void* src = MODE == 0 ? (const void*)(reinterpret_cast<const uint8_t*>(p.src) + src_off) : (const void*)(reinterpret_cast<const float*>(p.src) + src_off);
    const uint8_t* mask = p.mask ? p.mask + (size_t)b * p.Hs * p.Ws : nullptr;
    for (int c = 0; c < p.Cd; ++c) {
        const int cs = c < p.C ? c : p.C - 1;               // Cd > C: a 1-channel source replicated (cv2.cvtColor(.., COLOR_GRAY2RGB) ahead of the warp)
        const auto t0 = warp_tap<MODE>(src, mask, p.Hs, p.Ws, p.C, sx, sy, cs), t1 = warp_tap<MODE>(src, mask, p.Hs, p.Ws, p.C, sx + 1, sy, cs);
        const auto t2 = warp_tap<MODE>(src, mask, p.Hs, p.Ws, p.C, sx, sy + 1, cs), t3 = warp_tap<MODE>(src, mask, p.Hs, p.Ws, p.C, sx + 1, sy + 1, cs);
        if constexpr (MODE == 1) {
            reinterpret_cast<float*>(p.dst)[dst_off + c] = xp_cv_bilinear_f32(t0, t1, t2, t3, ax, ay);
        } else {
            const int w0 = (32 - ay) * (32 - ax) * 32, w1 = (32 - ay) * ax * 32, w2 = ay * (32 - ax) * 32, w3 = ay * ax * 32;
            const int v = (t0 * w0 + t1 * w1 + t2 * w2 + t3 * w3 + 16384) >> 15;
            reinterpret_cast<uint8_t*>(p.dst)[dst_off + c] = (uint8_t)(v > 255 ? 255 : v);
        }
    }
}

}  // namespace

extern "C" int xp_warp_perspective_masked(const void* src, const uint8_t* mask, void* dst, const double* M, int batch, int Hs, int Ws, int Hd, int Wd,
                                          int channels, int dst_channels, int dtype, int inverse_map, void* stream) {
    XP_CHECK_ARG(src && dst && M, "xp_warp_perspective: null pointer");
    XP_CHECK_ARG(!mask || dtype == XP_WARP_F32_AS_U8, "xp_warp_perspective: a valid mask applies to the quantise-on-load mode (XP_WARP_F32_AS_U8) only");
    XP_CHECK_ARG(batch > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, "xp_warp_perspective: bad shape (batch %d, source %d x %d, destination %d x %d)", batch, Hs, Ws, Hd, Wd);
    XP_CHECK_ARG(Hs < 32768 && Ws < 32768 && Hd <= 65535 * 4 && batch <= 65535, "xp_warp_perspective: image too large (source coordinates are 16-bit, as in OpenCV's remap)");
    XP_CHECK_ARG(channels >= 1 && channels <= 4, "xp_warp_perspective: channels must be 1..4, got %d", channels);
    XP_CHECK_ARG(dst_channels == channels || (channels == 1 && dst_channels >= 1 && dst_channels <= 4),
                 "xp_warp_perspective: dst_channels must equal channels, or replicate a 1-channel source (got %d -> %d)", channels, dst_channels);
    XP_CHECK_ARG(dtype == XP_WARP_U8 || dtype == XP_WARP_F32 || dtype == XP_WARP_F32_AS_U8, "xp_warp_perspective: unknown dtype %d", dtype);
    XP_CHECK_ARG(((uintptr_t)M & 7) == 0 && (dtype == XP_WARP_U8 || ((uintptr_t)src & 3) == 0) && (dtype != XP_WARP_F32 || ((uintptr_t)dst & 3) == 0),
                 "xp_warp_perspective: misaligned pointer");
    XP_CHECK_ARG(src != dst, "xp_warp_perspective: in-place warp is not supported");
    WarpParams p{src, dst, M, mask, Hs, Ws, Hd, Wd, channels, dst_channels, inverse_map ? 1 : 0};
    const dim3 grid = xp_tile_grid(Wd, Hd, batch), block(256);
    const double px = (double)batch * Hd * Wd, eb = dtype == XP_WARP_F32 ? 4.0 : 1.0;
    XpProfScope prof("warp_perspective", (hipStream_t)stream, 0.0, px * dst_channels * eb + (double)batch * Hs * Ws * channels * (dtype == XP_WARP_U8 ? 1.0 : 4.0));
    if (dtype == XP_WARP_U8) hipLaunchKernelGGL(warp_perspective_kernel<0>, grid, block, 0, (hipStream_t)stream, p);
    else if (dtype == XP_WARP_F32) hipLaunchKernelGGL(warp_perspective_kernel<1>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(warp_perspective_kernel<2>, grid, block, 0, (hipStream_t)stream, p);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_warp_perspective(const void* src, void* dst, const double* M, int batch, int Hs, int Ws, int Hd, int Wd, int channels,
                                   int dst_channels, int dtype, int inverse_map, void* stream) {
    return xp_warp_perspective_masked(src, nullptr, dst, M, batch, Hs, Ws, Hd, Wd, channels, dst_channels, dtype, inverse_map, stream);
}
