// Training-pair augmentation for a whole batch on the device (reference xpoint/datasets/augmentation/augmentation.py,
// photometric_augmentation.py; xpoint_amd/augmentation.py drives these).  No launch count below depends on the batch size.
//
//   xp_aug_warp            cv2.warpPerspective(image, H, (w, h), INTER_LINEAR, borderMode) of B one-channel f32 images: the 1/32-pixel scheme
//                          of csrc/cv_geom.h, shared with csrc/warp.hip, with borderMode = BORDER_CONSTANT (a tap outside reads 0: bit-equal to
//                          xp_warp_perspective) or BORDER_REFLECT_101 (every tap coordinate goes through borderInterpolate: folded about
//                          0 and len - 1 until inside, a dimension of 1 gives 0).  A sample with warp[b] == 0 is copied, and its valid
//                          mask (written by xp_ha_valid_mask before this launch) is set to all ones: the reference's dummy_valid_mask.
//   xp_aug_scatter_labels  warp_keypoints + filter_points + generate_keypoint_map: every set pixel (y, x) of the label map goes to
//                          (trunc(Y / W), trunc(X / W)), [X Y W] = H [x y 1] in f64 ((m0 x + m1 y) + m2, plain division), kept when
//                          0 <= y' < h and 0 <= x' < w AFTER the truncation toward zero (-0.9 -> 0 is kept, as numpy's .astype(int)).
//                          The scatter stores the constant byte 1: collisions are benign and the result is deterministic.
//   xp_aug_random_field    the generator of the noise primitives on its own: Philox4x32-10 per pixel (see aug_philox), uniform
//                          (x >> 8) * 2^-24 or Box-Muller normal sqrt(-2 ln(1 - u0)) cos(2 pi u1).
//   xp_aug_photo_prologue  f64 partial sums of the input images (random_contrast's mean when it is the first primitive) and the 0/1
//                          shade mask: union of rotated ellipses by the analytic inside test in f64.
//   xp_aug_blur            one pass of cv2.GaussianBlur's separable filter, BORDER_REFLECT_101, per-sample kernel size (the radius may
//                          exceed the image).
//   xp_aug_photo_step      step s of every sample's program: the opcode is read per sample (uniform per workgroup), so samples of one
//                          batch run different orders in the same launch.  Every step also writes the f64 partial sums of its output; a
//                          random_contrast step adds the previous step's partials in a fixed order (no float atomics: deterministic and
//                          independent of the batch neighbours).
#include "cv_geom.h"
#include "philox.h"
#include "../../include/xpoint_hip.h"

namespace {

constexpr int AUG_BLOCK = 256;

template <int REFLECT>
__device__ __forceinline__ float aug_tap(const float* __restrict__ src, int H, int W, int sx, int sy) {
    if (REFLECT) return src[(size_t)xp_cv_reflect101(sy, H) * W + xp_cv_reflect101(sx, W)];
    const bool in = (unsigned)sx < (unsigned)W && (unsigned)sy < (unsigned)H;
    return in ? src[(size_t)sy * W + sx] : 0.f;
}

template <int REFLECT>
__global__ __launch_bounds__(256) void aug_warp_kernel(const float* __restrict__ src, float* __restrict__ dst, const double* __restrict__ Hm,
                                                       const uint8_t* __restrict__ warp, uint8_t* __restrict__ mask, int H, int W) {
    __shared__ double s_m[9];
    const int b = blockIdx.z;
    const bool on = warp == nullptr || warp[b] != 0;
    xp_cv_load_map(s_m, Hm + (size_t)b * 9, false, on);
    const int x = xp_tile_x(), y = xp_tile_y();
    if (x >= W || y >= H) return;
    const size_t off = (size_t)b * H * W, pix = (size_t)y * W + x;
    if (!on) {
        dst[off + pix] = src[off + pix];
        if (mask) mask[off + pix] = 1;
        return;
    }
    int X, Y, sx, sy, ax, ay;
    xp_cv_source<32>(s_m, x, y, H, W, X, Y);
    xp_cv_split(X, sx, ax); xp_cv_split(Y, sy, ay);
    const float* s = src + off;
    const float t0 = aug_tap<REFLECT>(s, H, W, sx, sy), t1 = aug_tap<REFLECT>(s, H, W, sx + 1, sy);
    const float t2 = aug_tap<REFLECT>(s, H, W, sx, sy + 1), t3 = aug_tap<REFLECT>(s, H, W, sx + 1, sy + 1);
    dst[off + pix] = xp_cv_bilinear_f32(t0, t1, t2, t3, ax, ay);
}

__global__ __launch_bounds__(256) void aug_scatter_kernel(const uint8_t* __restrict__ kin, uint8_t* __restrict__ kout, const double* __restrict__ Hm,
                                                          const uint8_t* __restrict__ warp, int H, int W) {
    const int b = blockIdx.z;
    const int x = xp_tile_x(), y = xp_tile_y();
    if (x >= W || y >= H) return;
    const size_t off = (size_t)b * H * W;
    if (!kin[off + (size_t)y * W + x]) return;
    if (warp && !warp[b]) { kout[off + (size_t)y * W + x] = 1; return; }
    const double* m = Hm + (size_t)b * 9;
    const double xd = (double)x, yd = (double)y;
    const double Xn = (m[0] * xd + m[1] * yd) + m[2];
    const double Yn = (m[3] * xd + m[4] * yd) + m[5];
    const double Wn = (m[6] * xd + m[7] * yd) + m[8];
    const double tx = trunc(Xn / Wn), ty = trunc(Yn / Wn);          // NaN / inf fail the comparisons below
    if (tx >= 0.0 && tx < (double)W && ty >= 0.0 && ty < (double)H) kout[off + (size_t)(int)ty * W + (int)tx] = 1;
}

// aug_philox / aug_uniform: philox.h (Philox4x32-10, shared with the training dropout)
__device__ __forceinline__ float aug_normal(const AugU4& r) {
    const float u0 = aug_uniform(r.x), u1 = aug_uniform(r.y);
    return sqrtf(-2.f * logf(1.f - u0)) * cosf(6.28318530717958647692f * u1);
}

__global__ __launch_bounds__(AUG_BLOCK) void aug_field_kernel(float* __restrict__ out, uint64_t seed, const int* __restrict__ ids, int primitive,
                                                              int kind, int npix) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * AUG_BLOCK + threadIdx.x;
    if (p >= npix) return;
    const AugU4 r = aug_philox(seed, (uint32_t)ids[b], (uint32_t)primitive, (uint32_t)p);
    out[(size_t)b * npix + p] = kind == XP_AUG_FIELD_UNIFORM ? aug_uniform(r.x) : aug_normal(r);
}

// sum of v over the workgroup in a fixed order (LDS tree); every thread calls it, thread 0 holds the result
__device__ __forceinline__ double aug_block_sum(double v, double* s_red) {
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int n = AUG_BLOCK / 2; n > 0; n >>= 1) {
        if ((int)threadIdx.x < n) s_red[threadIdx.x] = s_red[threadIdx.x] + s_red[threadIdx.x + n];
        __syncthreads();
    }
    return s_red[0];
}

// ellipses: (B, NE, 6) f64 = centre x, centre y, half axis a, half axis b, cos(angle), sin(angle)
__global__ __launch_bounds__(AUG_BLOCK) void aug_prologue_kernel(const float* __restrict__ img, double* __restrict__ partials,
                                                                 const double* __restrict__ ellipses, float* __restrict__ shade, int NE, int H,
                                                                 int W) {
    __shared__ double s_red[AUG_BLOCK];
    const int b = blockIdx.y, npix = H * W;
    const int p = blockIdx.x * AUG_BLOCK + threadIdx.x;
    const bool in = p < npix;
    const double v = in ? (double)img[(size_t)b * npix + p] : 0.0;
    const double sum = aug_block_sum(v, s_red);
    if (threadIdx.x == 0) partials[(size_t)b * gridDim.x + blockIdx.x] = sum;
    if (!shade || !in) return;
    const double xd = (double)(p % W), yd = (double)(p / W);
    float m = 0.f;
    for (int e = 0; e < NE; ++e) {
        const double* q = ellipses + ((size_t)b * NE + e) * 6;
        const double dx = xd - q[0], dy = yd - q[1];
        const double u = (dx * q[4] + dy * q[5]) / q[2], w = (dy * q[4] - dx * q[5]) / q[3];
        if (u * u + w * w <= 1.0) m = 1.f;
    }
    shade[(size_t)b * npix + p] = m;
}

template <int VERTICAL>
__global__ __launch_bounds__(256) void aug_blur_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ weights,
                                                       const int* __restrict__ ksizes, int KMAX, int H, int W) {
    const int b = blockIdx.z;
    const int x = xp_tile_x(), y = xp_tile_y();
    if (x >= W || y >= H) return;
    const float* s = src + (size_t)b * H * W;
    const float* wt = weights + (size_t)b * KMAX;
    const int ks = min(max(ksizes[b], 1), KMAX), r = ks / 2;
    float acc = 0.f;
    for (int d = 0; d < ks; ++d) {
        const float t = VERTICAL ? s[(size_t)xp_cv_reflect101(y + d - r, H) * W + x] : s[(size_t)y * W + xp_cv_reflect101(x + d - r, W)];
        acc = acc + wt[d] * t;
    }
    dst[((size_t)b * H + y) * W + x] = acc;
}

struct AugStepParams {
    const float* src; float* dst;
    const int* ops; const float* params;            // (B, S) opcode / scalar of each step
    const double* part_in; double* part_out;        // (B, nblk) partial sums of src / of dst
    const float* shade;                             // (B, H, W) blurred shade mask
    const float* motion;                            // (B, 121) motion-blur kernels, row-major ksize x ksize
    const float* field_gauss; const float* field_speckle;   // injected fields, or null: generated
    const int* ids;
    uint64_t seed;
    int step, S, H, W;
};

__device__ __forceinline__ float aug_clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__global__ __launch_bounds__(AUG_BLOCK) void aug_step_kernel(AugStepParams q) {
    __shared__ double s_red[AUG_BLOCK];
    const int b = blockIdx.y, npix = q.H * q.W, nblk = gridDim.x;
    const int p = blockIdx.x * AUG_BLOCK + threadIdx.x;
    const bool in = p < npix;
    const int op = q.ops[(size_t)b * q.S + q.step];
    const float par = q.params[(size_t)b * q.S + q.step];
    const float* s = q.src + (size_t)b * npix;
    float v = in ? s[p] : 0.f;
    if (op == XP_AUG_GAUSSIAN_NOISE) {
        if (in) {
            const float z = q.field_gauss ? q.field_gauss[(size_t)b * npix + p] : aug_normal(aug_philox(q.seed, (uint32_t)q.ids[b], (uint32_t)op, (uint32_t)p));
            v = aug_clip01(v + par * z);
        }
    } else if (op == XP_AUG_SPECKLE_NOISE) {
        if (in) {
            const float u = q.field_speckle ? q.field_speckle[(size_t)b * npix + p] : aug_uniform(aug_philox(q.seed, (uint32_t)q.ids[b], (uint32_t)op, (uint32_t)p).x);
            if (u < par) v = 0.f;
            if (u > 1.f - par) v = 1.f;
        }
    } else if (op == XP_AUG_BRIGHTNESS) {
        v = aug_clip01(v + par);
    } else if (op == XP_AUG_CONTRAST) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < nblk; i += AUG_BLOCK) acc = acc + q.part_in[(size_t)b * nblk + i];
        const double total = aug_block_sum(acc, s_red);
        __syncthreads();                            // s_red is reused below
        const float mean = (float)(total / (double)npix);
        v = aug_clip01((v - mean) * par + mean);
    } else if (op == XP_AUG_SHADE && q.shade) {
        if (in) v = aug_clip01(v * (1.f - par * q.shade[(size_t)b * npix + p]));
    } else if (op == XP_AUG_MOTION_BLUR && q.motion) {
        if (in) {
            const int ks = min(max((int)par, 1), 11), r = ks / 2, x = p % q.W, y = p / q.W;       // the table row holds 11 x 11
            const float* k = q.motion + (size_t)b * 121;
            float acc = 0.f;
            for (int dy = 0; dy < ks; ++dy) {
                const int yy = xp_cv_reflect101(y + dy - r, q.H);
                for (int dx = 0; dx < ks; ++dx) {
                    const float wgt = k[dy * ks + dx];
                    if (wgt != 0.f) acc = acc + wgt * s[(size_t)yy * q.W + xp_cv_reflect101(x + dx - r, q.W)];
                }
            }
            v = acc;
        }
    }
    if (in) q.dst[(size_t)b * npix + p] = v;
    const double sum = aug_block_sum(in ? (double)v : 0.0, s_red);
    if (threadIdx.x == 0) q.part_out[(size_t)b * nblk + blockIdx.x] = sum;
}

bool aug_shape_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H > 0 && W > 0 && H < 32768 && W < 32768 && (int64_t)H * W <= (1 << 30); }

}  // namespace

extern "C" int xp_aug_partials_per_sample(int H, int W) {
    if (H <= 0 || W <= 0 || (int64_t)H * W > (1 << 30)) return 0;
    return xp_cdiv((int64_t)H * W, AUG_BLOCK);
}

extern "C" int xp_aug_warp(const float* src, float* dst, const double* Hm, const uint8_t* warp, uint8_t* mask, int B, int H, int W,
                           int border_reflect, void* stream) {
    XP_CHECK_ARG(src && dst && Hm, "xp_aug_warp: null pointer");
    XP_CHECK_ARG(aug_shape_ok(B, H, W), "xp_aug_warp: bad shape (%d images of %d x %d)", B, H, W);
    XP_CHECK_ARG(((uintptr_t)Hm & 7) == 0 && ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0, "xp_aug_warp: misaligned pointer");
    XP_CHECK_ARG(src != dst, "xp_aug_warp: in-place warp is not supported");
    const dim3 grid = xp_tile_grid(W, H, B), block(256);
    XpProfScope prof("aug_warp", (hipStream_t)stream, 0.0, (double)B * H * W * (mask ? 9.0 : 8.0));
    if (border_reflect) hipLaunchKernelGGL(aug_warp_kernel<1>, grid, block, 0, (hipStream_t)stream, src, dst, Hm, warp, mask, H, W);
    else hipLaunchKernelGGL(aug_warp_kernel<0>, grid, block, 0, (hipStream_t)stream, src, dst, Hm, warp, mask, H, W);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_aug_scatter_labels(const uint8_t* kp_in, uint8_t* kp_out, const double* Hm, const uint8_t* warp, int B, int H, int W, void* stream) {
    XP_CHECK_ARG(kp_in && kp_out && Hm, "xp_aug_scatter_labels: null pointer");
    XP_CHECK_ARG(aug_shape_ok(B, H, W), "xp_aug_scatter_labels: bad shape (%d maps of %d x %d)", B, H, W);
    XP_CHECK_ARG(((uintptr_t)Hm & 7) == 0, "xp_aug_scatter_labels: misaligned matrix pointer");
    XP_CHECK_ARG(kp_in != kp_out, "xp_aug_scatter_labels: in-place scatter is not supported");
    const dim3 grid = xp_tile_grid(W, H, B), block(256);
    XpProfScope prof("aug_scatter_labels", (hipStream_t)stream, 0.0, (double)B * H * W * 2.0);
    XP_HIP(hipMemsetAsync(kp_out, 0, (size_t)B * H * W, (hipStream_t)stream));
    hipLaunchKernelGGL(aug_scatter_kernel, grid, block, 0, (hipStream_t)stream, kp_in, kp_out, Hm, warp, H, W);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_aug_random_field(float* out, unsigned long long seed, const int* sample_ids, int primitive, int kind, int B, int npix, void* stream) {
    XP_CHECK_ARG(out && sample_ids, "xp_aug_random_field: null pointer");
    XP_CHECK_ARG(B > 0 && B <= 65535 && npix > 0 && npix <= (1 << 30), "xp_aug_random_field: bad shape (%d fields of %d)", B, npix);
    XP_CHECK_ARG(primitive >= 0 && primitive <= XP_SYNTH_KEY_TEXTURE, "xp_aug_random_field: primitive must be 0..%d, got %d", XP_SYNTH_KEY_TEXTURE,
                 primitive);
    XP_CHECK_ARG(kind == XP_AUG_FIELD_UNIFORM || kind == XP_AUG_FIELD_NORMAL, "xp_aug_random_field: unknown kind %d", kind);
    const dim3 grid(xp_cdiv(npix, AUG_BLOCK), B), block(AUG_BLOCK);
    XpProfScope prof("aug_random_field", (hipStream_t)stream, 0.0, 4.0 * B * npix);
    hipLaunchKernelGGL(aug_field_kernel, grid, block, 0, (hipStream_t)stream, out, (uint64_t)seed, sample_ids, primitive, kind, npix);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_aug_photo_prologue(const float* images, double* partials, const double* ellipses, float* shade, int n_ellipses, int B, int H, int W,
                                     void* stream) {
    XP_CHECK_ARG(images && partials, "xp_aug_photo_prologue: null pointer");
    XP_CHECK_ARG(!shade || (ellipses && n_ellipses >= 0), "xp_aug_photo_prologue: a shade mask needs the ellipse table");
    XP_CHECK_ARG(aug_shape_ok(B, H, W), "xp_aug_photo_prologue: bad shape (%d images of %d x %d)", B, H, W);
    XP_CHECK_ARG(((uintptr_t)partials & 7) == 0 && ((uintptr_t)ellipses & 7) == 0, "xp_aug_photo_prologue: misaligned pointer");
    const dim3 grid(xp_cdiv((int64_t)H * W, AUG_BLOCK), B), block(AUG_BLOCK);
    XpProfScope prof("aug_photo_prologue", (hipStream_t)stream, 0.0, (double)B * H * W * (shade ? 8.0 : 4.0));
    hipLaunchKernelGGL(aug_prologue_kernel, grid, block, 0, (hipStream_t)stream, images, partials, ellipses, shade, n_ellipses, H, W);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_aug_blur(const float* src, float* dst, const float* weights, const int* ksizes, int kmax, int B, int H, int W, int vertical,
                           void* stream) {
    XP_CHECK_ARG(src && dst && weights && ksizes, "xp_aug_blur: null pointer");
    XP_CHECK_ARG(aug_shape_ok(B, H, W) && H <= 4 * 65535, "xp_aug_blur: bad shape (%d images of %d x %d)", B, H, W);
    XP_CHECK_ARG(kmax >= 1, "xp_aug_blur: bad weight-table width %d", kmax);
    XP_CHECK_ARG(src != dst, "xp_aug_blur: in-place filtering is not supported");
    const dim3 grid = xp_tile_grid(W, H, B), block(256);
    XpProfScope prof("aug_blur", (hipStream_t)stream, 2.0 * kmax * B * H * W, 8.0 * B * H * W);
    if (vertical) hipLaunchKernelGGL(aug_blur_kernel<1>, grid, block, 0, (hipStream_t)stream, src, dst, weights, ksizes, kmax, H, W);
    else hipLaunchKernelGGL(aug_blur_kernel<0>, grid, block, 0, (hipStream_t)stream, src, dst, weights, ksizes, kmax, H, W);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_aug_photo_step(const float* src, float* dst, const int* ops, const float* params, int step, int n_steps, const double* partials_in,
                                 double* partials_out, const float* shade, const float* motion_kernels, const float* field_gauss,
                                 const float* field_speckle, unsigned long long seed, const int* sample_ids, int B, int H, int W, void* stream) {
    XP_CHECK_ARG(src && dst && ops && params && partials_in && partials_out && sample_ids, "xp_aug_photo_step: null pointer");
    XP_CHECK_ARG(aug_shape_ok(B, H, W), "xp_aug_photo_step: bad shape (%d images of %d x %d)", B, H, W);
    XP_CHECK_ARG(n_steps > 0 && step >= 0 && step < n_steps, "xp_aug_photo_step: step %d of %d", step, n_steps);
    XP_CHECK_ARG(src != dst && partials_in != partials_out, "xp_aug_photo_step: the step reads one buffer and writes the other");
    XP_CHECK_ARG(((uintptr_t)partials_in & 7) == 0 && ((uintptr_t)partials_out & 7) == 0, "xp_aug_photo_step: misaligned pointer");
    // the opcodes live on the device (per sample): the tables a program MAY need are demanded by the caller's primitive set, checked in Python
    AugStepParams q{src, dst, ops, params, partials_in, partials_out, shade, motion_kernels, field_gauss, field_speckle, sample_ids,
                    (uint64_t)seed, step, n_steps, H, W};
    const dim3 grid(xp_cdiv((int64_t)H * W, AUG_BLOCK), B), block(AUG_BLOCK);
    XpProfScope prof("aug_photo_step", (hipStream_t)stream, 0.0, 8.0 * B * H * W);
    hipLaunchKernelGGL(aug_step_kernel, grid, block, 0, (hipStream_t)stream, q);
    XP_LAUNCH_CHECK();
    return XP_OK;
}
