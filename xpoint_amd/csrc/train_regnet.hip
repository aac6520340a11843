// Element-wise and per-sample kernels of the homography head's training (reference xpoint/models/RegNet.py; xpoint_amd/training.py RegNetHead;
// DESIGN.md §15).  The head's order is conv -> BatchNorm -> ReLU, so the ReLU gates read the BatchNorm OUTPUT (the heads' trunk is conv -> ReLU ->
// BatchNorm and gates inside xp_bn_train_bwd).  The dense work — both zero-padded convolutions' weight and input gradients — is in train_dense.hip and train_dgrad.hip.
//
//   xp_relu_fwd / xp_relu_bwd   y = max(x, 0);  dy = dr where y > 0, else 0.
//   xp_maxpool2_relu_bwd        backward of MaxPool2d(2)(ReLU(y)) as torch computes it: the gradient of a window goes to the FIRST position (row-major
//                               inside the window) that attains the window's maximum, if that maximum is > 0; everything else, the trailing row /
//                               column of an odd H / W included, gets 0.
//   xp_costvolume_mean_bwd      backward of xp_costvolume_mean (v[n][p] = a[n][p] . mean_q b[n][q]); the sums over positions run in ascending order.
//   xp_dropout_rows             nn.Dropout(p) over (rows, C): Philox4x32-10 draws keyed by (seed, sample id, tag), the column is the counter.
// Nothing here uses an atomic: two calls are bit-identical.
#include "philox.h"
#include "xp_common.h"
#include "xpoint_hip.h"

namespace {

__global__ __launch_bounds__(256) void rn_relu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = fmaxf(x[i], 0.f);
}
__global__ __launch_bounds__(256) void rn_relu_bwd_kernel(const float* __restrict__ dr, const float* __restrict__ y, float* __restrict__ dy, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dy[i] = y[i] > 0.f ? dr[i] : 0.f;
}

// one thread per (window, channel) over the ceil(H / 2) x ceil(W / 2) windows that cover the map; a window cut by the edge has no pooled output
__global__ __launch_bounds__(256) void rn_maxpool2_relu_bwd_kernel(const float* __restrict__ dpool, const float* __restrict__ y, float* __restrict__ dy,
                                                                   int B, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    const int64_t total = (int64_t)B * Hc * Wc * C;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const int64_t win = idx / C;
    const int ow = (int)(win % Wc), oh = (int)((win / Wc) % Hc);
    const int64_t b = win / ((int64_t)Wc * Hc);
    const int64_t base = ((b * H + 2 * oh) * W + 2 * ow) * (int64_t)C + c;
    const int64_t off[4] = {0, C, (int64_t)W * C, (int64_t)W * C + C};
    if (oh < Ho && ow < Wo) {
        int arg = 0;
        float best = y[base];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float v = y[base + off[k]];
            if (v > best) { best = v; arg = k; }              // strict: a tie stays with the first index
        }
        const float g = best > 0.f ? dpool[((b * Ho + oh) * Wo + ow) * (int64_t)C + c] : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) dy[base + off[k]] = k == arg ? g : 0.f;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = 2 * oh + (k >> 1) < H && 2 * ow + (k & 1) < W;
            if (in) dy[base + off[k]] = 0.f;
        }
    }
}

// One workgroup per sample.  m[c] = mean_q b[q][c] (as the forward forms it) and s[c] = (sum_p dv[p] a[p][c]) / hw, a thread per channel with the
// positions in ascending order; then da[p][c] = dv[p] m[c] and db[q][c] = s[c].
__global__ __launch_bounds__(256) void rn_costvolume_mean_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ dv,
                                                                     float* __restrict__ da, float* __restrict__ db, int hw, int C) {
    extern __shared__ float s_ms[];                       // m (C floats), then s (C floats)
    const int n = blockIdx.x;
    const float* aa = a + (int64_t)n * hw * C;
    const float* bb = b + (int64_t)n * hw * C;
    const float* dvn = dv + (int64_t)n * hw;
    for (int c = threadIdx.x; c < C; c += 256) {
        float m = 0.f, s = 0.f;
        for (int q = 0; q < hw; ++q) { m += bb[(int64_t)q * C + c]; s = fmaf(dvn[q], aa[(int64_t)q * C + c], s); }
        s_ms[c] = m / (float)hw;
        s_ms[C + c] = s / (float)hw;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p = wave; p < hw; p += 4) {
        const float g = dvn[p];
        const int64_t row = ((int64_t)n * hw + p) * C;
        for (int c = lane; c < C; c += 64) { da[row + c] = g * s_ms[c]; db[row + c] = s_ms[C + c]; }
    }
}

__global__ __launch_bounds__(256) void rn_dropout_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ mask, int use_mask,
                                                         uint64_t seed, const int* __restrict__ ids, int tag, float p, float inv_keep, int C) {
    const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t i = (int64_t)r * C + c;
    bool keep;
    if (use_mask) {
        keep = mask[i] != 0;
    } else {
        keep = aug_uniform(aug_philox(seed, (uint32_t)ids[r], (uint32_t)tag, (uint32_t)c).x) >= p;
        if (mask) mask[i] = keep ? 1 : 0;
    }
    y[i] = keep ? x[i] * inv_keep : 0.f;
}

int rn_grid(int64_t n) { return (int)(n < (int64_t)256 * 65536 ? (n + 255) / 256 : 65536); }

}  // namespace

extern "C" int xp_relu_fwd(const float* x, float* y, int64_t n, void* stream) {
    XP_CHECK_ARG(x && y && n > 0, "xp_relu_fwd: null pointer or n <= 0");
    XpProfScope prof("relu_fwd", (hipStream_t)stream, 0.0, 8.0 * n);
    hipLaunchKernelGGL(rn_relu_fwd_kernel, dim3(rn_grid(n)), dim3(256), 0, (hipStream_t)stream, x, y, n);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_relu_bwd(const float* dr, const float* y, float* dy, int64_t n, void* stream) {
    XP_CHECK_ARG(dr && y && dy && n > 0, "xp_relu_bwd: null pointer or n <= 0");
    XpProfScope prof("relu_bwd", (hipStream_t)stream, 0.0, 12.0 * n);
    hipLaunchKernelGGL(rn_relu_bwd_kernel, dim3(rn_grid(n)), dim3(256), 0, (hipStream_t)stream, dr, y, dy, n);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_maxpool2_relu_bwd(const float* dpool, const float* y, float* dy, int batch, int H, int W, int C, void* stream) {
    XP_CHECK_ARG(y && dy && batch > 0 && H > 0 && W > 0 && C > 0, "xp_maxpool2_relu_bwd: null pointer or bad shape batch=%d H=%d W=%d C=%d", batch, H, W, C);
    XP_CHECK_ARG(dpool || H < 2 || W < 2, "xp_maxpool2_relu_bwd: null pointer");
    const int64_t total = (int64_t)batch * ((H + 1) / 2) * ((W + 1) / 2) * C;
    XP_CHECK_ARG(total < (int64_t)256 * 0x7fffffff, "xp_maxpool2_relu_bwd: shape too large");
    XpProfScope prof("maxpool2_relu_bwd", (hipStream_t)stream, 0.0, 36.0 * total);
    hipLaunchKernelGGL(rn_maxpool2_relu_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dpool, y, dy, batch, H, W, C);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_costvolume_mean_bwd(const float* a, const float* b, const float* dv, float* da, float* db, int batch, int hw, int C, void* stream) {
    XP_CHECK_ARG(a && b && dv && da && db, "xp_costvolume_mean_bwd: null pointer");
    XP_CHECK_ARG(batch > 0 && hw > 0 && C > 0 && C <= 4096, "xp_costvolume_mean_bwd: bad shape batch %d, hw %d, C %d", batch, hw, C);
    XpProfScope prof("costvolume_mean_bwd", (hipStream_t)stream, 4.0 * batch * hw * (double)C, 16.0 * batch * hw * (double)C);
    hipLaunchKernelGGL(rn_costvolume_mean_bwd_kernel, dim3(batch), dim3(256), (size_t)2 * C * sizeof(float), (hipStream_t)stream, a, b, dv, da, db, hw, C);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_dropout_rows(const float* x, float* y, unsigned char* mask, int use_mask, unsigned long long seed, const int* sample_ids, int tag, float p,
                               int rows, int C, void* stream) {
    XP_CHECK_ARG(x && y && rows > 0 && rows <= 65535 && C > 0, "xp_dropout_rows: null pointer or bad shape rows=%d C=%d (rows <= 65535)", rows, C);
    XP_CHECK_ARG(p >= 0.f && p < 1.f, "xp_dropout_rows: p must lie in [0, 1), got %g", (double)p);
    XP_CHECK_ARG(use_mask ? mask != nullptr : sample_ids != nullptr, "xp_dropout_rows: %s", use_mask ? "use_mask needs a mask" : "drawing a mask needs sample_ids");
    XP_CHECK_ARG(tag >= 0 && tag < 8, "xp_dropout_rows: tag must lie in 0..7 (the key holds sample id * 8 + tag), got %d", tag);
    XpProfScope prof("dropout_rows", (hipStream_t)stream, 0.0, 9.0 * rows * (double)C);
    hipLaunchKernelGGL(rn_dropout_kernel, dim3(xp_cdiv(C, 256), rows), dim3(256), 0, (hipStream_t)stream, x, y, mask, use_mask, (uint64_t)seed, sample_ids, tag,
                       p, 1.f / (1.f - p), C);
    XP_LAUNCH_CHECK();
    return XP_OK;
}
