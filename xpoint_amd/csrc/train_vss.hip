// Glue backward kernels of VSS-block training (reference VMamba.py:1153-1234, SS2D forwardv2 / forward_corev2; xpoint_amd/training.py VSSBlock;
// DESIGN.md §16).  The block's dense work runs on the engines of §14 (xp_gemm_nt_h2, xp_gemm_tn_h2, xp_colsum_rows) and its SS2D core on the
// differentiable scan / cross-scan / cross-merge operators of §10; what is here is HBM-bound:
//
//   xp_layernorm_bwd         backward of xp_layernorm: the row statistics are recomputed with the forward's lane geometry and arithmetic (the same bits),
//                            dx per row, dgamma / dbeta by the fixed-order column sums of train_rows.h.
//   xp_dwconv3x3_silu_bwd    backward of xp_dwconv3x3_silu: dz (the gradient of the convolution's output, z recomputed) goes to the workspace, dx is the
//                            mirrored-tap convolution of dz, dw the nine per-channel sums of dz x_shifted(tap).
//   xp_gelu_fwd / _bwd       the GEMM epilogue's GELU (xp_gelu_fast) as a launch of its own, and dy (Phi(x) + x phi(x)).
//   xp_add_scaled_rows       y = x + s[b] r: the residual add under stochastic depth; x = NULL: s[b] r, its backward.
// dx_scale follows xp_bn_train_bwd: a device float[2] that receives {S, 1 / S}, dx is written as S x the gradient (xp_scale_grad, train_dense.hip).
// Nothing here uses an atomic: every cross-row sum runs in a fixed order with f64 accumulators, two calls are bit-identical.
#include "train_rows.h"
#include "train_scale.h"
#include "xpoint_hip.h"

namespace {

// xp_scale_grad's workspace (XP_SCALE_HEAD_BYTES, train_scale.h) is at the head of every workspace here

__device__ __forceinline__ double vs_group_sum(double v, int lpr) {
    for (int o = lpr / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- LayerNorm backward: the lane geometry of layernorm_vec_kernel (elementwise.hip): LPR lanes share a row, each owns NV float4s ----
template <int LPR, int NV>
__global__ __launch_bounds__(256) void vs_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                                                        float* __restrict__ dx, float2* __restrict__ stat, int64_t M, int C, float eps) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, sub = lane % LPR;
    const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
    const bool rok = row < M;
    const int C4 = C >> 2;
    const float4* xr = reinterpret_cast<const float4*>(x + (rok ? row : 0) * C);
    const float4* gr = reinterpret_cast<const float4*>(dy + (rok ? row : 0) * C);
    float4 v[NV], g[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = sub + i * LPR;
        v[i] = (c4 < C4) ? xr[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
        g[i] = (c4 < C4) ? gr[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // mean and rstd: the forward's sequence, operation for operation
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (sub + i * LPR < C4) {
            const float ax = v[i].x - mean, ay = v[i].y - mean, az = v[i].z - mean, aw = v[i].w - mean;
            q = fmaf(ax, ax, q); q = fmaf(ay, ay, q); q = fmaf(az, az, q); q = fmaf(aw, aw, q);
        }
    }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.f / sqrtf(q / (float)C + eps);
    // g = gamma dy; xhat = (x - mean) rstd, the forward's xhat; the two row sums in f64 (lanes, then the butterfly: a fixed order)
    double sg = 0.0, sgx = 0.0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = sub + i * LPR;
        if (c4 < C4) {
            const float4 gm = reinterpret_cast<const float4*>(gamma)[c4];
            g[i].x *= gm.x; g[i].y *= gm.y; g[i].z *= gm.z; g[i].w *= gm.w;
            v[i].x = (v[i].x - mean) * rstd; v[i].y = (v[i].y - mean) * rstd; v[i].z = (v[i].z - mean) * rstd; v[i].w = (v[i].w - mean) * rstd;
            sg += ((double)g[i].x + (double)g[i].y) + ((double)g[i].z + (double)g[i].w);
            sgx += ((double)g[i].x * (double)v[i].x + (double)g[i].y * (double)v[i].y) + ((double)g[i].z * (double)v[i].z + (double)g[i].w * (double)v[i].w);
        }
    }
    const double mg = vs_group_sum(sg, LPR) / (double)C, mgx = vs_group_sum(sgx, LPR) / (double)C;
    if (!rok) return;
    if (sub == 0) stat[row] = make_float2(mean, rstd);
    float4* dr = reinterpret_cast<float4*>(dx + row * C);
    const double rs = (double)rstd;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = sub + i * LPR;
        if (c4 < C4) {
            // the bracket in f64: its three terms cancel
            float4 o;
            o.x = (float)(rs * ((double)g[i].x - mg - (double)v[i].x * mgx)); o.y = (float)(rs * ((double)g[i].y - mg - (double)v[i].y * mgx));
            o.z = (float)(rs * ((double)g[i].z - mg - (double)v[i].z * mgx)); o.w = (float)(rs * ((double)g[i].w - mg - (double)v[i].w * mgx));
            dr[c4] = o;
        }
    }
}

// dbeta = sum_r dy, dgamma = sum_r dy xhat, xhat from the row statistics the dx kernel left
__global__ __launch_bounds__(256) void vs_ln_param_parts_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float2* __restrict__ stat,
                                                                int64_t rows, int C, double* __restrict__ part) {
    td_colsum_parts<2>(rows, C, part, [&](int64_t r, int c, double (&a)[2]) {
        const float2 st = stat[r];
        const float g = dy[r * C + c], xh = (x[r * C + c] - st.x) * st.y;
        a[0] += (double)g; a[1] += (double)g * (double)xh;
    });
}
__global__ __launch_bounds__(256) void vs_ln_param_finish_kernel(const double* __restrict__ part, int C, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    if (dbeta) dbeta[c] = (float)td_sum_parts(part, 2, 0, C, c);
    if (dgamma) dgamma[c] = (float)td_sum_parts(part, 2, 1, C, c);
}

// ---- depthwise 3x3 + SiLU backward: one thread per (pixel, 4 channels) ----
// dz = dy sigma(z) (1 + z (1 - sigma(z))), z = the forward's convolution (taps in (kh, kw) order, a tap outside the image skipped)
__global__ __launch_bounds__(256) void vs_dw_dz_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ dy,
                                                       float* __restrict__ dz, int B, int H, int W, int C) {
    const int C4 = C >> 2;
    const int64_t total = (int64_t)B * H * W * C4;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    const int64_t pix = idx / C4;
    const int px = (int)(pix % W), py = (int)((pix / W) % H);
    const int64_t b = pix / ((int64_t)W * H);
    const float4* xv = reinterpret_cast<const float4*>(x);
    const float4* wv = reinterpret_cast<const float4*>(w);
    float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int iy = py + kh - 1;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ix = px + kw - 1;
            if (ix < 0 || ix >= W) continue;
            const float4 a = xv[((b * H + iy) * W + ix) * C4 + c4], t = wv[(kh * 3 + kw) * C4 + c4];
            z.x = fmaf(a.x, t.x, z.x); z.y = fmaf(a.y, t.y, z.y); z.z = fmaf(a.z, t.z, z.z); z.w = fmaf(a.w, t.w, z.w);
        }
    }
    const float4 g = reinterpret_cast<const float4*>(dy)[idx];
    auto dsilu = [](float zz, float gg) { const float sg = 1.f / (1.f + expf(-zz)); return gg * sg * (1.f + zz * (1.f - sg)); };
    reinterpret_cast<float4*>(dz)[idx] = make_float4(dsilu(z.x, g.x), dsilu(z.y, g.y), dsilu(z.z, g.z), dsilu(z.w, g.w));
}
// dx[y][x] = sum over taps of dz[y + 1 - kh][x + 1 - kw] w[kh][kw]: output pixel (yo, xo) read input (yo + kh - 1, xo + kw - 1).  An output pixel outside
// the image does not exist, and b never changes: nothing crosses a sample boundary
__global__ __launch_bounds__(256) void vs_dw_dx_kernel(const float* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dx, int B, int H,
                                                       int W, int C) {
    const int C4 = C >> 2;
    const int64_t total = (int64_t)B * H * W * C4;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    const int64_t pix = idx / C4;
    const int px = (int)(pix % W), py = (int)((pix / W) % H);
    const int64_t b = pix / ((int64_t)W * H);
    const float4* zv = reinterpret_cast<const float4*>(dz);
    const float4* wv = reinterpret_cast<const float4*>(w);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int oy = py + 1 - kh;
        if (oy < 0 || oy >= H) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ox = px + 1 - kw;
            if (ox < 0 || ox >= W) continue;
            const float4 a = zv[((b * H + oy) * W + ox) * C4 + c4], t = wv[(kh * 3 + kw) * C4 + c4];
            o.x = fmaf(a.x, t.x, o.x); o.y = fmaf(a.y, t.y, o.y); o.z = fmaf(a.z, t.z, o.z); o.w = fmaf(a.w, t.w, o.w);
        }
    }
    reinterpret_cast<float4*>(dx)[idx] = o;
}
// dw[t][c] = sum over (b, y, x) of dz x_shifted(t): nine sums per channel by the fixed-order reduction.  blockIdx.z = the tap row kh: three sums per
// thread instead of nine — three times the workgroups and a third of the accumulator registers; the order of every sum is unchanged
__global__ __launch_bounds__(256) void vs_dw_dw_parts_kernel(const float* __restrict__ dz, const float* __restrict__ x, int64_t rows, int H, int W, int C,
                                                             double* __restrict__ part) {
    const int kh = blockIdx.z;
    td_colsum_parts<3>(rows, C, part + (size_t)kh * BN_PARTS * 3 * C, [&](int64_t r, int c, double (&a)[3]) {
        const int px = (int)(r % W), iy = (int)((r / W) % H) + kh - 1;
        if (iy < 0 || iy >= H) return;
        const double d = (double)dz[r * C + c];
        const float* xr = x + (r + (int64_t)(kh - 1) * W) * C + c;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ix = px + kw - 1;
            if (ix >= 0 && ix < W) a[kw] += d * (double)xr[(kw - 1) * C];
        }
    });
}
__global__ __launch_bounds__(256) void vs_dw_dw_finish_kernel(const double* __restrict__ part, int C, float* __restrict__ dw) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 9 * C) return;
    const int t = idx / C, c = idx - t * C;
    dw[idx] = (float)td_sum_parts(part + (size_t)(t / 3) * BN_PARTS * 3 * C, 3, t % 3, C, c);
}

// ---- element-wise: 16-byte accesses over the aligned body, scalar over the tail ----
template <class F4, class F1>
__device__ __forceinline__ void vs_elementwise(int64_t n, bool vec, F4 f4, F1 f1) {
    const int64_t n4 = vec ? n >> 2 : 0;
    const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = t0; i < n4; i += stride) f4(i);
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) f1(i);
}
__global__ __launch_bounds__(256) void vs_gelu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int vec) {
    vs_elementwise(n, vec != 0,
        [&](int64_t i) {
            const float4 v = reinterpret_cast<const float4*>(x)[i];
            reinterpret_cast<float4*>(y)[i] = make_float4(xp_gelu_fast(v.x), xp_gelu_fast(v.y), xp_gelu_fast(v.z), xp_gelu_fast(v.w));
        },
        [&](int64_t i) { y[i] = xp_gelu_fast(x[i]); });
}
// d/dx [x Phi(x)] = Phi(x) + x phi(x); Phi through erfc: no cancellation on the negative side
__device__ __forceinline__ float vs_dgelu(float x, float g) {
    const float cdf = 0.5f * erfcf(x * -0.70710678118654752440f);
    const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
    return g * (cdf + x * pdf);
}
__global__ __launch_bounds__(256) void vs_gelu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, int64_t n,
                                                          int vec) {
    vs_elementwise(n, vec != 0,
        [&](int64_t i) {
            const float4 v = reinterpret_cast<const float4*>(x)[i], g = reinterpret_cast<const float4*>(dy)[i];
            reinterpret_cast<float4*>(dx)[i] = make_float4(vs_dgelu(v.x, g.x), vs_dgelu(v.y, g.y), vs_dgelu(v.z, g.z), vs_dgelu(v.w, g.w));
        },
        [&](int64_t i) { dx[i] = vs_dgelu(x[i], dy[i]); });
}
// blockIdx.y = the sample: its factor is one scalar load, no division per element.  x may be NULL (y = s r) and y may alias x or r
__global__ __launch_bounds__(256) void vs_add_scaled_kernel(const float* x, const float* r, const float* __restrict__ s, float* y, int64_t per, int vec) {
    const int64_t base = (int64_t)blockIdx.y * per;
    const float f = s[blockIdx.y];
    vs_elementwise(per, vec != 0,
        [&](int64_t i) {
            const float4 rv = reinterpret_cast<const float4*>(r + base)[i];
            float4 o = make_float4(f * rv.x, f * rv.y, f * rv.z, f * rv.w);
            if (x) { const float4 xv = reinterpret_cast<const float4*>(x + base)[i]; o.x = xv.x + o.x; o.y = xv.y + o.y; o.z = xv.z + o.z; o.w = xv.w + o.w; }
            reinterpret_cast<float4*>(y + base)[i] = o;
        },
        [&](int64_t i) { const float o = f * r[base + i]; y[base + i] = x ? x[base + i] + o : o; });
}

static bool vs_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}
static int vs_elem_blocks(int64_t n) { return (int)min((int64_t)8192, max((int64_t)1, (n / 4 + 255) / 256)); }

static size_t vs_ln_bytes(int64_t rows, int C) {
    if (rows <= 0 || C <= 0) return 0;
    return XP_SCALE_HEAD_BYTES + xp_up256((size_t)BN_PARTS * 2 * C * sizeof(double)) + xp_up256((size_t)rows * sizeof(float2));
}
static size_t vs_dw_bytes(int batch, int H, int W, int C) {
    if (batch <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    return XP_SCALE_HEAD_BYTES + xp_up256((size_t)BN_PARTS * 9 * C * sizeof(double)) + xp_up256((size_t)batch * H * W * C * sizeof(float));
}

}  // namespace

extern "C" size_t xp_layernorm_bwd_workspace_bytes(int64_t rows, int C) { return vs_ln_bytes(rows, C); }

extern "C" int xp_layernorm_bwd(const float* dy, const float* x, const float* gamma, float* dx, float* dgamma, float* dbeta, int64_t rows, int C, float eps,
                                float* dx_scale, void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(dy && x && gamma && dx, "xp_layernorm_bwd: null pointer");
    XP_CHECK_ARG(rows >= 1 && rows < ((int64_t)1 << 31) && C >= 4 && C <= 1024 && C % 4 == 0,
                 "xp_layernorm_bwd: bad shape rows=%lld C=%d (rows >= 1, C a multiple of 4 in [4, 1024])", (long long)rows, C);
    XP_CHECK_ARG(vs_aligned16(dy, x, gamma, dx), "xp_layernorm_bwd: dy, x, gamma and dx must be 16-byte aligned (the forward's vector form)");
    XP_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= vs_ln_bytes(rows, C),
                 "xp_layernorm_bwd: workspace of %zu bytes, 256-byte aligned, needed (got %zu)", vs_ln_bytes(rows, C), workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double* part = (double*)(ws + XP_SCALE_HEAD_BYTES);
    float2* stat = (float2*)(ws + XP_SCALE_HEAD_BYTES + xp_up256((size_t)BN_PARTS * 2 * C * sizeof(double)));
    const int C4 = C / 4;
    {
        XpProfScope prof("layernorm_bwd", s, 0.0, 12.0 * rows * C);
        // xp_layernorm's table: the same LPR x NV for the same C, so the statistics are the forward's bits
#define XP_LNB_LAUNCH(LPR, NV) hipLaunchKernelGGL((vs_ln_bwd_kernel<LPR, NV>), dim3(xp_cdiv(rows, 4 * (64 / LPR))), dim3(256), 0, s, dy, x, gamma, dx, stat, rows, C, eps)
        if (C4 <= 4) XP_LNB_LAUNCH(4, 1);
        else if (C4 <= 8) XP_LNB_LAUNCH(8, 1);
        else if (C4 <= 16) XP_LNB_LAUNCH(16, 1);
        else if (C4 <= 32) XP_LNB_LAUNCH(32, 1);
        else if (C4 <= 64) XP_LNB_LAUNCH(64, 1);
        else if (C4 <= 128) XP_LNB_LAUNCH(64, 2);
        else if (C4 <= 192) XP_LNB_LAUNCH(64, 3);
        else XP_LNB_LAUNCH(64, 4);
#undef XP_LNB_LAUNCH
        XP_LAUNCH_CHECK();
    }
    if (dgamma || dbeta) {
        XpProfScope prof("layernorm_bwd_params", s, 0.0, 8.0 * rows * C);
        hipLaunchKernelGGL(vs_ln_param_parts_kernel, dim3(xp_cdiv(C, 32), BN_PARTS), dim3(256), 0, s, dy, x, stat, rows, C, part);
        XP_LAUNCH_CHECK();
        hipLaunchKernelGGL(vs_ln_param_finish_kernel, dim3(xp_cdiv(C, 256)), dim3(256), 0, s, part, C, dgamma, dbeta);
        XP_LAUNCH_CHECK();
    }
    if (dx_scale) XP_TRY(xp_scale_grad(dx, dx, rows * C, dx_scale, workspace, XP_SCALE_HEAD_BYTES, stream));
    return XP_OK;
}

extern "C" size_t xp_dwconv3x3_silu_bwd_workspace_bytes(int batch, int H, int W, int C) { return vs_dw_bytes(batch, H, W, C); }

extern "C" int xp_dwconv3x3_silu_bwd(const float* x, const float* w9c, const float* dy, float* dx, float* dw9c, int batch, int H, int W, int C,
                                     float* dx_scale, void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(x && w9c && dy && dx, "xp_dwconv3x3_silu_bwd: null pointer");
    XP_CHECK_ARG(batch >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && (int64_t)batch * H * W < ((int64_t)1 << 31) / 16 && C <= (1 << 20),
                 "xp_dwconv3x3_silu_bwd: bad shape batch=%d H=%d W=%d C=%d (C a multiple of 4, H, W >= 1)", batch, H, W, C);
    XP_CHECK_ARG(vs_aligned16(x, w9c, dy, dx), "xp_dwconv3x3_silu_bwd: x, w9c, dy and dx must be 16-byte aligned");
    XP_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= vs_dw_bytes(batch, H, W, C),
                 "xp_dwconv3x3_silu_bwd: workspace of %zu bytes, 256-byte aligned, needed (got %zu)", vs_dw_bytes(batch, H, W, C), workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    double* part = (double*)(ws + XP_SCALE_HEAD_BYTES);
    float* dz = (float*)(ws + XP_SCALE_HEAD_BYTES + xp_up256((size_t)BN_PARTS * 9 * C * sizeof(double)));
    const int64_t rows = (int64_t)batch * H * W, total = rows * (C / 4);
    {
        XpProfScope prof("dwconv3x3_silu_bwd", s, 42.0 * rows * C, 20.0 * rows * C);
        hipLaunchKernelGGL(vs_dw_dz_kernel, dim3(xp_cdiv(total, 256)), dim3(256), 0, s, x, w9c, dy, dz, batch, H, W, C);
        XP_LAUNCH_CHECK();
        hipLaunchKernelGGL(vs_dw_dx_kernel, dim3(xp_cdiv(total, 256)), dim3(256), 0, s, dz, w9c, dx, batch, H, W, C);
        XP_LAUNCH_CHECK();
    }
    if (dw9c) {
        XpProfScope prof("dwconv3x3_silu_bwd_dw", s, 18.0 * rows * C, 8.0 * rows * C);
        hipLaunchKernelGGL(vs_dw_dw_parts_kernel, dim3(xp_cdiv(C, 32), BN_PARTS, 3), dim3(256), 0, s, dz, x, rows, H, W, C, part);
        XP_LAUNCH_CHECK();
        hipLaunchKernelGGL(vs_dw_dw_finish_kernel, dim3(xp_cdiv(9 * C, 256)), dim3(256), 0, s, part, C, dw9c);
        XP_LAUNCH_CHECK();
    }
    if (dx_scale) XP_TRY(xp_scale_grad(dx, dx, rows * C, dx_scale, workspace, XP_SCALE_HEAD_BYTES, stream));
    return XP_OK;
}

extern "C" int xp_gelu_fwd(const float* x, float* y, int64_t n, void* stream) {
    XP_CHECK_ARG(x && y && n > 0, "xp_gelu_fwd: null pointer or n <= 0");
    hipStream_t s = (hipStream_t)stream;
    XpProfScope prof("gelu_fwd", s, 20.0 * n, 8.0 * n);
    hipLaunchKernelGGL(vs_gelu_fwd_kernel, dim3(vs_elem_blocks(n)), dim3(256), 0, s, x, y, n, (int)vs_aligned16(x, y));
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_gelu_bwd(const float* dy, const float* x, float* dx, int64_t n, float* dx_scale, void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(dy && x && dx && n > 0, "xp_gelu_bwd: null pointer or n <= 0");
    XP_CHECK_ARG(!dx_scale || (workspace && workspace_bytes >= XP_SCALE_HEAD_BYTES), "xp_gelu_bwd: dx_scale needs a workspace of %zu bytes", XP_SCALE_HEAD_BYTES);
    hipStream_t s = (hipStream_t)stream;
    {
        XpProfScope prof("gelu_bwd", s, 40.0 * n, 12.0 * n);
        hipLaunchKernelGGL(vs_gelu_bwd_kernel, dim3(vs_elem_blocks(n)), dim3(256), 0, s, dy, x, dx, n, (int)vs_aligned16(dy, x, dx));
        XP_LAUNCH_CHECK();
    }
    if (dx_scale) XP_TRY(xp_scale_grad(dx, dx, n, dx_scale, workspace, workspace_bytes, stream));
    return XP_OK;
}

extern "C" int xp_add_scaled_rows(const float* x, const float* r, const float* s, float* y, int batch, int64_t rows_per_sample, int C, void* stream) {
    XP_CHECK_ARG(r && s && y, "xp_add_scaled_rows: null pointer");
    XP_CHECK_ARG(batch >= 1 && batch <= 65535 && rows_per_sample >= 1 && C >= 1 && rows_per_sample * C < ((int64_t)1 << 40),
                 "xp_add_scaled_rows: bad shape batch=%d rows_per_sample=%lld C=%d (batch <= 65535)", batch, (long long)rows_per_sample, C);
    hipStream_t st = (hipStream_t)stream;
    const int64_t per = rows_per_sample * C;
    const bool vec = per % 4 == 0 && vs_aligned16(x, r, y);
    XpProfScope prof("add_scaled_rows", st, 2.0 * batch * per, (x ? 12.0 : 8.0) * batch * per);
    hipLaunchKernelGGL(vs_add_scaled_kernel, dim3(min(vs_elem_blocks(per), 1024), batch), dim3(256), 0, st, x, r, s, y, per, (int)vec);
    XP_LAUNCH_CHECK();
    return XP_OK;
}
