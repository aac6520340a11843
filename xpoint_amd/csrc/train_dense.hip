// Dense backward kernels of head training: the weight-gradient GEMM on the split-fp16 matrix path, its implicit 3x3 form,
// BatchNorm training forward / backward over NHWC rows, the column sums behind the bias gradients and the L2-normalise backward; at the end of the
// file the zero-padded 3x3 convolution's weight gradient and INPUT gradient of the homography head, the same two for the STRIDE-2 convolutions
// of patch embed and the downsamplers with the stem's weight gradient (encoder training), the INPUT gradient of the head trunk's
// reflection-padded convolution (whole-model training), and xp_scale_grad, the amax / power-of-two
// / scale kernels of the weight gradient as an entry point of their own (VSS-block training).  The row walks and the fixed-order column sums
// are in train_rows.h, which train_vss.hip shares.
//
// Weight gradient.  out[i][j] = sum_m P[m][i] Q[m][j]: the reduction runs over the SLOW dimension of both operands, so a 32-row slab of each is split
// into its two fp16 planes (gemm_h2_core.h) in registers and stored to the LDS in the transposed image — tile row = output row / column, 32 k values
// per plane, the row format of the forward engine (H2_ROWB) — with plain ds_write_b32 stores of two consecutive k; the fragments are then read back as
// rows, exactly as the forward engine reads them.  Three products per multiply on v_mfma_f32_32x32x16_f16, smallest first.
// P is the GRADIENT operand: its elements are not O(1), so it is multiplied by one power of two per call that brings its largest magnitude into
// [2^13, 2^14) (the range the offline weight split uses) and the power is undone, exactly, when the partial sums are added.
// M is cut into chunks of WG_CHUNK rows — a compile-time constant — one workgroup per (tile, chunk); the partial tiles go to the workspace and a second
// kernel adds them in chunk order: no atomics, two calls are bit-identical, and a result does not depend on the device.
#include "gemm_h2_core.h"
#include "train_rows.h"
#include "xpoint_hip.h"

#ifndef XP_TRY
#define XP_TRY(call) do { const int rc__ = (call); if (rc__ != XP_OK) return rc__; } while (0)
#endif

namespace {

constexpr int WG_CHUNK = 256;        // rows of M per partial sum (XP_WGRAD_CHUNK in the header)
constexpr int WG_BT = 64;            // output tile side of a workgroup: 2 x 2 waves of one 32 x 32 accumulator tile
constexpr int AMAX_PARTS = 1024;     // partial maxima an operand's scale is taken from
constexpr int WG_HEAD_BYTES = AMAX_PARTS * 4 + 256;   // workspace head: partial maxima, then the float2 {S, 1 / S}

static_assert(WG_CHUNK == XP_WGRAD_CHUNK, "the header quotes the chunk length");

// ---- largest magnitude of a (rows x C, ld) matrix and its power of two: maxima are order-free, hence deterministic ----
__global__ __launch_bounds__(256) void td_amax_kernel(const float* __restrict__ x, int64_t rows, int C, int ld, float* __restrict__ part) {
    float m = 0.f;
    td_for_each(rows, C, [&](int64_t r, int c) { m = fmaxf(m, fabsf(x[r * ld + c])); });
    m = xp_wave_max(m);
    __shared__ float sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

// scale = {S, 1 / S} with max|x| S in [2^13, 2^14); S = 1 for an all-zero operand.  fmaxf drops NaN and an infinite maximum gives S = 1: non-finite elements
// take no part in the choice and pass through the split as they are (NaN / Inf in the planes, hence in the results they touch)
__global__ __launch_bounds__(256) void td_scale_kernel(const float* __restrict__ part, int nparts, float2* __restrict__ scale) {
    float m = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) m = fmaxf(m, part[i]);
    m = xp_wave_max(m);
    __shared__ float sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
        int e = 14;
        if (m > 0.f && m <= 3.0e38f) (void)frexpf(m, &e);           // m = f 2^e, f in [0.5, 1)  ->  m 2^(14 - e) in [2^13, 2^14)
        int se = 14 - e;
        se = se < -100 ? -100 : (se > 100 ? 100 : se);
        *scale = make_float2(ldexpf(1.f, se), ldexpf(1.f, -se));
    }
}

__global__ __launch_bounds__(256) void td_mul_scale_kernel(float* __restrict__ x, int64_t rows, int C, int ld, const float2* __restrict__ scale) {
    const float S = scale->x;
    td_for_each(rows, C, [&](int64_t r, int c) { x[r * ld + c] *= S; });
}

// ---- weight-gradient GEMM ----
struct WgParams {
    const float* P;          // (M, I) rows, ldp: the gradient operand
    const float* Q;          // (M, J) rows, ldq; CONV: the NHWC input (batch, H, W, Ci), J = 9 Ci in (ky, kx, ci) order
    float* part;             // (nchunk, I, J)
    const float2* scale;     // {S, 1 / S}
    int M, I, J, ldp, ldq;
    int prescaled;           // P already holds S x the gradient
    int H, W, Ci;
    int Ho, Wo;              // CONV 3: the output grid the rows of P walk (stride 2)
};

__device__ __forceinline__ int td_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// CONV: 0 = Q is a matrix, 1 = the im2col view under reflection padding, 2 = under zero padding (a tap outside the image contributes 0),
// 3 = zero padding at STRIDE 2: row m is output pixel (yo, xo) of the (Ho, Wo) grid and tap (ky, kx) reads x at (2 yo + ky - 1, 2 xo + kx - 1)
template <int CONV>
__global__ __launch_bounds__(256) void td_wgrad_kernel(const WgParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * WG_BT * H2_ROWB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * WG_BT, i0 = blockIdx.y * WG_BT, chunk = blockIdx.z;
    const int m_begin = chunk * WG_CHUNK, m_end = min(p.M, m_begin + WG_CHUNK);
    const int cq = tid & 15, mp = tid >> 4;            // this thread stages columns 4 cq .. + 3 of slab rows 2 mp and 2 mp + 1
    const float mul = p.prescaled ? 1.f : p.scale->x;

    // the four Q columns of this thread: loop-invariant tap geometry of the implicit form
    int qky[4], qkx[4], qci[4];
    bool qok[4], pok[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = j0 + 4 * cq + e;
        qok[e] = j < p.J;
        pok[e] = i0 + 4 * cq + e < p.I;
        if (CONV) {
            const int jj = qok[e] ? j : 0, tap = jj / p.Ci;
            qci[e] = jj - tap * p.Ci; qky[e] = tap / 3 - 1; qkx[e] = tap % 3 - 1;
        }
    }
    float pa[2][4], qa[2][4];
    auto gload = [&](int t) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int m = m_begin + t * H2_BK + 2 * mp + r;
            const bool mok = m < m_end;
            const int mc = mok ? m : m_begin;                                  // a valid row: the load is unconditional, the value is selected
            const float* pr = p.P + (int64_t)mc * p.ldp + i0 + 4 * cq;
            int b = 0, y = 0, x = 0;
            if (CONV == 3) { b = mc / (p.Ho * p.Wo); const int rem = mc - b * p.Ho * p.Wo; y = rem / p.Wo; x = 2 * (rem - y * p.Wo); y *= 2; }
            else if (CONV) { b = mc / (p.H * p.W); const int rem = mc - b * p.H * p.W; y = rem / p.W; x = rem - y * p.W; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float pv = pr[pok[e] ? e : -(4 * cq)];                 // columns past I read the tile's first column, which exists
                pa[r][e] = (mok && pok[e]) ? pv * mul : 0.f;
                float qv;
                bool tap = true;
                if (CONV == 1) {
                    const int yy = td_reflect(y + qky[e], p.H), xx = td_reflect(x + qkx[e], p.W);
                    qv = p.Q[(((int64_t)b * p.H + yy) * p.W + xx) * p.Ci + qci[e]];
                } else if (CONV >= 2) {
                    const int ty = y + qky[e], tx = x + qkx[e];
                    tap = ty >= 0 && ty < p.H && tx >= 0 && tx < p.W;
                    const int yy = min(max(ty, 0), p.H - 1), xx = min(max(tx, 0), p.W - 1);      // a valid address: the load is unconditional, the value is selected
                    qv = p.Q[(((int64_t)b * p.H + yy) * p.W + xx) * p.Ci + qci[e]];
                } else {
                    qv = p.Q[(int64_t)mc * p.ldq + (qok[e] ? j0 + 4 * cq + e : j0)];
                }
                qa[r][e] = (mok && qok[e] && tap) ? qv : 0.f;
            }
        }
    };
    // transposed store: tile row = column of the operand, the thread's two slab rows are two consecutive k of one 32-bit store per plane
    auto lstore = [&]() {
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
            uint2 p0, p1;
            h2_split4(make_float4(pa[0][e], pa[1][e], pa[0][e + 1], pa[1][e + 1]), p0, p1);
            unsigned char* a = lds + (4 * cq + e) * H2_ROWB + mp * 4;
            *reinterpret_cast<unsigned*>(a) = p0.x; *reinterpret_cast<unsigned*>(a + 64) = p1.x;
            *reinterpret_cast<unsigned*>(a + H2_ROWB) = p0.y; *reinterpret_cast<unsigned*>(a + H2_ROWB + 64) = p1.y;
            h2_split4(make_float4(qa[0][e], qa[1][e], qa[0][e + 1], qa[1][e + 1]), p0, p1);
            unsigned char* q = a + WG_BT * H2_ROWB;
            *reinterpret_cast<unsigned*>(q) = p0.x; *reinterpret_cast<unsigned*>(q + 64) = p1.x;
            *reinterpret_cast<unsigned*>(q + H2_ROWB) = p0.y; *reinterpret_cast<unsigned*>(q + H2_ROWB + 64) = p1.y;
        }
    };
    const int fr = lane & 31, fh = lane >> 5, wi = wave >> 1, wj = wave & 1;
    const unsigned char* a_frag = lds + (wi * 32 + fr) * H2_ROWB + 16 * fh;
    const unsigned char* b_frag = lds + (WG_BT + wj * 32 + fr) * H2_ROWB + 16 * fh;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    const int nslab = (m_end - m_begin + H2_BK - 1) / H2_BK;
    gload(0);
    for (int t = 0; t < nslab; ++t) {
        lstore();
        __syncthreads();
        if (t + 1 < nslab) gload(t + 1);                   // in flight under this slab's matrix work
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const f16x8_t a0 = *reinterpret_cast<const f16x8_t*>(a_frag + ks * 32), a1 = *reinterpret_cast<const f16x8_t*>(a_frag + 64 + ks * 32);
            const f16x8_t b0 = *reinterpret_cast<const f16x8_t*>(b_frag + ks * 32), b1 = *reinterpret_cast<const f16x8_t*>(b_frag + 64 + ks * 32);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc, 0, 0, 0);      // smallest products first
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int j = j0 + wj * 32 + fr;
    if (j < p.J) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
            if (i < p.I) p.part[((int64_t)chunk * p.I + i) * p.J + j] = acc[r];
        }
    }
}

// out[i][j] = (sum over chunks, in chunk order) / S
__global__ __launch_bounds__(256) void td_wgrad_sum_kernel(const float* __restrict__ part, const float2* __restrict__ scale, int nchunk, int I, int J,
                                                           int ldo, float* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= I * J) return;
    float s = part[idx];
    for (int c = 1; c < nchunk; ++c) s += part[(int64_t)c * I * J + idx];
    const int i = idx / J;
    out[(int64_t)i * ldo + (idx - i * J)] = s * scale->y;
}

static size_t td_wgrad_bytes(int M, int I, int J) {
    if (M <= 0 || I <= 0 || J <= 0) return 0;
    return (size_t)WG_HEAD_BYTES + (size_t)xp_cdiv(M, WG_CHUNK) * I * J * sizeof(float);
}

static int td_wgrad_launch(const char* who, int conv, WgParams p, float* out, int ldo, const float* p_scale, void* ws, size_t ws_bytes, hipStream_t s) {
    XP_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0 && ws_bytes >= td_wgrad_bytes(p.M, p.I, p.J), "%s: workspace of %zu bytes, 256-byte aligned, needed (got %zu)",
                 who, td_wgrad_bytes(p.M, p.I, p.J), ws_bytes);
    XP_CHECK_ARG((int64_t)p.I * p.J < (1 << 30) && (int64_t)p.M * (int64_t)max(p.ldp, p.ldq) < ((int64_t)1 << 40), "%s: shape too large", who);
    float* amax = (float*)ws;
    float2* scale = (float2*)((char*)ws + AMAX_PARTS * 4);
    p.part = (float*)((char*)ws + WG_HEAD_BYTES);
    const int nchunk = xp_cdiv(p.M, WG_CHUNK);
    if (p_scale) {
        p.scale = (const float2*)p_scale; p.prescaled = 1;
    } else {
        const int nb = (int)min((int64_t)AMAX_PARTS, (int64_t)xp_cdiv(p.M, 4));
        hipLaunchKernelGGL(td_amax_kernel, dim3(nb), dim3(256), 0, s, p.P, (int64_t)p.M, p.I, p.ldp, amax);
        XP_LAUNCH_CHECK();
        hipLaunchKernelGGL(td_scale_kernel, dim3(1), dim3(256), 0, s, amax, nb, scale);
        XP_LAUNCH_CHECK();
        p.scale = scale; p.prescaled = 0;
    }
    const dim3 grid(xp_cdiv(p.J, WG_BT), xp_cdiv(p.I, WG_BT), nchunk);
    XP_CHECK_ARG(grid.y <= 65535 && grid.z <= 65535, "%s: shape too large", who);
    {
        XpProfScope prof(conv == 3 ? "conv3x3_s2_wgrad_h2" : conv == 2 ? "conv3x3_zp_wgrad_h2" : conv ? "conv3x3_wgrad_h2" : "gemm_tn_h2", s, 6.0 * p.M * p.I * p.J, 4.0 * p.M * (p.I + p.J));
        if (conv == 1) hipLaunchKernelGGL(td_wgrad_kernel<1>, grid, dim3(256), 0, s, p);
        else if (conv == 2) hipLaunchKernelGGL(td_wgrad_kernel<2>, grid, dim3(256), 0, s, p);
        else if (conv == 3) hipLaunchKernelGGL(td_wgrad_kernel<3>, grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL(td_wgrad_kernel<0>, grid, dim3(256), 0, s, p);
        XP_LAUNCH_CHECK();
    }
    XpProfScope prof("wgrad_sum", s, 0.0, 4.0 * (nchunk + 1) * p.I * p.J);
    hipLaunchKernelGGL(td_wgrad_sum_kernel, dim3(xp_cdiv((int64_t)p.I * p.J, 256)), dim3(256), 0, s, p.part, p.scale, nchunk, p.I, p.J, ldo, out);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

// BatchNorm forward statistics on data shifted by the channel's first element (exact in f64): sum d, sum d^2.  The saved mean is (2, C): the f32 mean
// and the f32 remainder of the f64 mean, so that x - mean keeps the data's precision when |mean| >> the deviation (mean 1e3, deviation 1e-2: the f32 mean
// alone is off by up to 3e-5, 3e-3 of the deviation).
__global__ __launch_bounds__(256) void td_bn_stat_parts_kernel(const float* __restrict__ x, int64_t rows, int C, int ldx, double* __restrict__ part) {
    td_colsum_parts<2>(rows, C, part, [&](int64_t r, int c, double (&a)[2]) {
        const double d = (double)x[r * ldx + c] - (double)x[c];
        a[0] += d; a[1] += d * d;
    });
}
__global__ __launch_bounds__(256) void td_bn_stat_finish_kernel(const float* __restrict__ x, const double* __restrict__ part, int64_t rows, int C, float eps,
                                                                float* __restrict__ mean, float* __restrict__ invstd, float* __restrict__ var) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double s = td_sum_parts(part, 2, 0, C, c), ss = td_sum_parts(part, 2, 1, C, c);
    const double md = s / (double)rows;
    double v = ss / (double)rows - md * md;
    v = v > 0.0 ? v : 0.0;
    const double m = (double)x[c] + md;
    mean[c] = (float)m;                                   // the f32 mean, and what it leaves of the f64 one: x - mean is formed from both
    mean[C + c] = (float)(m - (double)mean[c]);
    invstd[c] = (float)(1.0 / sqrt(v + (double)eps));
    if (var) var[c] = (float)v;
}
__global__ __launch_bounds__(256) void td_bn_apply_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, int64_t rows, int C,
                                                          float* __restrict__ y, int ldy) {
    td_for_each(rows, C, [&](int64_t r, int c) { y[r * ldy + c] = ((x[r * ldx + c] - mean[c]) - mean[C + c]) * invstd[c] * gamma[c] + beta[c]; });
}

// BatchNorm backward sums: sum dy, sum dy xhat (dy of a masked-out element still counts: the mask belongs to the layer BELOW the BatchNorm)
__global__ __launch_bounds__(256) void td_bn_bwd_parts_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx,
                                                              const float* __restrict__ mean, const float* __restrict__ invstd, int64_t rows, int C,
                                                              double* __restrict__ part) {
    td_colsum_parts<2>(rows, C, part, [&](int64_t r, int c, double (&a)[2]) {
        const float g = dy[r * lddy + c], xh = ((x[r * ldx + c] - mean[c]) - mean[C + c]) * invstd[c];
        a[0] += (double)g; a[1] += (double)g * (double)xh;
    });
}
__global__ __launch_bounds__(256) void td_bn_bwd_finish_kernel(const double* __restrict__ part, int64_t rows, int C, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, double2* __restrict__ means) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double s0 = td_sum_parts(part, 2, 0, C, c), s1 = td_sum_parts(part, 2, 1, C, c);
    if (dbeta) dbeta[c] = (float)s0;
    if (dgamma) dgamma[c] = (float)s1;
    means[c] = make_double2(s0 / (double)rows, s1 / (double)rows);
}
__global__ __launch_bounds__(256) void td_bn_bwd_dx_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const double2* __restrict__ means, int64_t rows, int C, int relu_mask, float* __restrict__ dx,
                                                           int lddx, float* __restrict__ amax_part) {
    float m = 0.f;
    td_for_each(rows, C, [&](int64_t r, int c) {
        const float xv = x[r * ldx + c], xh = ((xv - mean[c]) - mean[C + c]) * invstd[c];
        // the bracket in f64: its three terms cancel (completely at rows == 2, where xhat = +-1), and an f32 bracket would leave the roundings of the terms
        const double2 mm = means[c];
        float v = (float)((double)gamma[c] * (double)invstd[c] * ((double)dy[r * lddy + c] - mm.x - (double)xh * mm.y));
        if (relu_mask && !(xv > 0.f)) v = 0.f;
        dx[r * lddx + c] = v;
        m = fmaxf(m, fabsf(v));
    });
    if (amax_part) {
        m = xp_wave_max(m);
        __shared__ float sm[4];
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) amax_part[blockIdx.x] = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    }
}

__global__ __launch_bounds__(256) void td_colsum_parts_kernel(const float* __restrict__ x, int64_t rows, int C, int ldx, double* __restrict__ part) {
    td_colsum_parts<1>(rows, C, part, [&](int64_t r, int c, double (&a)[1]) { a[0] += (double)x[r * ldx + c]; });
}
__global__ __launch_bounds__(256) void td_colsum_finish_kernel(const double* __restrict__ part, int C, const float2* __restrict__ scale, float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float s = (float)td_sum_parts(part, 1, 0, C, c);
    out[c] = scale ? s * scale->y : s;
}

static size_t td_bn_bytes(int C) {
    if (C <= 0) return 0;
    return ((size_t)BN_PARTS * 2 * C * sizeof(double) + (size_t)C * sizeof(double2) + AMAX_PARTS * sizeof(float) + 255) & ~(size_t)255;
}
static int td_rows_check(const char* who, int64_t rows, int C) {
    XP_CHECK_ARG(rows > 0 && C > 0 && rows < ((int64_t)1 << 31) && C <= (1 << 20), "%s: bad shape rows=%lld C=%d", who, (long long)rows, C);
    return XP_OK;
}
static int td_elem_blocks(int64_t rows) { return (int)min((int64_t)AMAX_PARTS, (rows + 3) / 4); }

// ---- L2-normalise backward: one wave per row ----
__global__ __launch_bounds__(256) void td_l2norm_bwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ dy, float* __restrict__ dx,
                                                            int64_t rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* xr = x + r * ldx;
    const float* gr = dy + r * C;
    float ss = 0.f, dot = 0.f;
    for (int c = lane; c < C; c += 64) { const float v = xr[c]; ss += v * v; dot += gr[c] * v; }
    ss = xp_wave_sum(ss); dot = xp_wave_sum(dot);
    const float n = sqrtf(ss);
    if (n >= eps) {          // y = x / n:  dx = (dy - y <dy, y>) / n
        const float inv = 1.f / n, dn = dot * inv;
        for (int c = lane; c < C; c += 64) dx[r * C + c] = (gr[c] - xr[c] * inv * dn) * inv;
    } else {                 // y = x / eps: the clamp passes no gradient to the norm (torch's F.normalize)
        const float inv = 1.f / eps;
        for (int c = lane; c < C; c += 64) dx[r * C + c] = gr[c] * inv;
    }
}

}  // namespace

extern "C" size_t xp_gemm_tn_h2_workspace_bytes(int M, int I, int J) { return td_wgrad_bytes(M, I, J); }

extern "C" int xp_gemm_tn_h2(const float* P, const float* Q, float* out, int M, int I, int J, int ldp, int ldq, int ldo, const float* p_scale,
                             void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(P && Q && out, "xp_gemm_tn_h2: null pointer");
    XP_CHECK_ARG(M > 0 && I > 0 && J > 0 && ldp >= I && ldq >= J && ldo >= J, "xp_gemm_tn_h2: bad shape M=%d I=%d J=%d ldp=%d ldq=%d ldo=%d", M, I, J, ldp, ldq, ldo);
    WgParams p{};
    p.P = P; p.Q = Q; p.M = M; p.I = I; p.J = J; p.ldp = ldp; p.ldq = ldq;
    return td_wgrad_launch("xp_gemm_tn_h2", 0, p, out, ldo, p_scale, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int xp_conv3x3_wgrad_h2(const float* x, const float* dy, float* dw, int batch, int H, int W, int Ci, int Co, int stride, int reflect_pad,
                                   const float* dy_scale, void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(x && dy && dw, "xp_conv3x3_wgrad_h2: null pointer");
    XP_CHECK_ARG(stride == 1 && reflect_pad == 1, "xp_conv3x3_wgrad_h2: only stride 1 with reflection padding 1 is built (got stride %d, reflect_pad %d)",
                 stride, reflect_pad);
    XP_CHECK_ARG(batch > 0 && H >= 2 && W >= 2 && Ci > 0 && Co > 0 && (int64_t)batch * H * W < ((int64_t)1 << 31) / 16,
                 "xp_conv3x3_wgrad_h2: bad shape batch=%d H=%d W=%d Ci=%d Co=%d (reflection needs H, W >= 2)", batch, H, W, Ci, Co);
    WgParams p{};
    p.P = dy; p.Q = x; p.M = batch * H * W; p.I = Co; p.J = 9 * Ci; p.ldp = Co; p.ldq = 0; p.H = H; p.W = W; p.Ci = Ci;
    return td_wgrad_launch("xp_conv3x3_wgrad_h2", 1, p, dw, 9 * Ci, dy_scale, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t xp_bn_workspace_bytes(int C) { return td_bn_bytes(C); }

extern "C" int xp_bn_train_fwd(const float* x, int ldx, const float* gamma, const float* beta, float* y, int ldy, float* save_mean, float* save_invstd,
                               float* batch_var, int64_t rows, int C, float eps, void* workspace, size_t workspace_bytes, void* stream) {
    XP_TRY(td_rows_check("xp_bn_train_fwd", rows, C));
    XP_CHECK_ARG(x && gamma && beta && y && save_mean && save_invstd && ldx >= C && ldy >= C, "xp_bn_train_fwd: null pointer or ld < C");
    XP_CHECK_ARG(rows >= 2, "xp_bn_train_fwd: batch statistics need more than one value per channel");
    XP_CHECK_ARG(workspace && workspace_bytes >= td_bn_bytes(C), "xp_bn_train_fwd: workspace of %zu bytes needed", td_bn_bytes(C));
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    XpProfScope prof("bn_train_fwd", s, 0.0, 12.0 * rows * C);
    hipLaunchKernelGGL(td_bn_stat_parts_kernel, dim3(xp_cdiv(C, 32), BN_PARTS), dim3(256), 0, s, x, rows, C, ldx, part);
    XP_LAUNCH_CHECK();
    hipLaunchKernelGGL(td_bn_stat_finish_kernel, dim3(xp_cdiv(C, 256)), dim3(256), 0, s, x, part, rows, C, eps, save_mean, save_invstd, batch_var);
    XP_LAUNCH_CHECK();
    hipLaunchKernelGGL(td_bn_apply_kernel, dim3(td_elem_blocks(rows)), dim3(256), 0, s, x, ldx, save_mean, save_invstd, gamma, beta, rows, C, y, ldy);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_bn_train_bwd(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* save_mean, const float* save_invstd,
                               float* dx, int lddx, float* dgamma, float* dbeta, float* dx_scale, int relu_mask, int64_t rows, int C, void* workspace,
                               size_t workspace_bytes, void* stream) {
    XP_TRY(td_rows_check("xp_bn_train_bwd", rows, C));
    XP_CHECK_ARG(dy && x && gamma && save_mean && save_invstd && dx && lddy >= C && ldx >= C && lddx >= C, "xp_bn_train_bwd: null pointer or ld < C");
    XP_CHECK_ARG(workspace && workspace_bytes >= td_bn_bytes(C), "xp_bn_train_bwd: workspace of %zu bytes needed", td_bn_bytes(C));
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    double2* means = (double2*)(part + (size_t)BN_PARTS * 2 * C);
    float* amax = (float*)(means + C);
    XpProfScope prof("bn_train_bwd", s, 0.0, 20.0 * rows * C);
    hipLaunchKernelGGL(td_bn_bwd_parts_kernel, dim3(xp_cdiv(C, 32), BN_PARTS), dim3(256), 0, s, dy, lddy, x, ldx, save_mean, save_invstd, rows, C, part);
    XP_LAUNCH_CHECK();
    hipLaunchKernelGGL(td_bn_bwd_finish_kernel, dim3(xp_cdiv(C, 256)), dim3(256), 0, s, part, rows, C, dgamma, dbeta, means);
    XP_LAUNCH_CHECK();
    const int nb = td_elem_blocks(rows);
    hipLaunchKernelGGL(td_bn_bwd_dx_kernel, dim3(nb), dim3(256), 0, s, dy, lddy, x, ldx, save_mean, save_invstd, gamma, means, rows, C, relu_mask, dx, lddx,
                       dx_scale ? amax : nullptr);
    XP_LAUNCH_CHECK();
    if (dx_scale) {
        hipLaunchKernelGGL(td_scale_kernel, dim3(1), dim3(256), 0, s, amax, nb, (float2*)dx_scale);
        XP_LAUNCH_CHECK();
        hipLaunchKernelGGL(td_mul_scale_kernel, dim3(nb), dim3(256), 0, s, dx, rows, C, lddx, (const float2*)dx_scale);
        XP_LAUNCH_CHECK();
    }
    return XP_OK;
}

extern "C" int xp_colsum_rows(const float* x, int ldx, int64_t rows, int C, const float* x_scale, float* out, void* workspace, size_t workspace_bytes,
                              void* stream) {
    XP_TRY(td_rows_check("xp_colsum_rows", rows, C));
    XP_CHECK_ARG(x && out && ldx >= C, "xp_colsum_rows: null pointer or ld < C");
    XP_CHECK_ARG(workspace && workspace_bytes >= td_bn_bytes(C), "xp_colsum_rows: workspace of %zu bytes needed", td_bn_bytes(C));
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    XpProfScope prof("colsum_rows", s, 0.0, 4.0 * rows * C);
    hipLaunchKernelGGL(td_colsum_parts_kernel, dim3(xp_cdiv(C, 32), BN_PARTS), dim3(256), 0, s, x, rows, C, ldx, part);
    XP_LAUNCH_CHECK();
    hipLaunchKernelGGL(td_colsum_finish_kernel, dim3(xp_cdiv(C, 256)), dim3(256), 0, s, part, C, (const float2*)x_scale, out);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_l2norm_rows_bwd(const float* x, int ldx, const float* dy, float* dx, int64_t rows, int C, float eps, void* stream) {
    XP_TRY(td_rows_check("xp_l2norm_rows_bwd", rows, C));
    XP_CHECK_ARG(x && dy && dx && ldx >= C && eps > 0.f, "xp_l2norm_rows_bwd: null pointer, ld < C or eps <= 0");
    hipStream_t s = (hipStream_t)stream;
    XpProfScope prof("l2norm_rows_bwd", s, 0.0, 12.0 * rows * C);
    hipLaunchKernelGGL(td_l2norm_bwd_kernel, dim3(xp_cdiv(rows, 4)), dim3(256), 0, s, x, ldx, dy, dx, rows, C, eps);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

// ---- the zero-padded 3x3 convolution of the RegNet head (RegNet.py:13-18): weight gradient and input gradient ----
namespace {

// wr[ci][ky][kx][co] = w[co][2 - ky][2 - kx][ci]: the weight whose FORWARD zero-pad convolution of dy is the input gradient
__global__ __launch_bounds__(256) void td_rot_weights_kernel(const float* __restrict__ w, float* __restrict__ wr, int Ci, int Co) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Ci * 9 * Co) return;
    const int co = idx % Co, tap = (idx / Co) % 9, ci = idx / (9 * Co);
    wr[idx] = w[((int64_t)co * 9 + (8 - tap)) * Ci + ci];
}
// the epilogue's affine of the input gradient: scale[c] = 1 / S, shift[c] = 0
__global__ __launch_bounds__(256) void td_unscale_vec_kernel(const float2* __restrict__ s, float* __restrict__ scale, float* __restrict__ shift, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) { scale[c] = s->y; shift[c] = 0.f; }
}
__global__ __launch_bounds__(256) void td_scaled_copy_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t rows, int C, const float2* __restrict__ scale) {
    const float S = scale->x;
    td_for_each(rows, C, [&](int64_t r, int c) { y[r * C + c] = x[r * C + c] * S; });
}

static size_t td_up256(size_t n) { return (n + 255) & ~(size_t)255; }
struct DgradLayout { size_t vec, wrot, wsplit, dys, total; };
static DgradLayout td_dgrad_layout(int batch, int H, int W, int Ci, int Co) {
    DgradLayout l{};
    l.vec = WG_HEAD_BYTES;                                                   // head: partial maxima and {S, 1 / S}, as the weight gradient's
    l.wrot = l.vec + td_up256((size_t)2 * Ci * sizeof(float));
    l.wsplit = l.wrot + td_up256((size_t)9 * Ci * Co * sizeof(float));
    l.dys = l.wsplit + td_up256(xp_split_weights_h2_bytes(Ci, 9 * Co));
    l.total = l.dys + td_up256((size_t)batch * H * W * Co * sizeof(float));
    return l;
}
static bool td_conv_shape_ok(int batch, int H, int W, int Ci, int Co) {
    return batch > 0 && H >= 1 && W >= 1 && Ci > 0 && Co > 0 && (int64_t)batch * H * W < ((int64_t)1 << 31) / 16 && (int64_t)Ci * Co < (1 << 26);
}

}  // namespace

extern "C" int xp_conv3x3_zp_wgrad_h2(const float* x, const float* dy, float* dw, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(x && dy && dw, "xp_conv3x3_zp_wgrad_h2: null pointer");
    XP_CHECK_ARG(td_conv_shape_ok(batch, H, W, Ci, Co), "xp_conv3x3_zp_wgrad_h2: bad shape batch=%d H=%d W=%d Ci=%d Co=%d", batch, H, W, Ci, Co);
    WgParams p{};
    p.P = dy; p.Q = x; p.M = batch * H * W; p.I = Co; p.J = 9 * Ci; p.ldp = Co; p.ldq = 0; p.H = H; p.W = W; p.Ci = Ci;
    return td_wgrad_launch("xp_conv3x3_zp_wgrad_h2", 2, p, dw, 9 * Ci, dy_scale, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t xp_conv3x3_dgrad_h2_workspace_bytes(int batch, int H, int W, int Ci, int Co) {
    if (!td_conv_shape_ok(batch, H, W, Ci, Co)) return 0;
    return td_dgrad_layout(batch, H, W, Ci, Co).total;
}

extern "C" int xp_conv3x3_dgrad_h2(const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(dy && w && dx, "xp_conv3x3_dgrad_h2: null pointer");
    XP_CHECK_ARG(td_conv_shape_ok(batch, H, W, Ci, Co), "xp_conv3x3_dgrad_h2: bad shape batch=%d H=%d W=%d Ci=%d Co=%d", batch, H, W, Ci, Co);
    XP_CHECK_ARG(Co % 4 == 0, "xp_conv3x3_dgrad_h2: Co must be a multiple of 4 (got %d): the engine loads dy in 4-element channel groups", Co);
    const DgradLayout l = td_dgrad_layout(batch, H, W, Ci, Co);
    XP_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= l.total,
                 "xp_conv3x3_dgrad_h2: workspace of %zu bytes, 256-byte aligned, needed (got %zu)", l.total, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* amax = (float*)ws;
    const float2* scale = (const float2*)dy_scale;
    float* vscale = (float*)(ws + l.vec);
    float* vshift = vscale + Ci;
    float* wrot = (float*)(ws + l.wrot);
    const int64_t rows = (int64_t)batch * H * W;
    if (!dy_scale) {          // S from the largest magnitude of dy, and the scaled copy the engine reads
        float2* own = (float2*)(ws + AMAX_PARTS * 4);
        float* dys = (float*)(ws + l.dys);
        const int nb = td_elem_blocks(rows);
        hipLaunchKernelGGL(td_amax_kernel, dim3(nb), dim3(256), 0, s, dy, rows, Co, Co, amax);
        XP_LAUNCH_CHECK();
        hipLaunchKernelGGL(td_scale_kernel, dim3(1), dim3(256), 0, s, amax, nb, own);
        XP_LAUNCH_CHECK();
        hipLaunchKernelGGL(td_scaled_copy_kernel, dim3(nb), dim3(256), 0, s, dy, dys, rows, Co, own);
        XP_LAUNCH_CHECK();
        scale = own; dy = dys;
    }
    hipLaunchKernelGGL(td_unscale_vec_kernel, dim3(xp_cdiv(Ci, 256)), dim3(256), 0, s, scale, vscale, vshift, Ci);
    XP_LAUNCH_CHECK();
    hipLaunchKernelGGL(td_rot_weights_kernel, dim3(xp_cdiv(9 * Ci * Co, 256)), dim3(256), 0, s, w, wrot, Ci, Co);
    XP_LAUNCH_CHECK();
    XP_TRY(xp_split_weights_h2(wrot, ws + l.wsplit, Ci, 9 * Co, stream));
    // dx = conv3x3(zero_pad(S dy), wrot) / S on the forward's implicit-GEMM engine: no atomics, the engine's fixed summation order
    return xp_conv3x3_nhwc_h2(dy, ws + l.wsplit, dx, nullptr, vscale, vshift, batch, H, W, Co, Ci, 1, 0, 0, stream);
}

// ---- the zero-padded STRIDE-2 3x3 convolution of patch embed and the downsamplers (VMamba.py:1405-1440): weight gradient, input gradient ----
// Input gradient.  dx pixel (y, x) receives tap (ky, kx) only when y + 1 - ky and x + 1 - kx are even, from dy at ((y + 1 - ky) / 2, (x + 1 - kx) / 2):
// the pixels fall into four classes by the parity (py, px) of (y, x) with (1 + py)(1 + px) = 1, 2, 2, 4 taps — ky = 1 for an even y, ky = 0 (dy row
// i + 1) and ky = 2 (dy row i) for the odd y = 2 i + 1, the same along x.  Each class is an implicit GEMM of its own on the split-fp16 engine:
// M = its pixels, N = Ci, K = taps Co, the A row of a pixel gathered from dy tap by tap, the weight a K-slice of ONE rearranged (Ci, Ktot) matrix that
// is split once per call (every class's slice padded to whole 32-wide slabs).  No zero-stuffed dy, no products with structural zeros.
namespace {

struct S2Class { int py, px, Hc, Wc, taps, slab0, nslab; };
static S2Class td_s2_class(int c, int H, int W, int Co) {
    S2Class k{};
    k.py = c >> 1; k.px = c & 1;
    k.Hc = (H + 1 - k.py) / 2; k.Wc = (W + 1 - k.px) / 2;
    k.taps = (1 + k.py) * (1 + k.px);
    for (int q = 0; q <= c; ++q) {
        const int n = xp_cdiv((1 + (q >> 1)) * (1 + (q & 1)) * Co, H2_BK);
        if (q < c) k.slab0 += n; else k.nslab = n;
    }
    return k;
}
static int td_s2_ktot(int Co) { const S2Class k = td_s2_class(3, 1, 1, Co); return (k.slab0 + k.nslab) * H2_BK; }

// wc[ci][32 slab0(c) + (ty nx + tx) Co + co] = w[co][ky][kx][ci], ky = py ? 2 ty : 1, kx = px ? 2 tx : 1; zeros in the pad of every slice
__global__ __launch_bounds__(256) void td_s2_weights_kernel(const float* __restrict__ w, float* __restrict__ wc, int Ci, int Co, int Ktot) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Ci * Ktot) return;
    const int ci = idx / Ktot;
    int k = idx - ci * Ktot;
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int py = c >> 1, px = c & 1, taps = (1 + py) * (1 + px), span = (taps * Co + H2_BK - 1) / H2_BK * H2_BK;
        if (k >= 0 && k < taps * Co) {
            const int tap = k / Co, co = k - tap * Co;
            const int ty = px ? tap >> 1 : tap, tx = px ? tap & 1 : 0;
            v = w[((int64_t)co * 9 + (py ? 2 * ty : 1) * 3 + (px ? 2 * tx : 1)) * Ci + ci];
        }
        k = k < 0 ? k : (k < span ? -1 : k - span);          // consumed by this class, or moved on to the next
    }
    wc[idx] = v;
}

struct S2DgParams {
    const float* dy;         // S x the gradient, (batch, Ho, Wo, Co)
    const uint4* wsplit;     // xp_split_weights_h2 of wc (Ci, Ktot)
    const float* wscale;     // its Ci inverse row scales
    const float2* scale;     // {S, 1 / S}
    float* dx;               // (batch, H, W, Ci)
    int batch, H, W, Ci, Co, Ho, Wo;
    int slab0[4];            // first slab of class c's K-slice
};

// row m of class (py, px) is dx pixel (2 i + py, 2 j + px) of sample b: dx = accumulator x the weight row's power of two x 1 / S, both exact
template <class T, int TN>
__device__ __forceinline__ void td_s2_store(const S2DgParams& p, const f32x16 (&acc)[1][TN], int m0, int n0, int Mc, int Hc, int Wc, int py, int px) {
    const float inv_s = p.scale->y;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + T::row_of(0, r);
        if (m >= Mc) continue;
        const int b = m / (Hc * Wc), rr = m - b * (Hc * Wc), i = rr / Wc, j = rr - i * Wc;
        float* row = p.dx + (((int64_t)b * p.H + 2 * i + py) * p.W + 2 * j + px) * p.Ci;
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
            const int n = n0 + T::col_of(jn);
            if (n < p.Ci) row[n] = acc[0][jn][r] * p.wscale[n] * inv_s;
        }
    }
}

template <int TN>
__global__ __launch_bounds__(256) void td_s2_dgrad_kernel(const S2DgParams p) {
    using T = GemmTileH2<2, 2, 1, TN>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[T::kLdsBytes];
    const int cls = blockIdx.z, py = cls >> 1, px = cls & 1;
    const int Hc = (p.H + 1 - py) / 2, Wc = (p.W + 1 - px) / 2;
    const int Mc = p.batch * Hc * Wc, Kc = (1 + py) * (1 + px) * p.Co;
    const int m0 = blockIdx.x * T::BM, n0 = blockIdx.y * T::BN;
    if (m0 >= Mc) return;                          // block-uniform, before any barrier: this class has fewer row tiles (or no pixel at all)

    const float* a_ptr[T::A_LD];
    int a_i[T::A_LD], a_j[T::A_LD], a_tap[T::A_LD], a_co[T::A_LD];
#pragma unroll
    for (int s = 0; s < T::A_LD; ++s) {
        const int m = m0 + T::a_row(s);
        const int mc = m < Mc ? m : 0;           // rows past Mc only feed output rows that are never stored
        const int b = mc / (Hc * Wc), rr = mc - b * (Hc * Wc);
        a_i[s] = rr / Wc; a_j[s] = rr - a_i[s] * Wc;
        a_ptr[s] = p.dy + (int64_t)b * p.Ho * p.Wo * p.Co;
        const int k = T::a_quad(s) * 4;          // (tap, co) advance by one slab per call: no division in the K loop
        a_tap[s] = k / p.Co; a_co[s] = k - a_tap[s] * p.Co;
    }
    const int nslab = (Kc + H2_BK - 1) / H2_BK;
    const uint4* w_unit[T::B_LD];
#pragma unroll
    for (int s = 0; s < T::B_LD; ++s) {
        const int n = n0 + T::b_row(s);
        w_unit[s] = p.wsplit + (int64_t)(n < p.Ci ? n : 0) * H2_SLAB_UNITS + T::b_unit(s);
    }
    const int64_t w_slab = (int64_t)p.Ci * H2_SLAB_UNITS;
    const int slab0 = p.slab0[cls];
    auto ldA = [&](int s, int k, float4& v) -> bool {
        bool ok = k < Kc;
        int tap = a_tap[s], co = a_co[s];
        if (!ok) { tap = 0; co = 0; }
        a_co[s] += H2_BK;                                  // Co >= 4: at most eight wraps per 32-wide slab, as selects
#pragma unroll
        for (int w = 0; w < 8; ++w) { const bool wrap = a_co[s] >= p.Co; a_co[s] -= wrap ? p.Co : 0; a_tap[s] += wrap ? 1 : 0; }
        const int ty = px ? tap >> 1 : tap, tx = px ? tap & 1 : 0;
        int yo = a_i[s] + ((py && ty == 0) ? 1 : 0), xo = a_j[s] + ((px && tx == 0) ? 1 : 0);      // never negative
        ok = ok && yo < p.Ho && xo < p.Wo;
        yo = yo < p.Ho ? yo : p.Ho - 1; xo = xo < p.Wo ? xo : p.Wo - 1;      // a valid address: the load is unconditional, the slot is staged as zeros
        v = *reinterpret_cast<const float4*>(a_ptr[s] + ((int64_t)yo * p.Wo + xo) * p.Co + co);
        return ok;
    };
    auto ldB = [&](int s, int t) -> uint4 { return w_unit[s][(slab0 + (t < nslab ? t : nslab - 1)) * w_slab]; };

    f32x16 acc[1][TN];
    T::run(lds, Kc, ldA, ldB, acc);

    td_s2_store<T, TN>(p, acc, m0, n0, Mc, Hc, Wc, py, px);
}

// The same GEMMs on the row-stationary engine (GemmTileH2R: every lane loads its own row's fragment straight from global memory, only the weights go
// through the LDS), for Co % 16 == 0 and a dy below 2 GB: a 16-wide k-step then lies inside ONE tap, the same for the whole wave, so (tap, co) advance as
// scalars and the lane's geometry — which dy pixel the tap reads, whether it exists — is worked out once per tap, at most four times per launch, as a
// 32-bit byte offset into a buffer resource over dy; a tap outside dy and a k-step past the class's K carry an offset beyond its end and the hardware
// returns zeros (the scheme of gemm_h2r_kernel's convolution form).  Same values in the same order as the tile-engine form above: the same bits.
template <int TN>
__global__ __launch_bounds__(256) void td_s2_dgrad_r_kernel(const S2DgParams p) {
    using T = GemmTileH2R<TN>;
    extern __shared__ __align__(16) unsigned char lds[];
    const int cls = blockIdx.z, py = cls >> 1, px = cls & 1;
    const int Hc = (p.H + 1 - py) / 2, Wc = (p.W + 1 - px) / 2;
    const int Mc = p.batch * Hc * Wc, taps = (1 + py) * (1 + px), Kc = taps * p.Co;
    const int m0 = blockIdx.x * T::BM, n0 = blockIdx.y * T::BN;
    if (m0 >= Mc) return;                          // block-uniform, before any barrier

    const int fh = (threadIdx.x & 63) >> 5;
    const int m = m0 + T::a_row();
    const int mc = m < Mc ? m : 0;               // rows past Mc only feed output rows that are never stored
    const int b = mc / (Hc * Wc), rr = mc - b * (Hc * Wc), ai = rr / Wc, aj = rr - ai * Wc;
    const int nslab = (Kc + H2_BK - 1) / H2_BK;
    const uint4* w_unit[T::B_LD];
#pragma unroll
    for (int s = 0; s < T::B_LD; ++s) {
        const int n = n0 + T::b_row(s);
        w_unit[s] = p.wsplit + (int64_t)(n < p.Ci ? n : 0) * H2_SLAB_UNITS + T::b_unit(s);
    }
    const int64_t w_slab = (int64_t)p.Ci * H2_SLAB_UNITS;
    const int slab0 = p.slab0[cls];
    auto ldB = [&](int s, int t) -> uint4 { return w_unit[s][(slab0 + (t < nslab ? t : nslab - 1)) * w_slab]; };

    constexpr unsigned kPastEnd = 0x80000000u;                 // >= the bytes of dy (the host checks), and no 32-bit wrap when the channel offset is added
    const unsigned dy_bytes = (unsigned)p.batch * p.Ho * p.Wo * p.Co * 4u;
    const unsigned lane_base = (unsigned)b * p.Ho * p.Wo * p.Co * 4u + (unsigned)fh * 32u;       // the lane's sample and its half of the k-step
    auto tap_offset = [&](int tap) -> unsigned {
        if (tap >= taps) return kPastEnd;
        const int ty = px ? tap >> 1 : tap, tx = px ? tap & 1 : 0;
        const int yo = ai + ((py && ty == 0) ? 1 : 0), xo = aj + ((px && tx == 0) ? 1 : 0);      // never negative
        return (yo < p.Ho && xo < p.Wo) ? lane_base + (unsigned)((yo * p.Wo + xo) * p.Co) * 4u : kPastEnd;
    };
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, 0, (int)dy_bytes, 0x00020000);
    int tap = 0, co4 = 0;                                       // of the next k-step: wave-uniform (co4 = byte offset of its first channel)
    unsigned cur = tap_offset(0);
    typedef unsigned raw4 __attribute__((ext_vector_type(4)));
    auto ldA8 = [&](int, float4& lo, float4& hi) -> bool {
        const raw4 a = __builtin_bit_cast(raw4, __builtin_amdgcn_raw_buffer_load_b128(rs, cur, co4, 0));
        const raw4 c = __builtin_bit_cast(raw4, __builtin_amdgcn_raw_buffer_load_b128(rs, cur + 16, co4, 0));
        lo = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w));
        hi = make_float4(__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z), __uint_as_float(c.w));
        co4 += 64;
        if (co4 == p.Co * 4) { co4 = 0; ++tap; cur = tap_offset(tap); }
        return true;
    };
    f32x16 acc[1][TN];
    T::template run<false>(lds, Kc, ldA8, ldB, acc);

    td_s2_store<T, TN>(p, acc, m0, n0, Mc, Hc, Wc, py, px);
}

template <int TN>
static int td_s2_dgrad_r_launch(const S2DgParams& p, int64_t m_even, hipStream_t s) {
    using T = GemmTileH2R<TN>;
    hipLaunchKernelGGL(td_s2_dgrad_r_kernel<TN>, dim3((unsigned)xp_cdiv(m_even, (int64_t)T::BM), xp_cdiv(p.Ci, T::BN), 4), dim3(256), T::kLdsBytes, s, p);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

template <int TN>
static int td_s2_dgrad_launch(const S2DgParams& p, int64_t m_even, hipStream_t s) {
    using T = GemmTileH2<2, 2, 1, TN>;
    hipLaunchKernelGGL(td_s2_dgrad_kernel<TN>, dim3((unsigned)xp_cdiv(m_even, (int64_t)T::BM), xp_cdiv(p.Ci, T::BN), 4), dim3(256), 0, s, p);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

struct S2DgradLayout { size_t wc, wsplit, dys, total; };
static S2DgradLayout td_s2_dgrad_layout(int batch, int Ho, int Wo, int Ci, int Co) {
    S2DgradLayout l{};
    const int Ktot = td_s2_ktot(Co);
    l.wc = WG_HEAD_BYTES;                                                    // head: partial maxima and {S, 1 / S}, as the weight gradient's
    l.wsplit = l.wc + td_up256((size_t)Ci * Ktot * sizeof(float));
    l.dys = l.wsplit + td_up256(xp_split_weights_h2_bytes(Ci, Ktot));
    l.total = l.dys + td_up256((size_t)batch * Ho * Wo * Co * sizeof(float));
    return l;
}
static bool td_s2_shape_ok(int batch, int H, int W, int Ci, int Co) {
    return batch > 0 && H >= 1 && W >= 1 && Ci > 0 && Co > 0 && (int64_t)batch * H * W < ((int64_t)1 << 31) / 16 && (int64_t)Ci * Co < (1 << 24);
}

// dw9co[t][co] = sum over output pixels of dy[b, yo, xo, co] img[b, 2 yo + ky - 1, 2 xo + kx - 1]: the 9 Co sums of the stem in the fixed order of the
// BatchNorm sums (train_rows.h), f64 accumulators
__global__ __launch_bounds__(256) void td_stem_wgrad_parts_kernel(const float* __restrict__ img, const float* __restrict__ dy, int H, int W, int Ho, int Wo,
                                                                  int64_t rows, int Co, double* __restrict__ part) {
    td_colsum_parts<9>(rows, Co, part, [&](int64_t r, int c, double (&a)[9]) {
        const int64_t b = r / ((int64_t)Ho * Wo);
        const int rem = (int)(r - b * Ho * Wo), yo = rem / Wo, xo = rem - yo * Wo;
        const double g = (double)dy[r * Co + c];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ih = 2 * yo + t / 3 - 1, iw = 2 * xo + t % 3 - 1;
            const bool in = ih >= 0 && ih < H && iw >= 0 && iw < W;
            const float v = img[(b * H + (in ? ih : 0)) * W + (in ? iw : 0)];
            a[t] += in ? g * (double)v : 0.0;
        }
    });
}
__global__ __launch_bounds__(256) void td_stem_wgrad_finish_kernel(const double* __restrict__ part, int Co, const float2* __restrict__ scale,
                                                                   float* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 9 * Co) return;
    const int t = idx / Co, c = idx - t * Co;
    const float s = (float)td_sum_parts(part, 9, t, Co, c);
    out[idx] = scale ? s * scale->y : s;
}
static size_t td_stem_wgrad_bytes(int Co) { return Co > 0 ? td_up256((size_t)BN_PARTS * 9 * Co * sizeof(double)) : 0; }

}  // namespace

extern "C" int xp_conv3x3_s2_wgrad_h2(const float* x, const float* dy, float* dw, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(x && dy && dw, "xp_conv3x3_s2_wgrad_h2: null pointer");
    XP_CHECK_ARG(td_s2_shape_ok(batch, H, W, Ci, Co), "xp_conv3x3_s2_wgrad_h2: bad shape batch=%d H=%d W=%d Ci=%d Co=%d", batch, H, W, Ci, Co);
    WgParams p{};
    p.Ho = (H - 1) / 2 + 1; p.Wo = (W - 1) / 2 + 1;
    p.P = dy; p.Q = x; p.M = batch * p.Ho * p.Wo; p.I = Co; p.J = 9 * Ci; p.ldp = Co; p.ldq = 0; p.H = H; p.W = W; p.Ci = Ci;
    return td_wgrad_launch("xp_conv3x3_s2_wgrad_h2", 3, p, dw, 9 * Ci, dy_scale, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t xp_conv3x3_s2_dgrad_h2_workspace_bytes(int batch, int H, int W, int Ci, int Co) {
    if (!td_s2_shape_ok(batch, H, W, Ci, Co)) return 0;
    return td_s2_dgrad_layout(batch, (H - 1) / 2 + 1, (W - 1) / 2 + 1, Ci, Co).total;
}

extern "C" int xp_conv3x3_s2_dgrad_h2(const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(dy && w && dx, "xp_conv3x3_s2_dgrad_h2: null pointer");
    XP_CHECK_ARG(td_s2_shape_ok(batch, H, W, Ci, Co), "xp_conv3x3_s2_dgrad_h2: bad shape batch=%d H=%d W=%d Ci=%d Co=%d", batch, H, W, Ci, Co);
    XP_CHECK_ARG(Co % 4 == 0, "xp_conv3x3_s2_dgrad_h2: Co must be a multiple of 4 (got %d): the engine loads dy in 4-element channel groups", Co);
    XP_CHECK_ARG(((uintptr_t)dy & 15) == 0, "xp_conv3x3_s2_dgrad_h2: dy must be 16-byte aligned");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const S2DgradLayout l = td_s2_dgrad_layout(batch, Ho, Wo, Ci, Co);
    XP_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= l.total,
                 "xp_conv3x3_s2_dgrad_h2: workspace of %zu bytes, 256-byte aligned, needed (got %zu)", l.total, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const float2* scale = (const float2*)dy_scale;
    const int64_t rows = (int64_t)batch * Ho * Wo;
    if (!dy_scale) {          // S from the largest magnitude of dy, and the scaled copy the engine reads
        float* amax = (float*)ws;
        float2* own = (float2*)(ws + AMAX_PARTS * 4);
        float* dys = (float*)(ws + l.dys);
        const int nb = td_elem_blocks(rows);
        hipLaunchKernelGGL(td_amax_kernel, dim3(nb), dim3(256), 0, s, dy, rows, Co, Co, amax);
        XP_LAUNCH_CHECK();
        hipLaunchKernelGGL(td_scale_kernel, dim3(1), dim3(256), 0, s, amax, nb, own);
        XP_LAUNCH_CHECK();
        hipLaunchKernelGGL(td_scaled_copy_kernel, dim3(nb), dim3(256), 0, s, dy, dys, rows, Co, own);
        XP_LAUNCH_CHECK();
        scale = own; dy = dys;
    }
    const int Ktot = td_s2_ktot(Co);
    float* wc = (float*)(ws + l.wc);
    hipLaunchKernelGGL(td_s2_weights_kernel, dim3(xp_cdiv(Ci * Ktot, 256)), dim3(256), 0, s, w, wc, Ci, Co, Ktot);
    XP_LAUNCH_CHECK();
    XP_TRY(xp_split_weights_h2(wc, ws + l.wsplit, Ci, Ktot, stream));
    S2DgParams p{};
    p.dy = dy; p.wsplit = (const uint4*)(ws + l.wsplit); p.wscale = h2_scales(ws + l.wsplit, Ci, Ktot); p.scale = scale; p.dx = dx;
    p.batch = batch; p.H = H; p.W = W; p.Ci = Ci; p.Co = Co; p.Ho = Ho; p.Wo = Wo;
    for (int c = 0; c < 4; ++c) p.slab0[c] = td_s2_class(c, H, W, Co).slab0;
    const int64_t m_even = (int64_t)batch * ((H + 1) / 2) * ((W + 1) / 2);        // the largest class
    XpProfScope prof("conv3x3_s2_dgrad_h2", s, 6.0 * rows * 9.0 * Ci * Co, 4.0 * (rows * Co + (double)batch * H * W * Ci));
    // Row-stationary form where a k-step lies inside one tap and 32-bit offsets reach all of dy; the tile-engine form otherwise.  Both walk K in the same
    // order, so the choice never changes a result bit (measured at the three downsampler shapes, batch 16: 40 / 42 / 68 us against 65 / 58 / 87 us).
    if (Co % 16 == 0 && rows * Co * 4 < ((int64_t)1 << 31)) {
        if (Ci <= 32) return td_s2_dgrad_r_launch<1>(p, m_even, s);
        if (Ci <= 64) return td_s2_dgrad_r_launch<2>(p, m_even, s);
        if (Ci <= 96 || Ci % 96 == 0) return td_s2_dgrad_r_launch<3>(p, m_even, s);          // 96, 192, 384: no column of the tile is wasted
        return td_s2_dgrad_r_launch<4>(p, m_even, s);
    }
    return Ci <= 64 ? td_s2_dgrad_launch<1>(p, m_even, s) : td_s2_dgrad_launch<2>(p, m_even, s);
}

extern "C" size_t xp_stem_conv_wgrad_workspace_bytes(int Co) { return td_stem_wgrad_bytes(Co); }

extern "C" int xp_stem_conv_wgrad(const float* img, const float* dy, float* dw9co, int batch, int H, int W, int Co, const float* dy_scale, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(img && dy && dw9co, "xp_stem_conv_wgrad: null pointer");
    XP_CHECK_ARG(batch > 0 && H >= 1 && W >= 1 && Co > 0 && Co <= (1 << 16) && (int64_t)batch * H * W < ((int64_t)1 << 31),
                 "xp_stem_conv_wgrad: bad shape batch=%d H=%d W=%d Co=%d", batch, H, W, Co);
    XP_CHECK_ARG(workspace && workspace_bytes >= td_stem_wgrad_bytes(Co), "xp_stem_conv_wgrad: workspace of %zu bytes needed", td_stem_wgrad_bytes(Co));
    hipStream_t s = (hipStream_t)stream;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t rows = (int64_t)batch * Ho * Wo;
    double* part = (double*)workspace;
    XpProfScope prof("stem_conv_wgrad", s, 18.0 * rows * Co, 4.0 * rows * (Co + 9));
    hipLaunchKernelGGL(td_stem_wgrad_parts_kernel, dim3(xp_cdiv(Co, 32), BN_PARTS), dim3(256), 0, s, img, dy, H, W, Ho, Wo, rows, Co, part);
    XP_LAUNCH_CHECK();
    hipLaunchKernelGGL(td_stem_wgrad_finish_kernel, dim3(xp_cdiv(9 * Co, 256)), dim3(256), 0, s, part, Co, (const float2*)dy_scale, dw9co);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

// ---- the REFLECTION-padded 3x3 convolution of the head trunk (XPoint.py:112-138): input gradient ----
// With g the zero-padded input gradient on the PADDED frame (rows -1 .. H, columns -1 .. W; g[v][u] = sum_k w[k]^T dy[v - ky + 1][u - kx + 1], taps
// outside dy absent), reflection folds the frame back: dx[y][x] = sum of g[v][u] over v in {y} + {-1 if y == 1} + {H if y == H - 2} and u likewise.
// The interior term g[y][x] is xp_conv3x3_dgrad_h2 as it stands.  The frame — 2 (W + 2) + 2 H pixels per image — is a thin implicit GEMM of its own
// in four classes (top row v = -1: only ky = 0, from dy row 0; bottom row v = H: only ky = 2, from dy row H - 1; left column u = -1: only kx = 0;
// right column u = W: only kx = 2), each cut by its three taps along the line: twelve GEMMs with M = the class's frame pixels, N = Ci, K = Co over
// their slice of ONE rearranged weight that is split once per call (every slice padded to whole 32-wide slabs), the scheme of the stride-2 input
// gradient above.  The cut by tap keeps the reduction short — the frame has few rows, so one workgroup per (row tile, class) walking K = 3 Co alone
// would be a long serial loop on a few CUs — and the three partial results go to three planes that the last kernel adds in tap order, together with
// the fold: it adds the frame terms to the at most 2 (H + W) - 4 pixels of rows / columns 1 and n - 2 in a fixed order.  No (H + 2) x (W + 2) copy
// of dy or dx, no atomics.
namespace {

static int td_rp_span(int Co) { return xp_cdiv(Co, H2_BK) * H2_BK; }          // K of one (class, tap) slice
static int td_rp_frame(int H, int W) { return 2 * (W + 2) + 2 * H; }          // per image: top (W + 2), bottom (W + 2), left (H), right (H)

// wf[ci][span (3 cls + t) + co] = w[co][ky][kx][ci]: cls 0 (ky, kx) = (0, t), 1: (2, t), 2: (t, 0), 3: (t, 2); zeros in the pad of every slice
__global__ __launch_bounds__(256) void td_rp_weights_kernel(const float* __restrict__ w, float* __restrict__ wf, int Ci, int Co, int span) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Ci * 12 * span) return;
    const int ci = idx / (12 * span), rem = idx - ci * 12 * span, slice = rem / span, co = rem - slice * span;
    float v = 0.f;
    if (co < Co) {
        const int cls = slice / 3, t = slice - 3 * cls;
        const int ky = cls == 0 ? 0 : (cls == 1 ? 2 : t), kx = cls == 2 ? 0 : (cls == 3 ? 2 : t);
        v = w[((int64_t)co * 9 + ky * 3 + kx) * Ci + ci];
    }
    wf[idx] = v;
}

struct RpDgParams {
    const float* dy;         // S x the gradient, (batch, H, W, Co)
    const uint4* wsplit;     // xp_split_weights_h2 of wf (Ci, 12 span)
    const float* wscale;     // its Ci inverse row scales
    const float2* scale;     // {S, 1 / S}
    float* gf;               // (3, batch, frame, Ci): the unscaled g on the frame, one plane per tap
    float* dx;               // (batch, H, W, Ci): holds the interior term, receives the frame terms
    int batch, H, W, Ci, Co;
    int slabs;               // slabs per (class, tap) slice
};

// Row m of class cls is frame pixel i of sample b: i = u + 1 along the top / bottom row, i = v along the left / right column.  Tap t reads the dy
// pixel at line position i - t (rows: the column u - kx + 1) or i - t + 1 (columns: the row v - ky + 1) of dy's first / last row or column.
template <int TN>
__global__ __launch_bounds__(256) void td_rp_frame_kernel(const RpDgParams p) {
    using T = GemmTileH2<2, 2, 1, TN>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[T::kLdsBytes];
    const int cls = blockIdx.z / 3, tap = blockIdx.z - 3 * cls;
    const bool horiz = cls < 2;
    const int Lc = horiz ? p.W + 2 : p.H, n_line = horiz ? p.W : p.H;
    const int Mc = p.batch * Lc, Kc = p.Co;
    const int m0 = blockIdx.x * T::BM, n0 = blockIdx.y * T::BN;
    if (m0 >= Mc) return;                          // block-uniform, before any barrier: this class has fewer row tiles
    // dy pixel of line position j: pix0 + j * step
    const int pix0 = cls == 1 ? (p.H - 1) * p.W : (cls == 3 ? p.W - 1 : 0), step = horiz ? 1 : p.W, shift = horiz ? 0 : 1;

    const float* a_ptr[T::A_LD];
    bool a_ok[T::A_LD];
#pragma unroll
    for (int s = 0; s < T::A_LD; ++s) {
        const int m = m0 + T::a_row(s);
        const int mc = m < Mc ? m : 0;           // rows past Mc only feed output rows that are never stored
        const int b = mc / Lc;
        int j = mc - b * Lc + shift - tap;      // the line position this row's tap reads: fixed for the whole K loop
        a_ok[s] = j >= 0 && j < n_line;
        j = j < 0 ? 0 : (j < n_line ? j : n_line - 1);     // a valid address: the load is unconditional, the slot is staged as zeros
        a_ptr[s] = p.dy + ((int64_t)b * p.H * p.W + pix0 + (int64_t)j * step) * p.Co;
    }
    const int nslab = (Kc + H2_BK - 1) / H2_BK;
    const uint4* w_unit[T::B_LD];
#pragma unroll
    for (int s = 0; s < T::B_LD; ++s) {
        const int n = n0 + T::b_row(s);
        w_unit[s] = p.wsplit + (int64_t)(n < p.Ci ? n : 0) * H2_SLAB_UNITS + T::b_unit(s);
    }
    const int64_t w_slab = (int64_t)p.Ci * H2_SLAB_UNITS;
    const int slab0 = (int)blockIdx.z * p.slabs;
    auto ldA = [&](int s, int k, float4& v) -> bool {
        const bool ok = k < Kc;                            // k is the channel: a multiple of 4, so k < Co leaves four channels
        v = *reinterpret_cast<const float4*>(a_ptr[s] + (ok ? k : 0));
        return ok && a_ok[s];
    };
    auto ldB = [&](int s, int t) -> uint4 { return w_unit[s][(slab0 + (t < nslab ? t : nslab - 1)) * w_slab]; };

    f32x16 acc[1][TN];
    T::run(lds, Kc, ldA, ldB, acc);

    const float inv_s = p.scale->y;
    const int F = 2 * (p.W + 2) + 2 * p.H;
    const int off = cls == 0 ? 0 : (cls == 1 ? p.W + 2 : (cls == 2 ? 2 * (p.W + 2) : 2 * (p.W + 2) + p.H));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + T::row_of(0, r);
        if (m >= Mc) continue;
        const int b = m / Lc, i = m - b * Lc;
        float* row = p.gf + (((int64_t)tap * p.batch + b) * F + off + i) * p.Ci;
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
            const int n = n0 + T::col_of(jn);
            if (n < p.Ci) row[n] = acc[0][jn][r] * p.wscale[n] * inv_s;
        }
    }
}

// dx[y][x] += the frame terms (each the sum of its three tap planes, in tap order), rows of the frame first (top, bottom: u = x, then -1, then W), then the columns (left, right) at v = y.  The pixels of
// rows 1 and H - 2 come first (nry W of them), then those of columns 1 and W - 2 in the remaining rows.
__global__ __launch_bounds__(256) void td_rp_fold_kernel(const RpDgParams p, int nry, int ry0, int ry1, int ncx, int cx0, int cx1, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int na = nry * p.W + (p.H - nry) * ncx;           // affected pixels per image
    const int c = (int)(idx % p.Ci);
    const int64_t pa = idx / p.Ci;
    const int b = (int)(pa / na), a = (int)(pa - (int64_t)b * na);
    int y, x;
    if (a < nry * p.W) { const int q = a / p.W; y = q ? ry1 : ry0; x = a - q * p.W; }
    else {
        const int r = a - nry * p.W, q = r / ncx;
        x = (r - q * ncx) ? cx1 : cx0;
        y = q; if (y >= ry0) ++y; if (nry == 2 && y >= ry1) ++y;
    }
    const int F = 2 * (p.W + 2) + 2 * p.H;
    const int64_t plane = (int64_t)p.batch * F * p.Ci;
    auto term = [&](const float* q) { return (q[0] + q[plane]) + q[2 * plane]; };
    const float* g = p.gf + (int64_t)b * F * p.Ci + c;
    const float* top = g, *bot = g + (int64_t)(p.W + 2) * p.Ci, *lef = g + (int64_t)2 * (p.W + 2) * p.Ci, *rig = lef + (int64_t)p.H * p.Ci;
    float* d = p.dx + (((int64_t)b * p.H + y) * p.W + x) * p.Ci + c;
    const bool xl = x == 1, xr = x == p.W - 2;
    float s = *d;
    if (y == 1) {
        s += term(top + (int64_t)(x + 1) * p.Ci);
        if (xl) s += term(top);
        if (xr) s += term(top + (int64_t)(p.W + 1) * p.Ci);
    }
    if (y == p.H - 2) {
        s += term(bot + (int64_t)(x + 1) * p.Ci);
        if (xl) s += term(bot);
        if (xr) s += term(bot + (int64_t)(p.W + 1) * p.Ci);
    }
    if (xl) s += term(lef + (int64_t)y * p.Ci);
    if (xr) s += term(rig + (int64_t)y * p.Ci);
    *d = s;
}

struct RpDgradLayout { size_t wf, wsplit, gf, total; };
static RpDgradLayout td_rp_dgrad_layout(int batch, int H, int W, int Ci, int Co) {
    RpDgradLayout l{};
    const int Ktot = 12 * td_rp_span(Co);
    l.wf = td_dgrad_layout(batch, H, W, Ci, Co).total;                       // the interior launch's workspace comes first, as it is
    l.wsplit = l.wf + td_up256((size_t)Ci * Ktot * sizeof(float));
    l.gf = l.wsplit + td_up256(xp_split_weights_h2_bytes(Ci, Ktot));
    l.total = l.gf + td_up256((size_t)3 * batch * td_rp_frame(H, W) * Ci * sizeof(float));
    return l;
}
static bool td_rp_shape_ok(int batch, int H, int W, int Ci, int Co) {
    // the limits of the zero-padded input gradient, reflection's two pixels, and the rearranged weight's 12 Ci pad32(Co) elements indexed as int
    return td_conv_shape_ok(batch, H, W, Ci, Co) && H >= 2 && W >= 2 && (int64_t)12 * Ci * td_rp_span(Co) < ((int64_t)1 << 31);
}

template <int TN>
static int td_rp_frame_launch(const RpDgParams& p, hipStream_t s) {
    using T = GemmTileH2<2, 2, 1, TN>;
    const int64_t m_max = (int64_t)p.batch * max(p.W + 2, p.H);
    hipLaunchKernelGGL(td_rp_frame_kernel<TN>, dim3((unsigned)xp_cdiv(m_max, (int64_t)T::BM), xp_cdiv(p.Ci, T::BN), 12), dim3(256), 0, s, p);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

}  // namespace

extern "C" size_t xp_conv3x3_rp_dgrad_h2_workspace_bytes(int batch, int H, int W, int Ci, int Co) {
    if (!td_rp_shape_ok(batch, H, W, Ci, Co)) return 0;
    return td_rp_dgrad_layout(batch, H, W, Ci, Co).total;
}

extern "C" int xp_conv3x3_rp_dgrad_h2(const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(dy && w && dx, "xp_conv3x3_rp_dgrad_h2: null pointer");
    XP_CHECK_ARG(td_rp_shape_ok(batch, H, W, Ci, Co), "xp_conv3x3_rp_dgrad_h2: bad shape batch=%d H=%d W=%d Ci=%d Co=%d (reflection needs H, W >= 2)",
                 batch, H, W, Ci, Co);
    XP_CHECK_ARG(Co % 4 == 0, "xp_conv3x3_rp_dgrad_h2: Co must be a multiple of 4 (got %d): the engine loads dy in 4-element channel groups", Co);
    XP_CHECK_ARG(((uintptr_t)dy & 15) == 0, "xp_conv3x3_rp_dgrad_h2: dy must be 16-byte aligned");
    const RpDgradLayout l = td_rp_dgrad_layout(batch, H, W, Ci, Co);
    XP_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= l.total,
                 "xp_conv3x3_rp_dgrad_h2: workspace of %zu bytes, 256-byte aligned, needed (got %zu)", l.total, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    // the interior term g[y][x]: the zero-padded input gradient as it stands, in the head of the workspace
    XP_TRY(xp_conv3x3_dgrad_h2(dy, w, dx, batch, H, W, Ci, Co, dy_scale, workspace, l.wf, stream));
    const float2* scale = (const float2*)dy_scale;
    if (!dy_scale) {          // it left {S, 1 / S} and the scaled copy of dy in its workspace
        scale = (const float2*)(ws + AMAX_PARTS * 4);
        dy = (const float*)(ws + td_dgrad_layout(batch, H, W, Ci, Co).dys);
    }
    const int span = td_rp_span(Co), Ktot = 12 * span;
    float* wf = (float*)(ws + l.wf);
    hipLaunchKernelGGL(td_rp_weights_kernel, dim3(xp_cdiv(Ci * Ktot, 256)), dim3(256), 0, s, w, wf, Ci, Co, span);
    XP_LAUNCH_CHECK();
    XP_TRY(xp_split_weights_h2(wf, ws + l.wsplit, Ci, Ktot, stream));
    RpDgParams p{};
    p.dy = dy; p.wsplit = (const uint4*)(ws + l.wsplit); p.wscale = h2_scales(ws + l.wsplit, Ci, Ktot); p.scale = scale;
    p.gf = (float*)(ws + l.gf); p.dx = dx;
    p.batch = batch; p.H = H; p.W = W; p.Ci = Ci; p.Co = Co; p.slabs = span / H2_BK;
    const int64_t frame_rows = (int64_t)batch * td_rp_frame(H, W);
    {
        XpProfScope prof("conv3x3_rp_dgrad_frame_h2", s, 6.0 * frame_rows * 3.0 * Ci * Co, 4.0 * frame_rows * (3.0 * Co + Ci));
        XP_TRY(Ci <= 64 ? td_rp_frame_launch<1>(p, s) : td_rp_frame_launch<2>(p, s));
    }
    // rows {1, H - 2} and columns {1, W - 2} as sets: H = 2 gives {0, 1} (H - 2 first does not matter: the order inside a pixel's sum is fixed), H = 3 {1}
    const int ry0 = min(1, H - 2), ry1 = max(1, H - 2), nry = ry0 == ry1 ? 1 : 2;
    const int cx0 = min(1, W - 2), cx1 = max(1, W - 2), ncx = cx0 == cx1 ? 1 : 2;
    const int64_t total = (int64_t)batch * (nry * W + (H - nry) * ncx) * Ci;
    XpProfScope prof("conv3x3_rp_dgrad_fold", s, 0.0, 16.0 * total);
    hipLaunchKernelGGL(td_rp_fold_kernel, dim3((unsigned)xp_cdiv(total, (int64_t)256)), dim3(256), 0, s, p, nry, ry0, ry1, ncx, cx0, cx1, total);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

// ---- one power of two for a gradient that arrives from elsewhere (the block's incoming dy, the scan / cross-scan backward): DESIGN.md §16 ----
extern "C" size_t xp_scale_grad_workspace_bytes(void) { return WG_HEAD_BYTES; }

extern "C" int xp_scale_grad(const float* g, float* out, int64_t n, float* scale_out, void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(g && out && scale_out && n > 0 && n < ((int64_t)1 << 40), "xp_scale_grad: null pointer or bad n = %lld", (long long)n);
    XP_CHECK_ARG(workspace && workspace_bytes >= (size_t)WG_HEAD_BYTES, "xp_scale_grad: workspace of %d bytes needed", WG_HEAD_BYTES);
    hipStream_t s = (hipStream_t)stream;
    float* amax = (float*)workspace;
    float2* scale = (float2*)scale_out;
    // the flat vector as (n / 256) rows of 256 and one tail row: the walks of the weight gradient's amax / scale kernels, no second copy
    const int64_t rows = n / 256;
    const int tail = (int)(n - rows * 256);
    const int nb = rows ? (int)min((int64_t)AMAX_PARTS - 1, (rows + 3) / 4) : 0;
    XpProfScope prof("scale_grad", s, 0.0, 12.0 * n);
    if (rows) { hipLaunchKernelGGL(td_amax_kernel, dim3(nb), dim3(256), 0, s, g, rows, 256, 256, amax); XP_LAUNCH_CHECK(); }
    if (tail) { hipLaunchKernelGGL(td_amax_kernel, dim3(1), dim3(256), 0, s, g + rows * 256, (int64_t)1, tail, tail, amax + nb); XP_LAUNCH_CHECK(); }
    hipLaunchKernelGGL(td_scale_kernel, dim3(1), dim3(256), 0, s, amax, nb + (tail ? 1 : 0), scale);
    XP_LAUNCH_CHECK();
    if (out == g) {
        if (rows) { hipLaunchKernelGGL(td_mul_scale_kernel, dim3(nb), dim3(256), 0, s, out, rows, 256, 256, scale); XP_LAUNCH_CHECK(); }
        if (tail) { hipLaunchKernelGGL(td_mul_scale_kernel, dim3(1), dim3(256), 0, s, out + rows * 256, (int64_t)1, tail, tail, scale); XP_LAUNCH_CHECK(); }
    } else {
        if (rows) { hipLaunchKernelGGL(td_scaled_copy_kernel, dim3(nb), dim3(256), 0, s, g, out, rows, 256, scale); XP_LAUNCH_CHECK(); }
        if (tail) { hipLaunchKernelGGL(td_scaled_copy_kernel, dim3(1), dim3(256), 0, s, g + rows * 256, out + rows * 256, (int64_t)1, tail, scale); XP_LAUNCH_CHECK(); }
    }
    return XP_OK;
}
