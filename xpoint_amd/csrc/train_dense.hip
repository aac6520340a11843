// Dense backward of training, the part that REDUCES OVER ROWS: the weight-gradient GEMM on the split-fp16 matrix path with its four
// operand forms (a matrix; the implicit im2col of the 3x3 convolution under reflection padding, under zero padding, and under zero padding at stride 2) and
// the stem's weight gradient; the norms over NHWC rows — BatchNorm training forward / backward, the column sums behind the bias gradients, the L2-normalise
// backward; and the gradient-scale kernels with the helper of train_scale.h and xp_scale_grad, their entry point.  The input gradients of the convolutions
// are in train_dgrad.hip; the row walks and the fixed-order column sums in train_rows.h, which train_vss.hip shares.
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
#include "train_scale.h"
#include "xpoint_hip.h"

namespace {

constexpr int WG_CHUNK = 256;        // rows of M per partial sum (XP_WGRAD_CHUNK in the header)
constexpr int WG_BT = 64;            // output tile side of a workgroup: 2 x 2 waves of one 32 x 32 accumulator tile

static_assert(WG_CHUNK == XP_WGRAD_CHUNK, "the header quotes the chunk length");

// ---- largest magnitude of a (rows x C, ld) matrix and its power of two: maxima are order-free, hence deterministic ----
__global__ __launch_bounds__(256) void td_amax_kernel(const float* __restrict__ x, int64_t rows, int C, int ld, float* __restrict__ part) {
    float m = 0.f;
    td_for_each(rows, C, [&](int64_t r, int c) { m = fmaxf(m, fabsf(x[r * ld + c])); });
    m = xp_block_max256(m);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// scale = {S, 1 / S} with max|x| S in [2^13, 2^14); S = 1 for an all-zero operand.  fmaxf drops NaN and an infinite maximum gives S = 1: non-finite elements
// take no part in the choice and pass through the split as they are (NaN / Inf in the planes, hence in the results they touch)
__global__ __launch_bounds__(256) void td_scale_kernel(const float* __restrict__ part, int nparts, float2* __restrict__ scale) {
    float m = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) m = fmaxf(m, part[i]);
    m = xp_block_max256(m);
    if (threadIdx.x == 0) {
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
__global__ __launch_bounds__(256) void td_scaled_copy_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t rows, int C, const float2* __restrict__ scale) {
    const float S = scale->x;
    td_for_each(rows, C, [&](int64_t r, int c) { y[r * C + c] = x[r * C + c] * S; });
}

}  // namespace

int xp_scale_from_parts(const float* parts, const XpScaleWalk& w, float2* scale, XpScaleApply apply, const float* x, float* out, hipStream_t s) {
    int nparts = 0;
    for (int i = 0; i < w.npieces; ++i) nparts += w.piece[i].blocks;
    hipLaunchKernelGGL(td_scale_kernel, dim3(1), dim3(256), 0, s, parts, nparts, scale);
    XP_LAUNCH_CHECK();
    for (int i = 0; i < w.npieces && apply != XP_SCALE_ONLY; ++i) {
        const auto& q = w.piece[i];
        if (apply == XP_SCALE_IN_PLACE) hipLaunchKernelGGL(td_mul_scale_kernel, dim3(q.blocks), dim3(256), 0, s, out + q.off, q.rows, q.C, q.ld, (const float2*)scale);
        else hipLaunchKernelGGL(td_scaled_copy_kernel, dim3(q.blocks), dim3(256), 0, s, x + q.off, out + q.off, q.rows, q.C, (const float2*)scale);
        XP_LAUNCH_CHECK();
    }
    return XP_OK;
}

int xp_own_scale(const float* x, const XpScaleWalk& w, float* parts, float2* scale, XpScaleApply apply, float* out, hipStream_t s) {
    int nparts = 0;
    for (int i = 0; i < w.npieces; ++i) {
        const auto& q = w.piece[i];
        hipLaunchKernelGGL(td_amax_kernel, dim3(q.blocks), dim3(256), 0, s, x + q.off, q.rows, q.C, q.ld, parts + nparts);
        XP_LAUNCH_CHECK();
        nparts += q.blocks;
    }
    return xp_scale_from_parts(parts, w, scale, apply, x, out, s);
}

namespace {

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
    return XP_SCALE_HEAD_BYTES + (size_t)xp_cdiv(M, WG_CHUNK) * I * J * sizeof(float);
}

static int td_wgrad_launch(const char* who, int conv, WgParams p, float* out, int ldo, const float* p_scale, void* ws, size_t ws_bytes, hipStream_t s) {
    XP_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0 && ws_bytes >= td_wgrad_bytes(p.M, p.I, p.J), "%s: workspace of %zu bytes, 256-byte aligned, needed (got %zu)",
                 who, td_wgrad_bytes(p.M, p.I, p.J), ws_bytes);
    XP_CHECK_ARG((int64_t)p.I * p.J < (1 << 30) && (int64_t)p.M * (int64_t)max(p.ldp, p.ldq) < ((int64_t)1 << 40), "%s: shape too large", who);
    p.part = (float*)((char*)ws + XP_SCALE_HEAD_BYTES);
    const int nchunk = xp_cdiv(p.M, WG_CHUNK);
    if (p_scale) {
        p.scale = (const float2*)p_scale; p.prescaled = 1;
    } else {
        XP_TRY(xp_own_scale(p.P, xp_walk_rows(p.M, p.I, p.ldp), (float*)ws, xp_head_scale(ws), XP_SCALE_ONLY, nullptr, s));
        p.scale = xp_head_scale(ws); p.prescaled = 0;
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

// the three implicit forms: P = dy, one row of Co per pixel of the (Ho, Wo) output grid, Q = the NHWC input read through the 3x3 taps
static int td_conv_wgrad(const char* who, int conv, const float* x, const float* dy, float* dw, int batch, int H, int W, int Ci, int Co, int Ho, int Wo,
                         const float* dy_scale, void* ws, size_t ws_bytes, void* stream) {
    WgParams p{};
    p.P = dy; p.Q = x; p.M = batch * Ho * Wo; p.I = Co; p.J = 9 * Ci; p.ldp = Co; p.H = H; p.W = W; p.Ci = Ci; p.Ho = Ho; p.Wo = Wo;
    return td_wgrad_launch(who, conv, p, dw, 9 * Ci, dy_scale, ws, ws_bytes, (hipStream_t)stream);
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
        m = xp_block_max256(m);
        if (threadIdx.x == 0) amax_part[blockIdx.x] = m;
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
    return ((size_t)BN_PARTS * 2 * C * sizeof(double) + (size_t)C * sizeof(double2) + XP_AMAX_PARTS * sizeof(float) + 255) & ~(size_t)255;
}
static int td_rows_check(const char* who, int64_t rows, int C) {
    XP_CHECK_ARG(rows > 0 && C > 0 && rows < ((int64_t)1 << 31) && C <= (1 << 20), "%s: bad shape rows=%lld C=%d", who, (long long)rows, C);
    return XP_OK;
}

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
static size_t td_stem_wgrad_bytes(int Co) { return Co > 0 ? xp_up256((size_t)BN_PARTS * 9 * Co * sizeof(double)) : 0; }

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
    return td_conv_wgrad("xp_conv3x3_wgrad_h2", 1, x, dy, dw, batch, H, W, Ci, Co, H, W, dy_scale, workspace, workspace_bytes, stream);
}

extern "C" int xp_conv3x3_zp_wgrad_h2(const float* x, const float* dy, float* dw, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(x && dy && dw, "xp_conv3x3_zp_wgrad_h2: null pointer");
    XP_CHECK_ARG(xp_conv_grad_shape_ok(batch, H, W, Ci, Co, 26), "xp_conv3x3_zp_wgrad_h2: bad shape batch=%d H=%d W=%d Ci=%d Co=%d", batch, H, W, Ci, Co);
    return td_conv_wgrad("xp_conv3x3_zp_wgrad_h2", 2, x, dy, dw, batch, H, W, Ci, Co, H, W, dy_scale, workspace, workspace_bytes, stream);
}

extern "C" int xp_conv3x3_s2_wgrad_h2(const float* x, const float* dy, float* dw, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(x && dy && dw, "xp_conv3x3_s2_wgrad_h2: null pointer");
    XP_CHECK_ARG(xp_conv_grad_shape_ok(batch, H, W, Ci, Co, 24), "xp_conv3x3_s2_wgrad_h2: bad shape batch=%d H=%d W=%d Ci=%d Co=%d", batch, H, W, Ci, Co);
    return td_conv_wgrad("xp_conv3x3_s2_wgrad_h2", 3, x, dy, dw, batch, H, W, Ci, Co, (H - 1) / 2 + 1, (W - 1) / 2 + 1, dy_scale, workspace, workspace_bytes,
                         stream);
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
    hipLaunchKernelGGL(td_bn_apply_kernel, dim3(xp_elem_blocks(rows)), dim3(256), 0, s, x, ldx, save_mean, save_invstd, gamma, beta, rows, C, y, ldy);
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
    hipLaunchKernelGGL(td_bn_bwd_dx_kernel, dim3(xp_elem_blocks(rows)), dim3(256), 0, s, dy, lddy, x, ldx, save_mean, save_invstd, gamma, means, rows, C, relu_mask,
                       dx, lddx, dx_scale ? amax : nullptr);
    XP_LAUNCH_CHECK();
    // the dx kernel left one partial maximum per block of its walk
    return dx_scale ? xp_scale_from_parts(amax, xp_walk_rows(rows, C, lddx), (float2*)dx_scale, XP_SCALE_IN_PLACE, nullptr, dx, s) : XP_OK;
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

// ---- one power of two for a gradient that arrives from elsewhere (the block's incoming dy, the scan / cross-scan backward): DESIGN.md §16 ----
extern "C" size_t xp_scale_grad_workspace_bytes(void) { return XP_SCALE_HEAD_BYTES; }

extern "C" int xp_scale_grad(const float* g, float* out, int64_t n, float* scale_out, void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(g && out && scale_out && n > 0 && n < ((int64_t)1 << 40), "xp_scale_grad: null pointer or bad n = %lld", (long long)n);
    XP_CHECK_ARG(workspace && workspace_bytes >= XP_SCALE_HEAD_BYTES, "xp_scale_grad: workspace of %d bytes needed", (int)XP_SCALE_HEAD_BYTES);
    hipStream_t s = (hipStream_t)stream;
    XpProfScope prof("scale_grad", s, 0.0, 12.0 * n);
    // the flat vector as rows of 256 and one tail row: the walks of the weight gradient's amax / scale kernels, no second copy
    return xp_own_scale(g, xp_walk_flat(n), (float*)workspace, (float2*)scale_out, out == g ? XP_SCALE_IN_PLACE : XP_SCALE_COPY, out, s);
}
