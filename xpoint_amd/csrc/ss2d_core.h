// What the two forms of the fused SS2D core share (ss2d.hip has the operator's description): the launch parameters, one scan step's operand evaluation, the
// matrix-pipe dt projection, the list of instantiated dt_ranks and the two launch functions the host code (ss2d.hip) reaches the forms through —
// ss2d_chunked.hip: the chunked three-pass form (stages 0-1); ss2d_seq.hip: the sequential form (deep stages).
#pragma once
#include <type_traits>

#include "gemm_h2_core.h"
#include "xp_common.h"

#ifndef XP_SS2D_DBG
#define XP_SS2D_DBG 0   /* timing experiments only (wrong results): 1 no out_norm tail, 2 no loads of the row pair's partial sums, 4 no step arithmetic (projection, softplus, exp), 8 no u loads */
#endif

// (What follows is at global scope, not in an anonymous namespace, because ss2d.hip, ss2d_chunked.hip and ss2d_seq.hip must agree on it: SS2DParams,
//  DtWeights, SS2DRankList / SS2DRanks, XP_L2E and the inline device helpers must stay unique among the library's translation units.)
constexpr float XP_L2E =1.44269504088896340736f;   // log2(e): folded into the dt weights, the dt bias and A where they are loaded

struct SS2DParams {
    const float* u;      // (B, H, W, C)   after dwconv + SiLU
    const float* xdbl;   // (B*H*W, 4*(R+2))  [pair][dir][dtr(R), B, C]
    const float* wdt;    // (4, R, C)  directions in the order (0,2,1,3); channel-contiguous so that a wave's weight loads coalesce
    const float* dtb;    // (4, C)
    const float* A;      // (4, C)    = -exp(A_logs)
    const float* Dp;     // (4, C)
    const float* ln_w;   // (C) out_norm
    const float* ln_b;
    float* wsP;          // (B, 2, nc, 2, C)
    float* wsS;          // same; pass 2 overwrites S with the chunk start state
    float* ya;           // (B, H, W, C) row-pair partial
    float* out;          // (B, H, W, C)
    int out_p32;         // sequential form only: out is the P32 image [row][c / 32][plane][32] of the result (ring_core.h), not f32 rows
    int Bn, H, W, C, T, nc, cpb;
    float eps;
};

__device__ __forceinline__ int pixel_of(int l, int L, int H, int W, bool colmajor) {
    if (l >= L) return -1;
    if (!colmajor) return l;
    int w = l / H, h = l - w * H;   // route 1: l = w*H + h   (x.transpose(2,3).flatten)
    return h * W + w;
}

// One scan step's operands for one route: xr = [dt_rank values, B, C] (R + 2 floats, 8-byte aligned in LDS; 16-byte
// aligned when (R + 2) % 4 == 0).  Read with the widest aligned LDS loads (b128 / b64 broadcasts), not R + 2 b32 reads.
// AMP (mixed-precision class, xp_set_amp_mode): the dt projection is a half convolution under autocast — its output is rounded to fp16 BEFORE
// the f32 bias is added (csms6s.py:47-50 adds delta_bias to the half tensor in f32) — so w and bias arrive WITHOUT the log2(e) factor
template <int R, bool AMP = false>
__device__ __forceinline__ void step_vals(const float* __restrict__ xr, const float (&w)[R], float bias, float A,
                                          float u, float& a, float& b, float& Cv) {
    float xv[R + 2];
    if constexpr ((R + 2) % 4 == 0) {
#pragma unroll
        for (int q = 0; q < (R + 2) / 4; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(xr + 4 * q);
            xv[4 * q] = t.x; xv[4 * q + 1] = t.y; xv[4 * q + 2] = t.z; xv[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < (R + 2) / 2; ++q) {
            const float2 t = *reinterpret_cast<const float2*>(xr + 2 * q);
            xv[2 * q] = t.x; xv[2 * q + 1] = t.y;
        }
    }
    if (XP_SS2D_DBG & 4) { a = 0.5f; b = xv[R] * u; Cv = xv[R + 1]; return; }
    // w, bias and A arrive pre-multiplied by log2(e) (XP_L2E at their loads): the chain below is x * log2(e) directly
    float dt;
    if constexpr (!AMP) {
        dt = fmaf(w[0], xv[0], bias);
#pragma unroll
        for (int r = 1; r < R; ++r) dt = fmaf(w[r], xv[r], dt);
    } else {
        dt = w[0] * xv[0];
#pragma unroll
        for (int r = 1; r < R; ++r) dt = fmaf(w[r], xv[r], dt);
        dt = ((float)(_Float16)dt + bias) * XP_L2E;
    }
    float delta;
    xp_softplus_decay_l2(dt, A, delta, a);          // softplus + exp(delta * A): xp_common.h
    b = delta * xv[R] * u;
    Cv = xv[R + 1];
}

// ---- dt projection of a 32-pixel tile on the matrix pipe (dt_rank >= 12: the deep stages) ------------------------------------------
//   dt[pixel][channel] = bias[channel] + sum_r x[pixel][r] Wdt[channel][r]   for the wave's 64 channels: two 32x32 MFMA tiles x ceil(R / 16)
// slabs, both operands split into two fp16 planes, three products per slab (gemm_h2_core.h: operand error <= 2^-23, per product <= 2^-21 worst / ~2^-25 typical — f32-grade) instead of R
// FMAs per step and lane.  The weight fragments stay in registers (as many as the R scalar weights they replace), the pixel rows are split
// from the LDS tile.  The accumulator layout (lane = column = channel, 16 registers = rows {0-3, 8-11, 16-19, 24-27} + 4 (lane >> 5))
// becomes "lane = channel, 32 registers = the tile's 32 pixels" with one v_permlane32_swap per register pair of the two tiles — the
// scan's own layout: dt of tile pixel j is dtv[(j >> 2) & 1][(j & 3) + 4 (j >> 3)].
template <int R>
struct DtWeights {
    static constexpr int KS = (R + 15) / 16;
    f16x8_t bw[2][KS][2];                                               // [channel tile][k slab][plane]
    float bias[2];
    float bias_lane;                                                    // AMP: the unscaled bias of channel cbase + lane (the layout AFTER dt_tile's lane swap)
};
__device__ __forceinline__ void dt_split8(const float (&v)[8], f16x8_t& hi, f16x8_t& lo) {
    uint2 a0, a1, b0, b1;
    h2_split4(make_float4(v[0], v[1], v[2], v[3]), a0, a1);
    h2_split4(make_float4(v[4], v[5], v[6], v[7]), b0, b1);
    union { uint4 u; f16x8_t h; } x, y;
    x.u = make_uint4(a0.x, a0.y, b0.x, b0.y); y.u = make_uint4(a1.x, a1.y, b1.x, b1.y);
    hi = x.h; lo = y.h;
}
// wdt_dir: (R, C) weights of one direction, dtb_dir: (C); cbase: first of the wave's 64 channels.  log2(e) folded in (see step_vals).
// AMP (mixed-precision classes): the projection is a half convolution whose output is rounded to fp16 BEFORE the f32 bias is added (see step_vals): weights
// and bias arrive without the log2(e) factor, the accumulator starts at 0, and dt_tile finishes with (r16(acc) + bias) * log2(e)
template <int R, bool AMP = false>
__device__ __forceinline__ void dt_load_weights(DtWeights<R>& w, const float* __restrict__ wdt_dir, const float* __restrict__ dtb_dir, int C, int cbase) {
    constexpr float WL2E = AMP ? 1.f : XP_L2E;
    const int fr = threadIdx.x & 31, fh = (threadIdx.x >> 5) & 1;
    w.bias_lane = dtb_dir[cbase + (threadIdx.x & 63)];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cj = cbase + 32 * j + fr;
        w.bias[j] = AMP ? 0.f : XP_L2E * dtb_dir[cj];
#pragma unroll
        for (int ks = 0; ks < DtWeights<R>::KS; ++ks) {
            float wv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int r = ks * 16 + fh * 8 + e;                     // clamped unconditional load + select: no branch per element
                const float t = wdt_dir[(int64_t)(r < R ? r : 0) * C + cj];
                wv[e] = r < R ? WL2E * t : 0.f;
            }
            dt_split8(wv, w.bw[j][ks][0], w.bw[j][ks][1]);
        }
    }
}
// rows: LDS, tile pixel i's dt_rank values at rows + i * stride (floats, 8-byte aligned)
template <int R, bool AMP = false>
__device__ __forceinline__ void dt_tile(const DtWeights<R>& w, const float* rows, int stride, float (&dtv)[2][16]) {
    const int fr = threadIdx.x & 31, fh = (threadIdx.x >> 5) & 1;
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        // (the accumulators' start value is the same for every tile; opaque here so that the two 16-register start tuples are rebuilt per tile — 32 moves —
        //  instead of being hoisted out of the caller's tile loop and held beside the working accumulators for the whole kernel)
        float b0 = w.bias[j];
        if constexpr (!AMP) asm volatile("" : "+v"(b0));                // (AMP starts from the constant 0)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = b0;
    }
#pragma unroll
    for (int ks = 0; ks < DtWeights<R>::KS; ++ks) {
        const int k0 = ks * 16 + fh * 8;
        const float* ar = rows + fr * stride + (k0 < R ? k0 : 0);      // a half slab wholly past R reads the row start instead and is cleared
        float v[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float2 t = *reinterpret_cast<const float2*>(ar + 2 * q);
            v[2 * q] = k0 + 2 * q < R ? t.x : 0.f;                      // (R is even: a float2 is inside or outside as a whole)
            v[2 * q + 1] = k0 + 2 * q < R ? t.y : 0.f;
        }
        f16x8_t hi, lo;
        dt_split8(v, hi, lo);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(lo, w.bw[j][ks][0], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hi, w.bw[j][ks][1], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hi, w.bw[j][ks][0], acc[j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[0][e]), __float_as_uint(acc[1][e]), false, false);
        dtv[0][e] = __uint_as_float(sw[0]); dtv[1][e] = __uint_as_float(sw[1]);
        if constexpr (AMP) {
            dtv[0][e] = ((float)(_Float16)dtv[0][e] + w.bias_lane) * XP_L2E;
            dtv[1][e] = ((float)(_Float16)dtv[1][e] + w.bias_lane) * XP_L2E;
        }
    }
}
#define XP_DTV(dtv, j) (dtv)[((j) >> 2) & 1][((j) & 3) + 4 * ((j) >> 3)]

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// THE list of dt_ranks every kernel of both forms is instantiated for.  dispatch calls f(std::integral_constant<int, R>) for the listed rank equal to R
// and says whether there was one.
template <int... Rs>
struct SS2DRankList {
    static bool has(int R) { return ((R == Rs) || ...); }
    template <typename F>
    static bool dispatch(int R, F&& f) { return ((R == Rs && (f(std::integral_constant<int, Rs>{}), true)) || ...); }
};
using SS2DRanks = SS2DRankList<2, 4, 6, 8, 12, 16, 24, 48>;

// One launch function per form; each dispatches over SS2DRanks in its own file (a rank outside the list: XP_ERR_ARG, nothing launched).
// half_io: the fp16-storage class (u / xdbl / out are halves).  The chunked form reads xp_amp_value() itself (the f32-container mixed-precision class).
int ss2d_launch_chunked(const SS2DParams& p, int R, bool half_io, hipStream_t s);                   // ss2d_chunked.hip
// ys: the four routes' y, 4 (B, H, W, C) planes.  half_out: the fp16-storage class — p.u / p.xdbl are f32 COPIES of the half tensors, out is stored as fp16
int ss2d_launch_seq(const SS2DParams& p, float* ys, int R, bool half_out, hipStream_t s);           // ss2d_seq.hip
bool ss2d_seq_scan2_applies(int R, int H, int W, int C);                                                 // ss2d_seq.hip
