// Row walks and fixed-order column sums shared by the training kernels (train_dense.hip, train_vss.hip): one definition each, so the BatchNorm sums,
// the bias sums and the LayerNorm / depthwise-convolution parameter gradients reduce in the same order.
#pragma once
#include "xp_common.h"

namespace {

// element-wise walks: a block is 4 rows x 64 channel lanes (one wave per row, 256-byte segments), rows strided by the grid: no division per element
template <class F>
__device__ __forceinline__ void td_for_each(int64_t rows, int C, F f) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4)
        for (int c = lane; c < C; c += 64) f(r, c);
}


// ---- per-channel sums over (rows x C) in a fixed order ----
// A block is 32 channels x 8 row lanes; BN_PARTS blocks share the rows of a channel group (row r belongs to part (r / 8) % BN_PARTS, lane r % 8).  Every
// thread accumulates in f64 (as det_reduce_kernel does), the 8 lanes are added in lane order, and the finishing kernels add the parts in part order.
constexpr int BN_PARTS = 64;

template <int NQ, class F>
__device__ __forceinline__ void td_colsum_parts(int64_t rows, int C, double* __restrict__ part, F f) {
    __shared__ double sm[NQ][8][32];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5, c = blockIdx.x * 32 + cl, pt = blockIdx.y;
    double a[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) a[q] = 0.0;
    if (c < C) {
#pragma unroll 4
        for (int64_t r = (int64_t)pt * 8 + rl; r < rows; r += BN_PARTS * 8) f(r, c, a);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) sm[q][rl][cl] = a[q];
    __syncthreads();
    if (rl == 0 && c < C) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            double s = sm[q][0][cl];
            for (int k = 1; k < 8; ++k) s += sm[q][k][cl];
            part[((size_t)pt * NQ + q) * C + c] = s;
        }
    }
}
__device__ __forceinline__ double td_sum_parts(const double* __restrict__ part, int NQ, int q, int C, int c) {
    double s = part[(size_t)q * C + c];
    for (int k = 1; k < BN_PARTS; ++k) s += part[((size_t)k * NQ + q) * C + c];
    return s;
}

}  // namespace
