// Matching evaluation for a batch of pairs (include/xpoint_hip.h, xp_pair_eval_*; DESIGN.md "Matching evaluation"): the device work of the
// reference's compute_repeatability_for_sample (benchmark_evaluation.py:396-467), compute_descriptor_for_sample (:588-751) and the corner
// error of compute_pts_dist_for_sample (:755-830), on the ragged layout the pipeline already uses: kp (2*pairs, cap, 2) int32 (y, x), optical
// images first, counts (2*pairs); match lists as xp_match_mnn writes them.
//
// All four are latency-sized (a few thousand points per image): what they buy is that a batch is four launches instead of a host loop with
// several read-backs per sample.  Nothing is accumulated in floats across lanes (the minimum is per lane, the counts are integers), so every
// quantity of pair p is what the pair gives alone and two calls agree bit for bit.  The library is built with -ffp-contract=off: the f64
// expressions below are evaluated as written, which is what the numpy restatement (tests/pair_eval_cases.py) states.
#include "xp_common.h"
#include "near_walk.h"

namespace {

constexpr int PE_TILE = 256;          // staged keypoints of the other image per LDS tile (= the block: one lane stages one point)
constexpr int PE_MAX_T = 16;          // thresholds per counting launch
constexpr double PE_INT64_MIN = -9223372036854775808.0;

struct PeThresholds {
    float v[PE_MAX_T];
};

__device__ __forceinline__ int pe_rows(const int* __restrict__ counts, int img, int cap) { return min(max(counts[img], 0), cap); }

// evaluation.warp_keypoints (homographies.py:479-497): (x, y, 1) . h^T, divided by the third coordinate; h row-major, acting on (x, y, 1)
__device__ __forceinline__ void pe_warp(const double* __restrict__ h, double y, double x, double& oy, double& ox) {
    const double u = (x * h[0] + y * h[1]) + h[2];
    const double v = (x * h[3] + y * h[4]) + h[5];
    const double w = (x * h[6] + y * h[7]) + h[8];
    ox = u / w;
    oy = v / w;
}

// numpy's float64 -> int64 astype as a double: toward zero, INT64_MIN for what does not fit (NaN included); "+ 0.0" turns -0.0 into 0.0
__device__ __forceinline__ double pe_trunc(double v) { return fabs(v) < 9223372036854775808.0 ? trunc(v) + 0.0 : PE_INT64_MIN; }

// grid (ceil(cap / 256), 2*pairs): one lane owns one query keypoint of image blockIdx.y; the other image's list goes through LDS in tiles,
// walked by xp_near_walk (near_walk.h) — the loop xp_points_min_dist runs, which is why the batched and per-sample paths agree bit for bit.
__global__ __launch_bounds__(256) void pair_eval_warp_near_kernel(const int* __restrict__ kp, const int* __restrict__ counts, int pairs, int cap,
                                                                  int H, int W, const double* __restrict__ map1, const double* __restrict__ map2,
                                                                  int truncate, double* __restrict__ warped, uint8_t* __restrict__ inframe,
                                                                  float* __restrict__ near_dist) {
    __shared__ double s_b[PE_TILE][2];
    const int img = blockIdx.y, other = img < pairs ? img + pairs : img - pairs;
    const int n = pe_rows(counts, img, cap), m = pe_rows(counts, other, cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    double wy = 0.0, wx = 0.0;
    if (live) {
        const int* k = kp + ((size_t)img * cap + i) * 2;
        pe_warp(map1 + (size_t)img * 9, (double)k[0], (double)k[1], wy, wx);
        if (truncate) { wy = pe_trunc(wy); wx = pe_trunc(wx); }
        if (map2) {
            pe_warp(map2 + (size_t)img * 9, wy, wx, wy, wx);
            if (truncate) { wy = pe_trunc(wy); wx = pe_trunc(wx); }
        }
    }
    float best = INFINITY;
    if (blockIdx.x * 256 < n) {                       // block-uniform: a block of filler rows stages nothing
        for (int j0 = 0; j0 < m; j0 += PE_TILE) {
            const int cnt = min(PE_TILE, m - j0);
            __syncthreads();
            if ((int)threadIdx.x < cnt) {
                const int* k = kp + ((size_t)other * cap + j0 + threadIdx.x) * 2;
                s_b[threadIdx.x][0] = (double)(float)k[0];          // kp.float(): the reference's list is float32
                s_b[threadIdx.x][1] = (double)(float)k[1];
            }
            __syncthreads();
            best = xp_near_walk(wy, wx, s_b, cnt, best);
        }
    }
    if (i < cap) {
        const size_t o = (size_t)img * cap + i;
        warped[2 * o] = live ? wy : 0.0;
        warped[2 * o + 1] = live ? wx : 0.0;
        inframe[o] = (live && wy >= 0.0 && wx >= 0.0 && wy < (double)H && wx < (double)W) ? 1 : 0;
        near_dist[o] = live ? sqrtf(best) : INFINITY;
    }
}

// grid (ceil(cap / 256), pairs): one lane per row of the match list, both directions
__global__ __launch_bounds__(256) void pair_eval_match_dist_kernel(const int* __restrict__ kp, const int* __restrict__ counts,
                                                                   const double* __restrict__ warped, const int* __restrict__ mq,
                                                                   const int* __restrict__ mt, const int* __restrict__ mcount, int pairs, int cap,
                                                                   float* __restrict__ dist) {
    const int p = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= cap) return;
    const int nm = pe_rows(mcount, p, cap), no = pe_rows(counts, p, cap), nt = pe_rows(counts, pairs + p, cap);
    float d_o = INFINITY, d_t = INFINITY;
    if (j < nm) {
        const int q = mq[(size_t)p * cap + j], t = mt[(size_t)p * cap + j];
        if (q >= 0 && q < no && t >= 0 && t < nt) {
            const size_t ro = (size_t)p * cap + q, rt = (size_t)(pairs + p) * cap + t;
            const double oy = (double)kp[2 * ro], ox = (double)kp[2 * ro + 1], ty = (double)kp[2 * rt], tx = (double)kp[2 * rt + 1];
            const float a0 = (float)(warped[2 * ro] - ty), a1 = (float)(warped[2 * ro + 1] - tx);
            const float b0 = (float)(warped[2 * rt] - oy), b1 = (float)(warped[2 * rt + 1] - ox);
            d_o = sqrtf(a0 * a0 + a1 * a1);
            d_t = sqrtf(b0 * b0 + b1 * b1);
        }
    }
    dist[(size_t)p * cap + j] = d_o;
    dist[(size_t)(pairs + p) * cap + j] = d_t;
}

// grid (2*pairs): one block per image = per (direction, pair).  Every count is a sum of wave ballots (integers: the order cannot matter),
// the four waves meet in LDS.
__global__ __launch_bounds__(256) void pair_eval_count_kernel(const float* __restrict__ near_dist, const uint8_t* __restrict__ inframe,
                                                              const int* __restrict__ counts, const float* __restrict__ dist,
                                                              const int* __restrict__ mcount, int pairs, int cap, PeThresholds th, int T,
                                                              int near_inframe_only, int* __restrict__ near_cnt, int* __restrict__ match_cnt,
                                                              int* __restrict__ n_inframe) {
    __shared__ int s_acc[4][2 * PE_MAX_T + 1];
    const int img = blockIdx.x, p = img < pairs ? img : img - pairs, wave = threadIdx.x >> 6;
    const int n = pe_rows(counts, img, cap), nm = dist ? pe_rows(mcount, p, cap) : 0;
    int acc_near[PE_MAX_T], acc_match[PE_MAX_T], acc_in = 0;
#pragma unroll
    for (int k = 0; k < PE_MAX_T; ++k) acc_near[k] = acc_match[k] = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        const bool live = i < n;
        const bool in = live && inframe[(size_t)img * cap + i] != 0;
        const float d = live ? near_dist[(size_t)img * cap + i] : INFINITY;
        const bool use = near_inframe_only ? in : live;
        acc_in += __popcll(__ballot(in));
#pragma unroll
        for (int k = 0; k < PE_MAX_T; ++k)
            if (k < T) acc_near[k] += __popcll(__ballot(use && d <= th.v[k]));
    }
    for (int base = 0; base < nm; base += 256) {
        const int j = base + threadIdx.x;
        const bool live = j < nm;
        const float d = live ? dist[(size_t)img * cap + j] : INFINITY;
#pragma unroll
        for (int k = 0; k < PE_MAX_T; ++k)
            if (k < T) acc_match[k] += __popcll(__ballot(live && d <= th.v[k]));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < PE_MAX_T; ++k) {
            s_acc[wave][k] = acc_near[k];
            s_acc[wave][PE_MAX_T + k] = acc_match[k];
        }
        s_acc[wave][2 * PE_MAX_T] = acc_in;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < 2 * PE_MAX_T + 1) {
        const int v = (s_acc[0][k] + s_acc[1][k]) + (s_acc[2][k] + s_acc[3][k]);
        if (k < PE_MAX_T) {
            if (k < T) near_cnt[(size_t)img * T + k] = v;
        } else if (k < 2 * PE_MAX_T) {
            if (k - PE_MAX_T < T) match_cnt[(size_t)img * T + (k - PE_MAX_T)] = v;
        } else {
            n_inframe[img] = v;
        }
    }
}

// one lane per pair: compute_pts_dist_for_sample's corner error (benchmark_evaluation.py:820-825)
__global__ __launch_bounds__(64) void pair_eval_corner_error_kernel(const double* __restrict__ H_gt, const double* __restrict__ H_est,
                                                                    const int* __restrict__ n_inliers, const int* __restrict__ mcount, int pairs,
                                                                    int H, int W, double* __restrict__ err) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= pairs) return;
    double e = 999.0;
    if (n_inliers[p] != 0 && mcount[p] >= 4) {
        // the reference's own list, as (y, x): [[0, 0], [H, 0], [0, W], [H, H]]
        const double py[4] = {0.0, (double)H, 0.0, (double)H}, px[4] = {0.0, 0.0, (double)W, (double)H};
        double sum = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double gy, gx, ey, ex;
            pe_warp(H_gt + (size_t)p * 9, py[c], px[c], gy, gx);
            pe_warp(H_est + (size_t)p * 9, py[c], px[c], ey, ex);
            const double dy = ey - gy, dx = ex - gx;
            const double nrm = sqrt(dy * dy + dx * dx);
            sum = c == 0 ? nrm : sum + nrm;
        }
        e = sum / 4.0;
    }
    err[p] = e;
}

int pe_check_shape(const char* fn, int pairs, int cap) {
    XP_CHECK_ARG(pairs >= 1 && pairs <= 32767, "%s: pairs must be in [1, 32767] (got %d)", fn, pairs);
    XP_CHECK_ARG(cap >= 1, "%s: cap must be positive (got %d)", fn, cap);
    return XP_OK;
}

}  // namespace

extern "C" int xp_pair_eval_warp_near(const int* kp, const int* counts, int pairs, int cap, int H, int W, const double* map1, const double* map2,
                                      int truncate, double* warped, uint8_t* inframe, float* near_dist, void* stream) {
    const char* fn = "xp_pair_eval_warp_near";
    if (int rc = pe_check_shape(fn, pairs, cap)) return rc;
    XP_CHECK_ARG(H >= 1 && W >= 1, "%s: H and W must be positive (got %d x %d)", fn, H, W);
    XP_CHECK_ARG(kp && counts && map1 && warped && inframe && near_dist, "%s: null pointer", fn);
    XpProfScope prof("pair_eval_warp_near", (hipStream_t)stream, 14.0 * 2 * pairs * (double)cap * cap, 2.0 * pairs * cap * (8.0 + 16.0 + 1.0 + 4.0));
    hipLaunchKernelGGL(pair_eval_warp_near_kernel, dim3(xp_cdiv(cap, 256), 2 * pairs), dim3(256), 0, (hipStream_t)stream, kp, counts, pairs, cap, H, W,
                       map1, map2, truncate, warped, inframe, near_dist);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_pair_eval_match_dist(const int* kp, const int* counts, const double* warped, const int* match_q, const int* match_t,
                                       const int* match_count, int pairs, int cap, float* dist, void* stream) {
    const char* fn = "xp_pair_eval_match_dist";
    if (int rc = pe_check_shape(fn, pairs, cap)) return rc;
    XP_CHECK_ARG(kp && counts && warped && match_q && match_t && match_count && dist, "%s: null pointer", fn);
    XpProfScope prof("pair_eval_match_dist", (hipStream_t)stream, 0.0, (double)pairs * cap * (8.0 + 48.0 + 8.0));
    hipLaunchKernelGGL(pair_eval_match_dist_kernel, dim3(xp_cdiv(cap, 256), pairs), dim3(256), 0, (hipStream_t)stream, kp, counts, warped, match_q,
                       match_t, match_count, pairs, cap, dist);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_pair_eval_count(const float* near_dist, const uint8_t* inframe, const int* counts, const float* dist, const int* match_count,
                                  int pairs, int cap, const float* thresholds_host, int T, int near_inframe_only, int* near_cnt, int* match_cnt,
                                  int* n_inframe, void* stream) {
    const char* fn = "xp_pair_eval_count";
    if (int rc = pe_check_shape(fn, pairs, cap)) return rc;
    XP_CHECK_ARG(T >= 1 && T <= PE_MAX_T, "%s: T must be in [1, %d] (got %d)", fn, PE_MAX_T, T);
    XP_CHECK_ARG(near_dist && inframe && counts && thresholds_host && near_cnt && match_cnt && n_inframe, "%s: null pointer", fn);
    XP_CHECK_ARG(!dist || match_count, "%s: null pointer: match_count", fn);
    PeThresholds th;
    for (int k = 0; k < PE_MAX_T; ++k) th.v[k] = k < T ? thresholds_host[k] : 0.f;
    XpProfScope prof("pair_eval_count", (hipStream_t)stream, 0.0, 2.0 * pairs * cap * (5.0 + (dist ? 4.0 : 0.0)));
    hipLaunchKernelGGL(pair_eval_count_kernel, dim3(2 * pairs), dim3(256), 0, (hipStream_t)stream, near_dist, inframe, counts, dist, match_count, pairs, cap,
                       th, T, near_inframe_only, near_cnt, match_cnt, n_inframe);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_pair_eval_corner_error(const double* H_gt, const double* H_est, const int* n_inliers, const int* match_count, int pairs, int H,
                                         int W, double* err, void* stream) {
    const char* fn = "xp_pair_eval_corner_error";
    if (int rc = pe_check_shape(fn, pairs, 1)) return rc;
    XP_CHECK_ARG(H >= 1 && W >= 1, "%s: H and W must be positive (got %d x %d)", fn, H, W);
    XP_CHECK_ARG(H_gt && H_est && n_inliers && match_count && err, "%s: null pointer", fn);
    XpProfScope prof("pair_eval_corner_error", (hipStream_t)stream, 0.0, (double)pairs * (144.0 + 8.0 + 8.0));
    hipLaunchKernelGGL(pair_eval_corner_error_kernel, dim3(xp_cdiv(pairs, 64)), dim3(64), 0, (hipStream_t)stream, H_gt, H_est, n_inliers, match_count,
                       pairs, H, W, err);
    XP_LAUNCH_CHECK();
    return XP_OK;
}
