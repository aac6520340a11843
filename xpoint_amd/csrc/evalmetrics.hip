// Evaluation-harness helper: distance from every point of one set to the nearest point of
// another set.  Reference call sites: xpoint/utils/benchmark_evaluation.py:441-450 (repeatability: np.linalg.norm of
// all-pairs differences, then min over one axis) and :652-659 (correct-match matrix torch.norm(dist.float(), dim=-1) <= th,
// reduced with .sum(1).nonzero()): both only need min_j |a_i - b_j|, so the N x M matrix is never materialised.
//
// HBM-bound on paper (8-byte points), in practice a tiny compute kernel: one thread per point of `a`, `b` staged through
// LDS in tiles of 512 float points.  The walk over a staged tile and its arithmetic (the reference's dist.float()) are
// xp_near_walk (near_walk.h), shared with pair_eval_warp_near_kernel; sqrt is monotonic, so the minimum of the norms is the
// norm at the minimum squared distance.
#include "xp_common.h"
#include "near_walk.h"

namespace {

__global__ __launch_bounds__(256) void points_min_dist_kernel(const double* __restrict__ a, int na, const float* __restrict__ b, int nb,
                                                              float* __restrict__ out) {
    __shared__ float s_b[512][2];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double a0 = i < na ? a[2 * i] : 0.0, a1 = i < na ? a[2 * i + 1] : 0.0;
    float best = INFINITY;
    for (int j0 = 0; j0 < nb; j0 += 512) {
        const int n = min(512, nb - j0);
        __syncthreads();
        for (int t = threadIdx.x; t < 2 * n; t += 256) s_b[t >> 1][t & 1] = b[2 * j0 + t];
        __syncthreads();
        best = xp_near_walk(a0, a1, s_b, n, best);
    }
    if (i < na) out[i] = sqrtf(best);
}


// ---------------------------------------------------------------------------------------------------------------------
// Detector evaluation (reference xpoint/utils/evaluation.py:57-97, compute_tp_fp_dist) without the P x K distance matrix and
// without the sequential loop over predictions.  The reference walks the predictions by descending probability; each one claims
// the FIRST (row-major) label within the radius and is a true positive iff that label was still free.  So prediction i is a true
// positive exactly when it is the best-ranked prediction among those whose first label is g(i): one window scan of the label map
// per candidate pixel and one 64-bit atomic minimum per label.
//
// Rank key of a candidate pixel (prob > zero_threshold, hence prob > 0 and its float bits are monotone in its value):
//   high word = ~float bits (a larger probability gives a smaller key), low word = row-major pixel index (ties: the lower index ranks
//   first — this project's rule; the reference leaves the order of equal probabilities to torch.sort).
// The key exists in registers only: the claim forms it for the atomic minimum, the resolve pass forms it again to compare.  The rank
// ORDER over a whole image is the same relation realised by a stable descending sort of the candidate probabilities (cand_prob: the
// probability of a candidate, 0 elsewhere, so that non-candidates sort last): a 4-byte sort key instead of an 8-byte one.
constexpr unsigned int XP_EVAL_NO_LABEL = ~0u;

// Labels within the radius of pixel (y, x), visited in row-major order (the order of torch.nonzero of the label map): f(label pixel
// index, distance).  The distance is sqrtf of an exact small integer in f32, as torch.norm of the integer difference cast to float.
__device__ __forceinline__ unsigned long long eval_rank_key(float v, size_t p) {
    return ((unsigned long long)(~__float_as_uint(v)) << 32) | (unsigned long long)(unsigned int)p;
}

template <typename F>
__device__ __forceinline__ void eval_scan_window(const uint8_t* __restrict__ lab, int H, int W, int y, int x, int r, float thresh, F f) {
    const int y0 = max(y - r, 0), y1 = min(y + r, H - 1), x0 = max(x - r, 0), x1 = min(x + r, W - 1);
    for (int yy = y0; yy <= y1; ++yy) {
        const int dy = yy - y;
        for (int xx = x0; xx <= x1; ++xx) {
            if (!lab[(size_t)yy * W + xx]) continue;
            const int dx = xx - x;
            const float d = sqrtf((float)(dy * dy + dx * dx));
            if (d <= thresh) f((unsigned int)yy * (unsigned int)W + (unsigned int)xx, d);
        }
    }
}

// grid (ceil(HW / 256), batch): one thread per pixel; a block never spans two images.
__global__ __launch_bounds__(256) void eval_claim_kernel(const float* __restrict__ prob, const uint8_t* __restrict__ labels, int H, int W,
                                                         float zero_threshold, float thresh, int r, float* __restrict__ cand_prob,
                                                         unsigned long long* __restrict__ winner, unsigned int* __restrict__ first_label,
                                                         int* __restrict__ n_within, int* __restrict__ n_cand, int* __restrict__ n_gt) {
    const size_t HW = (size_t)H * W, p = (size_t)blockIdx.x * 256 + threadIdx.x, base = (size_t)blockIdx.y * HW;
    const bool in = p < HW;
    const float v = in ? prob[base + p] : 0.f;
    const bool cand = in && v > zero_threshold;
    const bool is_label = in && labels[base + p] != 0;
    unsigned int g = XP_EVAL_NO_LABEL;
    int cnt = 0;
    if (cand) {
        const unsigned long long key = eval_rank_key(v, p);
        eval_scan_window(labels + base, H, W, (int)(p / W), (int)(p % W), r, thresh, [&](unsigned int q, float) {
            if (cnt == 0) g = q;
            ++cnt;
        });
        if (g != XP_EVAL_NO_LABEL) atomicMin(&winner[base + g], key);
    }
    if (in) {
        cand_prob[base + p] = cand ? v : 0.f;
        first_label[base + p] = g;
        n_within[base + p] = cnt;
    }
    const unsigned long long mc = __ballot(cand), ml = __ballot(is_label);
    if ((threadIdx.x & 63) == 0) {
        if (mc) atomicAdd(&n_cand[blockIdx.y], __popcll(mc));
        if (ml) atomicAdd(&n_gt[blockIdx.y], __popcll(ml));
    }
}

__global__ __launch_bounds__(256) void eval_resolve_kernel(const float* __restrict__ cand_prob, const unsigned long long* __restrict__ winner,
                                                           const unsigned int* __restrict__ first_label, size_t HW, uint8_t* __restrict__ tp_pix) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x, base = (size_t)blockIdx.y * HW;
    if (p >= HW) return;
    const unsigned int g = first_label[base + p];
    const float v = cand_prob[base + p];          // > 0 exactly at the candidates
    tp_pix[base + p] = (v > 0.f && g != XP_EVAL_NO_LABEL && winner[base + g] == eval_rank_key(v, p)) ? 1 : 0;
}

// one thread per rank (rank_pix: the pixel of every rank, from the sort): the candidate's true-positive flag and its pair count
__global__ __launch_bounds__(256) void eval_gather_kernel(const long long* __restrict__ rank_pix, const uint8_t* __restrict__ tp_pix,
                                                          const int* __restrict__ n_within, const int* __restrict__ n_cand, size_t HW,
                                                          uint8_t* __restrict__ tp_sorted, int* __restrict__ cnt_sorted) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, base = (size_t)blockIdx.y * HW;
    if (i >= HW) return;
    const long long p = rank_pix[base + i];
    const bool ok = i < (size_t)n_cand[blockIdx.y] && p >= 0 && (size_t)p < HW;
    tp_sorted[base + i] = ok ? tp_pix[base + p] : 0;
    cnt_sorted[base + i] = ok ? n_within[base + p] : 0;
}

// one thread per rank: the distances of its within-radius labels, at the offset the scan over ranks gives
__global__ __launch_bounds__(256) void eval_fill_dist_kernel(const long long* __restrict__ rank_pix, const uint8_t* __restrict__ labels,
                                                             const long long* __restrict__ incl, const int* __restrict__ cnt_sorted, int H, int W,
                                                             float thresh, int r, float* __restrict__ dist, long long dist_len) {
    const size_t HW = (size_t)H * W, i = (size_t)blockIdx.x * 256 + threadIdx.x, base = (size_t)blockIdx.y * HW;
    if (i >= HW) return;
    const int c = cnt_sorted[base + i];
    const long long p = rank_pix[base + i];
    if (c <= 0 || p < 0 || (size_t)p >= HW) return;
    long long off = incl[base + i] - c;
    const long long end = off + c;
    if (off < 0 || end > dist_len) return;
    eval_scan_window(labels + base, H, W, (int)(p / W), (int)(p % W), r, thresh, [&](unsigned int, float d) {
        if (off < end) dist[off++] = d;
    });
}

int eval_check_shape(const char* fn, int batch, int H, int W) {
    XP_CHECK_ARG(batch >= 1 && batch <= 65535, "%s: batch must be in [1, 65535] (got %d)", fn, batch);
    XP_CHECK_ARG(H >= 1 && W >= 1, "%s: H and W must be positive (got %d x %d)", fn, H, W);
    XP_CHECK_ARG((long long)H * W <= 0xFFFFFFFFll, "%s: H * W = %lld does not fit the 32-bit pixel index of the rank key", fn, (long long)H * W);
    return XP_OK;
}

int eval_check_thresh(const char* fn, float distance_thresh) {
    XP_CHECK_ARG(distance_thresh >= 0.f && distance_thresh <= 8.f, "%s: distance_thresh must be in [0, 8] (got %g)", fn, (double)distance_thresh);
    return XP_OK;
}

}  // namespace

extern "C" int xp_points_min_dist(const double* a, int na, const float* b, int nb, float* out, void* stream) {
    XP_CHECK_ARG(na >= 0 && nb >= 0, "xp_points_min_dist: negative count");
    if (na == 0) return XP_OK;
    XP_CHECK_ARG(a && out && (b || nb == 0), "xp_points_min_dist: null pointer");
    XpProfScope prof("points_min_dist", (hipStream_t)stream, 5.0 * na * (double)nb, 16.0 * na + 8.0 * nb);
    hipLaunchKernelGGL(points_min_dist_kernel, dim3(xp_cdiv(na, 256)), dim3(256), 0, (hipStream_t)stream, a, na, b, nb, out);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_detector_eval_claim(const float* prob, const uint8_t* labels, int batch, int H, int W, float zero_threshold, float distance_thresh,
                                      float* cand_prob, unsigned long long* winner, unsigned int* first_label, int* n_within,
                                      int* n_cand, int* n_gt, void* stream) {
    const char* fn = "xp_detector_eval_claim";
    if (int rc = eval_check_shape(fn, batch, H, W)) return rc;
    if (int rc = eval_check_thresh(fn, distance_thresh)) return rc;
    XP_CHECK_ARG(zero_threshold >= 0.f, "%s: zero_threshold must be >= 0 (got %g): the rank key needs positive probabilities", fn, (double)zero_threshold);
    XP_CHECK_ARG(prob, "%s: null pointer: prob", fn);
    XP_CHECK_ARG(labels, "%s: null pointer: labels", fn);
    XP_CHECK_ARG(cand_prob, "%s: null pointer: cand_prob", fn);
    XP_CHECK_ARG(winner, "%s: null pointer: winner", fn);
    XP_CHECK_ARG(first_label, "%s: null pointer: first_label", fn);
    XP_CHECK_ARG(n_within, "%s: null pointer: n_within", fn);
    XP_CHECK_ARG(n_cand, "%s: null pointer: n_cand", fn);
    XP_CHECK_ARG(n_gt, "%s: null pointer: n_gt", fn);
    const size_t HW = (size_t)H * W;
    const int r = (int)floorf(distance_thresh);
    hipStream_t st = (hipStream_t)stream;
    XP_HIP(hipMemsetAsync(winner, 0xFF, (size_t)batch * HW * sizeof(unsigned long long), st));
    XP_HIP(hipMemsetAsync(n_cand, 0, (size_t)batch * sizeof(int), st));
    XP_HIP(hipMemsetAsync(n_gt, 0, (size_t)batch * sizeof(int), st));
    XpProfScope prof("detector_eval_claim", st, 0.0, (double)batch * HW * (4.0 + (2 * r + 1) * (2 * r + 1) + 20.0));
    hipLaunchKernelGGL(eval_claim_kernel, dim3(xp_cdiv((int64_t)HW, 256), batch), dim3(256), 0, st, prob, labels, H, W, zero_threshold,
                       distance_thresh, r, cand_prob, winner, first_label, n_within, n_cand, n_gt);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_detector_eval_resolve(const float* cand_prob, const unsigned long long* winner, const unsigned int* first_label, int batch,
                                        int H, int W, uint8_t* tp_pix, void* stream) {
    const char* fn = "xp_detector_eval_resolve";
    if (int rc = eval_check_shape(fn, batch, H, W)) return rc;
    XP_CHECK_ARG(cand_prob, "%s: null pointer: cand_prob", fn);
    XP_CHECK_ARG(winner, "%s: null pointer: winner", fn);
    XP_CHECK_ARG(first_label, "%s: null pointer: first_label", fn);
    XP_CHECK_ARG(tp_pix, "%s: null pointer: tp_pix", fn);
    const size_t HW = (size_t)H * W;
    XpProfScope prof("detector_eval_resolve", (hipStream_t)stream, 0.0, (double)batch * HW * 17.0);
    hipLaunchKernelGGL(eval_resolve_kernel, dim3(xp_cdiv((int64_t)HW, 256), batch), dim3(256), 0, (hipStream_t)stream, cand_prob, winner, first_label, HW,
                       tp_pix);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_detector_eval_gather(const long long* rank_pix, const uint8_t* tp_pix, const int* n_within, const int* n_cand, int batch, int H,
                                       int W, uint8_t* tp_sorted, int* cnt_sorted, void* stream) {
    const char* fn = "xp_detector_eval_gather";
    if (int rc = eval_check_shape(fn, batch, H, W)) return rc;
    XP_CHECK_ARG(rank_pix, "%s: null pointer: rank_pix", fn);
    XP_CHECK_ARG(tp_pix, "%s: null pointer: tp_pix", fn);
    XP_CHECK_ARG(n_within, "%s: null pointer: n_within", fn);
    XP_CHECK_ARG(n_cand, "%s: null pointer: n_cand", fn);
    XP_CHECK_ARG(tp_sorted, "%s: null pointer: tp_sorted", fn);
    XP_CHECK_ARG(cnt_sorted, "%s: null pointer: cnt_sorted", fn);
    const size_t HW = (size_t)H * W;
    XpProfScope prof("detector_eval_gather", (hipStream_t)stream, 0.0, (double)batch * HW * 18.0);
    hipLaunchKernelGGL(eval_gather_kernel, dim3(xp_cdiv((int64_t)HW, 256), batch), dim3(256), 0, (hipStream_t)stream, rank_pix, tp_pix, n_within,
                       n_cand, HW, tp_sorted, cnt_sorted);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_detector_eval_fill_dist(const long long* rank_pix, const uint8_t* labels, const long long* incl, const int* cnt_sorted,
                                          int batch, int H, int W, float distance_thresh, float* dist, long long dist_len, void* stream) {
    const char* fn = "xp_detector_eval_fill_dist";
    if (int rc = eval_check_shape(fn, batch, H, W)) return rc;
    if (int rc = eval_check_thresh(fn, distance_thresh)) return rc;
    XP_CHECK_ARG(dist_len >= 0, "%s: dist_len must be >= 0 (got %lld)", fn, dist_len);
    if (dist_len == 0) return XP_OK;
    XP_CHECK_ARG(rank_pix, "%s: null pointer: rank_pix", fn);
    XP_CHECK_ARG(labels, "%s: null pointer: labels", fn);
    XP_CHECK_ARG(incl, "%s: null pointer: incl", fn);
    XP_CHECK_ARG(cnt_sorted, "%s: null pointer: cnt_sorted", fn);
    XP_CHECK_ARG(dist, "%s: null pointer: dist", fn);
    const size_t HW = (size_t)H * W;
    const int r = (int)floorf(distance_thresh);
    XpProfScope prof("detector_eval_fill_dist", (hipStream_t)stream, 0.0, (double)batch * HW * 20.0 + 4.0 * (double)dist_len);
    hipLaunchKernelGGL(eval_fill_dist_kernel, dim3(xp_cdiv((int64_t)HW, 256), batch), dim3(256), 0, (hipStream_t)stream, rank_pix, labels, incl,
                       cnt_sorted, H, W, distance_thresh, r, dist, dist_len);
    XP_LAUNCH_CHECK();
    return XP_OK;
}
