// Detector loss of XPoint training (reference xpoint/utils/losses.py:374-576, 'hard_assignment'), forward and backward.
// One thread per 8x8 cell: the label encoding (space_to_depth channel c = 8 dy + dx of the keypoint map, argmax over
// [3 label + noise, 2.0] with the first maximum winning), the block-product valid mask, the log-softmax over the 65 logits
// (NCHW: a cell's channels are HW apart, so a wave reads 64 consecutive cells per channel), the per-cell loss
//     kind 0: cross entropy with class weights [1] * 64 + [dustbin_weight];   kind 1: focal alpha (1 - pt)^gamma ce
// and the statistics code of the cell.  The statistics compare argmax(softmax(logits)) with label * valid, the loss uses the
// unmasked label and is multiplied by valid afterwards (losses.py:492, 564).  A second kernel sums every per-sample quantity in a
// fixed order (f64), so the result is bit-reproducible and independent of the other samples.
#include "xp_common.h"
#include "xpoint_hip.h"

namespace {

struct DetCell {
    float lse;       // log sum exp
    int pred;        // argmax of the softmax probabilities, first maximum
};

// softmax statistics of one cell; p[c] = exp(x_c - max) / sum as torch.softmax forms it (the statistics take their argmax)
__device__ __forceinline__ DetCell det_softmax(const float* __restrict__ x, size_t HW, float& sum, float& mx) {
    mx = x[0];
    for (int c = 1; c < 65; ++c) mx = fmaxf(mx, x[c * HW]);
    sum = 0.f;
    for (int c = 0; c < 65; ++c) sum += expf(x[c * HW] - mx);
    DetCell r;
    r.lse = mx + logf(sum);
    float best = -1.f;
    r.pred = 0;
    for (int c = 0; c < 65; ++c) {
        const float pc = expf(x[c * HW] - mx) / sum;
        if (pc > best) { best = pc; r.pred = c; }
    }
    return r;
}

__global__ __launch_bounds__(256) void det_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ kp, const float* __restrict__ mask,
                                                      const float* __restrict__ noise, int Hc, int Wc, int kind, float wdust, float alpha, float gamma,
                                                      int* __restrict__ labels, float* __restrict__ valid, float* __restrict__ cell_loss,
                                                      int* __restrict__ cell_code) {
    const int HW = Hc * Wc, b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= HW) return;
    const int cy = n / Wc, cx = n % Wc, W = Wc * 8;
    const float* kb = kp + ((size_t)b * Hc * 8 + cy * 8) * W + cx * 8;
    const float* mb = mask ? mask + ((size_t)b * Hc * 8 + cy * 8) * W + cx * 8 : nullptr;
    const float* nb = noise + (size_t)b * 64 * HW + n;
    float best = -INFINITY, v = 1.f;
    int label = 0;
    for (int c = 0; c < 64; ++c) {
        const float s = 3.0f * kb[(c >> 3) * W + (c & 7)] + nb[(size_t)c * HW];
        if (c == 0 || s > best) { best = s; label = c; }
        if (mb) v *= mb[(c >> 3) * W + (c & 7)];
    }
    if (2.0f > best) label = 64;
    const float* x = logits + (size_t)b * 65 * HW + n;
    float sum, mx;
    const DetCell sc = det_softmax(x, HW, sum, mx);
    const float ce = sc.lse - x[(size_t)label * HW];
    float loss;
    if (kind == 0) {
        loss = (label == 64 ? wdust : 1.f) * ce;
    } else {
        const float pt = expf(-ce);
        loss = alpha * powf(1.f - pt, gamma) * ce;
    }
    const float lm = (float)label * v;          // labels_hard_assigned * valid_mask
    const float pr = (float)sc.pred;
    const bool ppos = sc.pred <= 63, lpos = lm <= 63.f, pneg = sc.pred == 64, lneg = lm == 64.f;
    labels[(size_t)b * HW + n] = label;
    valid[(size_t)b * HW + n] = v;
    cell_loss[(size_t)b * HW + n] = loss * v;
    cell_code[(size_t)b * HW + n] = (pr == lm ? 1 : 0) | (ppos && lpos ? 2 : 0) | (ppos && lneg ? 4 : 0) | (pneg && lpos ? 8 : 0) | (pneg && lneg ? 16 : 0);
}

// stats (B, 8) f64: sum loss * valid, sum valid, correct, TP, FP, FN, TN, 0
__global__ __launch_bounds__(256) void det_reduce_kernel(const float* __restrict__ cell_loss, const float* __restrict__ valid, const int* __restrict__ code,
                                                         int HW, double* __restrict__ stats) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ double sm[7][256];
    double a[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int n = tid; n < HW; n += 256) {
        const size_t i = (size_t)b * HW + n;
        const int c = code[i];
        a[0] += (double)cell_loss[i];
        a[1] += (double)valid[i];
        for (int k = 0; k < 5; ++k) a[2 + k] += (double)((c >> k) & 1);
    }
    for (int k = 0; k < 7; ++k) sm[k][tid] = a[k];
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (tid < m)
            for (int k = 0; k < 7; ++k) sm[k][tid] += sm[k][tid + m];
        __syncthreads();
    }
    if (tid < 8) stats[b * 8 + tid] = tid < 7 ? sm[tid][0] : 0.0;
}

// dlogits[b][c][n] = coef_b valid_n dloss_n / dx_c
__global__ __launch_bounds__(256) void det_bwd_kernel(const float* __restrict__ logits, const int* __restrict__ labels, const float* __restrict__ valid,
                                                      const float* __restrict__ coef, int HW, int kind, float wdust, float alpha, float gamma,
                                                      float* __restrict__ dlogits) {
    const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= HW) return;
    const float* x = logits + (size_t)b * 65 * HW + n;
    float* dx = dlogits + (size_t)b * 65 * HW + n;
    const int label = labels[(size_t)b * HW + n];
    float sum, mx;
    const DetCell sc = det_softmax(x, HW, sum, mx);
    const float ce = sc.lse - x[(size_t)label * HW];
    float dce;                                  // d loss / d ce
    if (kind == 0) {
        dce = label == 64 ? wdust : 1.f;
    } else {
        const float pt = expf(-ce), q = 1.f - pt;
        // d/dce [ alpha q^gamma ce ] with q = 1 - exp(-ce): alpha (gamma q^(gamma - 1) pt ce + q^gamma)
        const float t = q > 0.f ? gamma * powf(q, gamma - 1.f) * pt * ce : 0.f;
        dce = alpha * (t + powf(q, gamma));
    }
    const float g = coef[b] * valid[(size_t)b * HW + n] * dce;
    for (int c = 0; c < 65; ++c) {
        const float pc = expf(x[(size_t)c * HW] - sc.lse);
        dx[(size_t)c * HW] = g * (pc - (c == label ? 1.f : 0.f));
    }
}

static int det_check(const char* who, int B, int Hc, int Wc, int kind) {
    XP_CHECK_ARG(B > 0 && Hc > 0 && Wc > 0 && (int64_t)Hc * Wc <= (1 << 24), "%s: bad shape B=%d Hc=%d Wc=%d", who, B, Hc, Wc);
    XP_CHECK_ARG(kind == 0 || kind == 1, "%s: kind must be 0 (cross_entropy) or 1 (focal_loss), got %d", who, kind);
    return XP_OK;
}

}  // namespace

extern "C" int xp_detector_loss_fwd(const float* logits, const float* keypoint_map, const float* valid_mask, const float* noise, int B, int Hc, int Wc,
                                    int kind, float dustbin_weight, float alpha, float gamma, int* labels, float* valid, float* cell_loss, int* cell_code,
                                    double* stats, void* stream) {
    if (int rc = det_check("xp_detector_loss_fwd", B, Hc, Wc, kind)) return rc;
    XP_CHECK_ARG(logits && keypoint_map && noise && labels && valid && cell_loss && cell_code && stats, "xp_detector_loss_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int HW = Hc * Wc;
    XpProfScope prof("detector_loss_fwd", s, 0.0, (double)B * HW * (65 + 64 * 3) * 4);
    hipLaunchKernelGGL(det_fwd_kernel, dim3(xp_cdiv(HW, 256), B), dim3(256), 0, s, logits, keypoint_map, valid_mask, noise, Hc, Wc, kind, dustbin_weight,
                       alpha, gamma, labels, valid, cell_loss, cell_code);
    XP_LAUNCH_CHECK();
    hipLaunchKernelGGL(det_reduce_kernel, dim3(B), dim3(256), 0, s, cell_loss, valid, cell_code, HW, stats);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_detector_loss_bwd(const float* logits, const int* labels, const float* valid, const float* coef, int B, int Hc, int Wc, int kind,
                                    float dustbin_weight, float alpha, float gamma, float* dlogits, void* stream) {
    if (int rc = det_check("xp_detector_loss_bwd", B, Hc, Wc, kind)) return rc;
    XP_CHECK_ARG(logits && labels && valid && coef && dlogits, "xp_detector_loss_bwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int HW = Hc * Wc;
    XpProfScope prof("detector_loss_bwd", s, 0.0, (double)B * HW * 65 * 2 * 4);
    hipLaunchKernelGGL(det_bwd_kernel, dim3(xp_cdiv(HW, 256), B), dim3(256), 0, s, logits, labels, valid, coef, HW, kind, dustbin_weight, alpha, gamma,
                       dlogits);
    XP_LAUNCH_CHECK();
    return XP_OK;
}
