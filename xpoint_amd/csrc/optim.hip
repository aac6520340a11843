// The optimiser step of xpoint_amd.training.Adam: the global gradient norm, a small device record that decides whether
// the step is applied, and torch's Adam (L2 weight decay, amsgrad off) over every tensor.  Pure streaming kernels: the apply launch moves
// 7 x 4 bytes per parameter element (p, g, m, v read; p, m, v written), the norm launch 4; HBM bandwidth is the only roof.
//
// Three kinds of launch, no atomics, no host read-back, no allocation:
//   op_sumsq_kernel   one table of (gradient, count) per launch, BY VALUE in the kernel arguments (the launch copies them, so no host buffer has to
//                     outlive the call); workgroup b of the table's tensor j sums g^2 over elements [c SPAN, (c + 1) SPAN) in f64 and writes ONE
//                     partial at the slot its (tensor index, offset) fixes.
//   op_header_kernel  one workgroup adds the partials in a fixed order and writes the XpOptimHeader record.  inf or NaN anywhere in any gradient
//                     makes the sum non-finite: that is the whole detection.
//   op_apply_kernel   the same kind of table (parameter, gradient, offset into the flat moment buffers, count); reads the record and returns at
//                     once when the step is not applied, so parameters and moments stay bit for bit.
// An element's arithmetic does not depend on the tensor's place in a table or on its alignment: a lane owns the four elements 4 (t + 256 k) ..
// + 3 of its workgroup's span either way and moves them with one 16-byte access where the array's address allows, with four 4-byte ones where not.
#include "xp_common.h"
#include "xpoint_hip.h"

#include <math.h>

namespace {

constexpr int OP_THREADS = 256;
constexpr int OP_SPAN = 8192;            // elements of one workgroup: 256 lanes x 4 floats x 8 rounds
constexpr int OP_TABLE = 64;             // tensors per launch: the apply table is 64 x 32 + 65 x 4 bytes of the 4 KB a launch's arguments may hold
constexpr int64_t OP_MAX_PARTIALS = (int64_t)1 << 30;

// the device record, eight 8-byte words (xpoint_amd/training/optim.py reads it as such)
struct XpOptimHeader {
    double norm2;            // sum of g^2 over every gradient of the step
    double bc1, bc2;         // 1 - beta1^t, 1 - beta2^t at the t the apply launch uses
    double clip_coef;        // min(1, max_norm / (sqrt(norm2) + 1e-6)); 1 when clipping is off
    long long t;             // steps applied so far
    long long skipped;       // steps not applied so far
    long long finite;        // norm2 is finite
    long long applied;       // this step is applied: finite, or the guard is off
};
static_assert(sizeof(XpOptimHeader) == 64, "the header record is eight 8-byte words");

struct SumsqTable {
    const float* g[OP_TABLE];
    long long n[OP_TABLE];
    int first[OP_TABLE + 1];          // first[j] = the table's workgroups before tensor j; first[count] = the grid
    int count;
};

struct ApplyEntry {
    float* p;
    const float* g;
    long long moff;
    long long n;
};
struct ApplyTable {
    ApplyEntry e[OP_TABLE];
    int first[OP_TABLE + 1];
    int count;
};

// the tensor a workgroup belongs to: the last j with first[j] <= b (wave-uniform: scalar loads from the kernel arguments)
__device__ __forceinline__ int op_find(const int* first, int count, int b) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// elements i .. i + 3 of a tensor of n (i a multiple of 4, i < n); what lies beyond n reads as 0 and is never written
__device__ __forceinline__ float4 op_ld4(const float* a, long long i, long long n, bool vec) {
    if (vec && i + 4 <= n) return *(const float4*)(a + i);
    float4 r;
    r.x = a[i];
    r.y = i + 1 < n ? a[i + 1] : 0.f;
    r.z = i + 2 < n ? a[i + 2] : 0.f;
    r.w = i + 3 < n ? a[i + 3] : 0.f;
    return r;
}
__device__ __forceinline__ void op_st4(float* a, long long i, long long n, bool vec, float4 r) {
    if (vec && i + 4 <= n) { *(float4*)(a + i) = r; return; }
    a[i] = r.x;
    if (i + 1 < n) a[i + 1] = r.y;
    if (i + 2 < n) a[i + 2] = r.z;
    if (i + 3 < n) a[i + 3] = r.w;
}
__device__ __forceinline__ bool op_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the 256 lanes' values added in a fixed tree; lane 0 gets the sum
__device__ __forceinline__ double op_block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = OP_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(OP_THREADS) void op_sumsq_kernel(const SumsqTable tb, double* partials) {
    __shared__ double sh[OP_THREADS];
    const int b = blockIdx.x;
    const int j = op_find(tb.first, tb.count, b);
    const float* g = tb.g[j];
    const long long n = tb.n[j];
    const long long base = (long long)(b - tb.first[j]) * OP_SPAN;
    const long long end = min(n, base + OP_SPAN);
    const bool vec = op_aligned16(g);
    double acc = 0.0;
    for (long long i = base + 4 * threadIdx.x; i < end; i += 4 * OP_THREADS) {
        const float4 v = op_ld4(g, i, n, vec);
        acc += (double)v.x * (double)v.x;
        acc += (double)v.y * (double)v.y;
        acc += (double)v.z * (double)v.z;
        acc += (double)v.w * (double)v.w;
    }
    const double s = op_block_sum(acc, sh);
    if (threadIdx.x == 0) partials[b] = s;
}

__global__ __launch_bounds__(OP_THREADS) void op_header_kernel(const double* partials, long long n_partials, XpOptimHeader* hdr, double beta1,
                                                               double beta2, double max_norm, int skip_nonfinite) {
    __shared__ double sh[OP_THREADS];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n_partials; i += OP_THREADS) acc += partials[i];
    const double norm2 = op_block_sum(acc, sh);
    if (threadIdx.x != 0) return;
    const bool finite = isfinite(norm2);
    const bool applied = finite || !skip_nonfinite;
    long long t = hdr->t;
    long long skipped = hdr->skipped;
    if (applied) t += 1; else skipped += 1;
    hdr->norm2 = norm2;
    hdr->clip_coef = max_norm > 0.0 ? fmin(1.0, max_norm / (sqrt(norm2) + 1e-6)) : 1.0;
    hdr->bc1 = 1.0 - pow(beta1, (double)t);
    hdr->bc2 = 1.0 - pow(beta2, (double)t);
    hdr->t = t;
    hdr->skipped = skipped;
    hdr->finite = finite ? 1 : 0;
    hdr->applied = applied ? 1 : 0;
}

struct AdamScalars {
    float clip, wd, b1, omb1, b2, omb2, step, bc2s, eps;
};

__device__ __forceinline__ void op_adam1(float& p, float g, float& m, float& v, const AdamScalars& a) {
    const float gg = a.clip * g + a.wd * p;
    m = a.b1 * m + a.omb1 * gg;
    v = a.b2 * v + a.omb2 * (gg * gg);
    const float denom = sqrtf(v) / a.bc2s + a.eps;
    p = p - a.step * (m / denom);
}

__global__ __launch_bounds__(OP_THREADS) void op_apply_kernel(const ApplyTable tb, float* exp_avg, float* exp_avg_sq, const XpOptimHeader* hdr,
                                                              double lr, float wd, float beta1, float omb1, float beta2, float omb2, float eps) {
    if (!hdr->applied) return;          // the guard: nothing is written
    AdamScalars a;
    a.clip = (float)hdr->clip_coef;
    a.wd = wd;
    a.b1 = beta1; a.omb1 = omb1;
    a.b2 = beta2; a.omb2 = omb2;
    a.step = (float)(lr / hdr->bc1);
    a.bc2s = (float)sqrt(hdr->bc2);
    a.eps = eps;
    const int b = blockIdx.x;
    const int j = op_find(tb.first, tb.count, b);
    const ApplyEntry e = tb.e[j];
    float* m = exp_avg + e.moff;
    float* v = exp_avg_sq + e.moff;
    const long long base = (long long)(b - tb.first[j]) * OP_SPAN;
    const long long end = min(e.n, base + OP_SPAN);
    const bool vp = op_aligned16(e.p), vg = op_aligned16(e.g), vm = op_aligned16(m) && op_aligned16(v);
    for (long long i = base + 4 * threadIdx.x; i < end; i += 4 * OP_THREADS) {
        float4 p4 = op_ld4(e.p, i, e.n, vp);
        const float4 g4 = op_ld4(e.g, i, e.n, vg);
        float4 m4 = op_ld4(m, i, e.n, vm);
        float4 v4 = op_ld4(v, i, e.n, vm);
        op_adam1(p4.x, g4.x, m4.x, v4.x, a);
        op_adam1(p4.y, g4.y, m4.y, v4.y, a);
        op_adam1(p4.z, g4.z, m4.z, v4.z, a);
        op_adam1(p4.w, g4.w, m4.w, v4.w, a);
        op_st4(e.p, i, e.n, vp, p4);
        op_st4(m, i, e.n, vm, m4);
        op_st4(v, i, e.n, vm, v4);
    }
}

inline int64_t op_blocks(int64_t n) { return (n + OP_SPAN - 1) / OP_SPAN; }

}  // namespace

extern "C" size_t xp_optim_header_bytes(void) { return sizeof(XpOptimHeader); }

extern "C" size_t xp_optim_workspace_bytes(int n_tensors, int64_t total_elements) {
    if (n_tensors <= 0 || total_elements <= 0) return 0;
    const int64_t partials = total_elements / OP_SPAN + n_tensors;          // >= sum of ceil(n_j / SPAN)
    return (size_t)((partials * 8 + 255) / 256 * 256);
}

extern "C" int xp_optim_grad_sumsq(const float* const* grads, const int64_t* counts, int n_tensors, void* workspace, size_t workspace_bytes,
                                   int64_t* n_partials, void* stream) {
    XP_CHECK_ARG(grads && counts && workspace && n_partials, "xp_optim_grad_sumsq: null pointer");
    XP_CHECK_ARG(n_tensors > 0, "xp_optim_grad_sumsq: bad n_tensors = %d", n_tensors);
    int64_t total = 0;
    for (int j = 0; j < n_tensors; ++j) {
        XP_CHECK_ARG(grads[j] && counts[j] > 0 && ((uintptr_t)grads[j] & 3) == 0, "xp_optim_grad_sumsq: tensor %d: null or misaligned pointer or bad count %lld",
                     j, (long long)counts[j]);
        total += op_blocks(counts[j]);
    }
    XP_CHECK_ARG(total < OP_MAX_PARTIALS && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= (size_t)total * 8,
                 "xp_optim_grad_sumsq: workspace of %lld bytes, 8-byte aligned, needed (got %zu)", (long long)total * 8, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    double* partials = (double*)workspace;
    int64_t done = 0;
    double elems = 0.0;
    for (int j = 0; j < n_tensors; ++j) elems += (double)counts[j];
    XpProfScope prof("optim_grad_sumsq", s, 0.0, 4.0 * elems);
    for (int j0 = 0; j0 < n_tensors;) {
        SumsqTable tb;
        int c = 0;
        int64_t blocks = 0;
        // a table ends at OP_TABLE tensors or before the launch's grid would pass 2^30 workgroups
        while (j0 + c < n_tensors && c < OP_TABLE && (c == 0 || blocks + op_blocks(counts[j0 + c]) < OP_MAX_PARTIALS)) {
            tb.g[c] = grads[j0 + c];
            tb.n[c] = counts[j0 + c];
            tb.first[c] = (int)blocks;
            blocks += op_blocks(counts[j0 + c]);
            ++c;
        }
        for (int k = c; k < OP_TABLE; ++k) { tb.g[k] = nullptr; tb.n[k] = 0; }
        for (int k = c; k <= OP_TABLE; ++k) tb.first[k] = (int)blocks;
        tb.count = c;
        hipLaunchKernelGGL(op_sumsq_kernel, dim3((unsigned)blocks), dim3(OP_THREADS), 0, s, tb, partials + done);
        XP_LAUNCH_CHECK();
        done += blocks;
        j0 += c;
    }
    *n_partials = done;
    return XP_OK;
}

extern "C" int xp_optim_step_header(const void* workspace, int64_t n_partials, void* header, double beta1, double beta2, double max_norm,
                                    int skip_nonfinite, void* stream) {
    XP_CHECK_ARG(workspace && header, "xp_optim_step_header: null pointer");
    XP_CHECK_ARG(n_partials > 0 && n_partials < OP_MAX_PARTIALS, "xp_optim_step_header: bad n_partials = %lld", (long long)n_partials);
    XP_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)header) & 7) == 0, "xp_optim_step_header: workspace and header must be 8-byte aligned");
    XP_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "xp_optim_step_header: betas must lie in [0, 1) (got %g, %g)", beta1, beta2);
    hipStream_t s = (hipStream_t)stream;
    XpProfScope prof("optim_step_header", s, 0.0, 8.0 * n_partials);
    hipLaunchKernelGGL(op_header_kernel, dim3(1), dim3(OP_THREADS), 0, s, (const double*)workspace, (long long)n_partials, (XpOptimHeader*)header, beta1,
                       beta2, max_norm, skip_nonfinite);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_optim_adam_apply(float* const* params, const float* const* grads, const int64_t* moment_offsets, const int64_t* counts, int n_tensors,
                                   float* exp_avg, float* exp_avg_sq, int64_t moment_elements, const void* header, double lr, double weight_decay,
                                   double beta1, double beta2, double eps, void* stream) {
    XP_CHECK_ARG(params && grads && moment_offsets && counts && exp_avg && exp_avg_sq && header, "xp_optim_adam_apply: null pointer");
    XP_CHECK_ARG(n_tensors > 0 && moment_elements > 0, "xp_optim_adam_apply: bad n_tensors = %d or moment_elements = %lld", n_tensors,
                 (long long)moment_elements);
    XP_CHECK_ARG((((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0 && ((uintptr_t)header & 7) == 0,
                 "xp_optim_adam_apply: the moment buffers must be 16-byte aligned, the header 8-byte");
    for (int j = 0; j < n_tensors; ++j) {
        XP_CHECK_ARG(params[j] && grads[j] && counts[j] > 0 && (((uintptr_t)params[j] | (uintptr_t)grads[j]) & 3) == 0,
                     "xp_optim_adam_apply: tensor %d: null or misaligned pointer or bad count %lld", j, (long long)counts[j]);
        XP_CHECK_ARG(moment_offsets[j] >= 0 && moment_offsets[j] <= moment_elements - counts[j],
                     "xp_optim_adam_apply: tensor %d: moments [%lld, +%lld) leave the buffers of %lld elements", j, (long long)moment_offsets[j],
                     (long long)counts[j], (long long)moment_elements);
    }
    hipStream_t s = (hipStream_t)stream;
    double elems = 0.0;
    for (int j = 0; j < n_tensors; ++j) elems += (double)counts[j];
    XpProfScope prof("optim_adam_apply", s, 0.0, 28.0 * elems);
    for (int j0 = 0; j0 < n_tensors;) {
        ApplyTable tb;
        int c = 0;
        int64_t blocks = 0;
        while (j0 + c < n_tensors && c < OP_TABLE && (c == 0 || blocks + op_blocks(counts[j0 + c]) < OP_MAX_PARTIALS)) {
            tb.e[c] = ApplyEntry{params[j0 + c], grads[j0 + c], (long long)moment_offsets[j0 + c], (long long)counts[j0 + c]};
            tb.first[c] = (int)blocks;
            blocks += op_blocks(counts[j0 + c]);
            ++c;
        }
        for (int k = c; k < OP_TABLE; ++k) tb.e[k] = ApplyEntry{nullptr, nullptr, 0, 0};
        for (int k = c; k <= OP_TABLE; ++k) tb.first[k] = (int)blocks;
        tb.count = c;
        XP_CHECK_ARG(blocks < OP_MAX_PARTIALS, "xp_optim_adam_apply: tensor %d of %lld elements is beyond one launch's grid", j0, (long long)counts[j0]);
        hipLaunchKernelGGL(op_apply_kernel, dim3((unsigned)blocks), dim3(OP_THREADS), 0, s, tb, exp_avg, exp_avg_sq, (const XpOptimHeader*)header, lr,
                           (float)weight_decay, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);          // 1 - beta in f64 first: 1.f - 0.999f is off by 1e-5
        XP_LAUNCH_CHECK();
        j0 += c;
    }
    return XP_OK;
}
