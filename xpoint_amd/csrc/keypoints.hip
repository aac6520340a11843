// Keypoints from the heat map and their descriptors.
//   extract_keypoints  reference predict_align_image_pair.py:242-243, predict_keypoints.py:213-215
//   sample_descriptors reference xpoint/utils/utils.py:229-238  (F.grid_sample bilinear, align_corners)
#include "xp_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Keypoint extraction: row-major (y, x) list of pixels with prob > thr (and mask != 0), per image — the order of
// torch.nonzero, which defines the match index space.  Ordered compaction in three stream-ordered launches:
// per-segment counts (V * 1024 pixels per workgroup), exclusive scan of the segment counts per image, ordered write.
// V pixels per thread: 1, or 4 (one 16-byte load; H * W % 4 == 0, 16-byte aligned maps).  Same lists, same order: the rank of
// pixel j of lane l inside its wave = hits of the lanes before l (V ballots) + hits of l's own earlier pixels.
// ---------------------------------------------------------------------------------------------
constexpr int KP_SEG = 1024;

// bit j: pixel i + j is a keypoint
template <int V>
__device__ __forceinline__ unsigned kp_hit(const float* __restrict__ pb, const uint8_t* __restrict__ mb, int64_t i, int64_t HW, float thr) {
    static_assert(V == 1 || V == 4, "one pixel or one 16-byte load per thread");
    if constexpr (V == 1) {
        return (i < HW && pb[i] > thr && (!mb || mb[i])) ? 1u : 0u;
    } else {
        if (i >= HW) return 0u;
        const float4 v = *reinterpret_cast<const float4*>(pb + i);
        unsigned h = (v.x > thr ? 1u : 0u) | (v.y > thr ? 2u : 0u) | (v.z > thr ? 4u : 0u) | (v.w > thr ? 8u : 0u);
        if (mb) {
            const unsigned m = *reinterpret_cast<const unsigned*>(mb + i);
            h &= ((m & 0xffu) ? 1u : 0u) | ((m & 0xff00u) ? 2u : 0u) | ((m & 0xff0000u) ? 4u : 0u) | ((m & 0xff000000u) ? 8u : 0u);
        }
        return h;
    }
}

template <int V>
__global__ __launch_bounds__(KP_SEG) void kp_count_kernel(const float* __restrict__ prob, const uint8_t* __restrict__ mask, float thr,
                                                           int* __restrict__ seg_counts, int64_t HW, int nseg) {
    __shared__ int s_wave[KP_SEG / 64];
    const int b = blockIdx.y, seg = blockIdx.x;
    const int64_t i = ((int64_t)seg * KP_SEG + threadIdx.x) * V;
    const unsigned h = kp_hit<V>(prob + b * HW, mask ? mask + b * HW : nullptr, i, HW, thr);
    int c = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) c += __popcll(__ballot(h & (1u << j)));
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < KP_SEG / 64; ++w) t += s_wave[w]; seg_counts[b * nseg + seg] = t; }
}

// one workgroup per image: exclusive scan of the segment counts in place; total -> counts[b]
__global__ __launch_bounds__(1024) void kp_scan_kernel(int* __restrict__ seg_counts, int* __restrict__ counts, int nseg) {
    __shared__ int s_part[1024];
    const int b = blockIdx.x;
    int* sc = seg_counts + b * nseg;
    const int per = (nseg + 1023) / 1024;
    const int j0 = threadIdx.x * per, j1 = min(nseg, j0 + per);
    int t = 0;
    for (int j = j0; j < j1; ++j) t += sc[j];
    s_part[threadIdx.x] = t;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {          // Hillis-Steele inclusive scan over the 1024 partials
        const int v = threadIdx.x >= o ? s_part[threadIdx.x - o] : 0;
        __syncthreads();
        s_part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = threadIdx.x ? s_part[threadIdx.x - 1] : 0;
    for (int j = j0; j < j1; ++j) { const int c = sc[j]; sc[j] = run; run += c; }
    if (threadIdx.x == 1023) counts[b] = s_part[1023];   // may exceed cap: the caller checks
}

template <int V>
__global__ __launch_bounds__(KP_SEG) void kp_write_kernel(const float* __restrict__ prob, const uint8_t* __restrict__ mask, float thr,
                                                           const int* __restrict__ seg_offsets, int* __restrict__ kp, int64_t HW, int W,
                                                           int nseg, int cap) {
    __shared__ int s_wave[KP_SEG / 64];
    const int b = blockIdx.y, seg = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = ((int64_t)seg * KP_SEG + threadIdx.x) * V;
    const unsigned h = kp_hit<V>(prob + b * HW, mask ? mask + b * HW : nullptr, i, HW, thr);
    const unsigned long long before = (1ull << lane) - 1ull;
    unsigned long long bal[V];
    int total = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) { bal[j] = __ballot(h & (1u << j)); total += __popcll(bal[j]); }
    if (lane == 0) s_wave[wave] = total;
    __syncthreads();
    if (!h) return;
    int pos = seg_offsets[b * nseg + seg];
#pragma unroll
    for (int j = 0; j < V; ++j) pos += __popcll(bal[j] & before);
    for (int w = 0; w < wave; ++w) pos += s_wave[w];
#pragma unroll
    for (int j = 0; j < V; ++j)
        if ((h >> j) & 1u) {
            if (pos < cap) { int* kb = kp + ((int64_t)b * cap + pos) * 2; kb[0] = (int)((i + j) / W); kb[1] = (int)((i + j) % W); }
            ++pos;
        }
}

// ---------------------------------------------------------------------------------------------
// Descriptor sampling at keypoints: bilinear grid_sample (zeros padding, align_corners=True) of the
// NHWC descriptor volume followed by L2 normalisation, in ATen's fp32 operation order so the result
// matches torch to rounding:  g = k / (S*0.5) - 1;  i = (g + 1) * ((Sc - 1) / 2);  weights
// nw=(ixe-ix)(iye-iy), ne=(ix-ixw)(iye-iy), sw=(ixe-ix)(iy-iyn), se=(ix-ixw)(iy-iyn); sum nw,ne,sw,se.
// One wave per keypoint, lanes over the descriptor dimension.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_descriptors_kernel(const int* __restrict__ kp, const int* __restrict__ counts,
                                                                 const float* __restrict__ desc, float* __restrict__ out, int cap,
                                                                 int Hc, int Wc, int D, int H, int W) {
    const int b = blockIdx.y;
    const int n = min(counts[b], cap);
    // XCD-aware block order: consecutive workgroup ids go round-robin to the 8 XCDs, each with its own L2.  Keypoints arrive in raster
    // order and neighbours share descriptor rows (4 cells per keypoint, ~8 keypoints per cell row and column), so every XCD gets ONE
    // contiguous run of the image's keypoints (sized from the actual count, not the capacity) instead of every eighth group of four:
    // PMC reads 216 -> MB per 16 images for a 79 MB descriptor volume.
    int blk = blockIdx.x;
    if ((gridDim.x & 7) == 0) {
        const int per = ((n + 3) / 4 + 7) >> 3;              // 4-keypoint groups per XCD
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        if (slot >= per) return;
        blk = xcd * per + slot;
    }
    const int i = blk * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const int* kb = kp + ((int64_t)b * cap + i) * 2;
    const float ky = (float)kb[0], kx = (float)kb[1];
    const float gy = ky / ((float)H * 0.5f) - 1.0f, gx = kx / ((float)W * 0.5f) - 1.0f;
    const float iy = (gy + 1.f) * ((float)(Hc - 1) / 2.f), ix = (gx + 1.f) * ((float)(Wc - 1) / 2.f);   // ATen CPU: (g + 1) * ((size-1)/2)
    const float iyn = floorf(iy), ixw = floorf(ix);
    const float iys = iyn + 1.f, ixe = ixw + 1.f;
    const float nw = (ixe - ix) * (iys - iy), ne = (ix - ixw) * (iys - iy);
    const float sw = (ixe - ix) * (iy - iyn), se = (ix - ixw) * (iy - iyn);
    const int y0 = (int)iyn, x0 = (int)ixw, y1 = y0 + 1, x1 = x0 + 1;
    const bool vy0 = y0 >= 0 && y0 < Hc, vy1 = y1 >= 0 && y1 < Hc, vx0 = x0 >= 0 && x0 < Wc, vx1 = x1 >= 0 && x1 < Wc;
    const float* db = desc + (int64_t)b * Hc * Wc * D;
    if (D == 256) {
        // the configured descriptor size: a lane owns 4 consecutive channels, a cell's row is ONE 16-byte-per-lane load (4 loads per keypoint
        // instead of 16); products and sums in the order of the general path below (nw, ne, sw, se), so results are identical
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = (vy0 && vx0) ? reinterpret_cast<const float4*>(db + ((int64_t)y0 * Wc + x0) * 256)[lane] : z;
        const float4 bq = (vy0 && vx1) ? reinterpret_cast<const float4*>(db + ((int64_t)y0 * Wc + x1) * 256)[lane] : z;
        const float4 cq = (vy1 && vx0) ? reinterpret_cast<const float4*>(db + ((int64_t)y1 * Wc + x0) * 256)[lane] : z;
        const float4 dq = (vy1 && vx1) ? reinterpret_cast<const float4*>(db + ((int64_t)y1 * Wc + x1) * 256)[lane] : z;
        auto mix = [&](float p0, float p1, float p2, float p3) {
            float o = 0.f;
            if (vy0 && vx0) o = p0 * nw;
            if (vy0 && vx1) o += p1 * ne;
            if (vy1 && vx0) o += p2 * sw;
            if (vy1 && vx1) o += p3 * se;
            return o;
        };
        float4 o4;
        o4.x = mix(a.x, bq.x, cq.x, dq.x); o4.y = mix(a.y, bq.y, cq.y, dq.y); o4.z = mix(a.z, bq.z, cq.z, dq.z); o4.w = mix(a.w, bq.w, cq.w, dq.w);
        // the general path sums the squares of channels lane, lane + 64, ... per lane; here a lane holds 4 neighbours — a different (equally
        // valid) association of the same 256 squares, so the norm may differ in the last bit
        float ss4 = fmaf(o4.x, o4.x, 0.f); ss4 = fmaf(o4.y, o4.y, ss4); ss4 = fmaf(o4.z, o4.z, ss4); ss4 = fmaf(o4.w, o4.w, ss4);
        const float nrm4 = fmaxf(sqrtf(xp_wave_sum(ss4)), 1e-12f);
        float4 r4; r4.x = o4.x / nrm4; r4.y = o4.y / nrm4; r4.z = o4.z / nrm4; r4.w = o4.w / nrm4;
        reinterpret_cast<float4*>(out + ((int64_t)b * cap + i) * 256)[lane] = r4;
        return;
    }
    float v[8];
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int c = lane + 64 * t;
        float o = 0.f;
        if (c < D) {
            if (vy0 && vx0) o = db[((int64_t)y0 * Wc + x0) * D + c] * nw;
            if (vy0 && vx1) o += db[((int64_t)y0 * Wc + x1) * D + c] * ne;
            if (vy1 && vx0) o += db[((int64_t)y1 * Wc + x0) * D + c] * sw;
            if (vy1 && vx1) o += db[((int64_t)y1 * Wc + x1) * D + c] * se;
        }
        v[t] = o;
        ss = fmaf(o, o, ss);
    }
    const float nrm = fmaxf(sqrtf(xp_wave_sum(ss)), 1e-12f);
    float* ob = out + ((int64_t)b * cap + i) * D;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int c = lane + 64 * t;
        if (c < D) ob[c] = v[t] / nrm;
    }
}

template <int V>
void kp_launch(const float* prob, const uint8_t* mask, float thr, int* seg, int* kp, int* counts, int batch, int64_t HW, int W, int cap, hipStream_t s) {
    const int nseg = xp_cdiv(HW, V * KP_SEG);
    hipLaunchKernelGGL(kp_count_kernel<V>, dim3(nseg, batch), dim3(KP_SEG), 0, s, prob, mask, thr, seg, HW, nseg);
    hipLaunchKernelGGL(kp_scan_kernel, dim3(batch), dim3(1024), 0, s, seg, counts, nseg);
    hipLaunchKernelGGL(kp_write_kernel<V>, dim3(nseg, batch), dim3(KP_SEG), 0, s, prob, mask, thr, seg, kp, HW, W, nseg, cap);
}

}  // namespace

extern "C" size_t xp_extract_keypoints_workspace_bytes(int batch, int H, int W) {
    return sizeof(int) * (size_t)batch * (size_t)xp_cdiv((int64_t)H * W, KP_SEG) + 256;
}

extern "C" int xp_extract_keypoints(const float* prob, const uint8_t* mask, float thr, int* kp, int* counts, int batch,
                                    int H, int W, int cap, void* workspace, size_t workspace_bytes, void* stream) {
    XP_CHECK_ARG(prob && kp && counts && workspace, "xp_extract_keypoints: null pointer");
    XP_CHECK_ARG(batch > 0 && cap > 0, "xp_extract_keypoints: bad batch/cap");
    XP_CHECK_ARG(workspace_bytes >= xp_extract_keypoints_workspace_bytes(batch, H, W), "xp_extract_keypoints: workspace too small");
    const int64_t HW = (int64_t)H * W;
    hipStream_t s = (hipStream_t)stream;
    XpProfScope prof("extract_keypoints", s, 0.0, 8.0 * batch * H * W);
    const bool vec4 = HW % 4 == 0 && (((uintptr_t)prob & 15) == 0) && (!mask || ((uintptr_t)mask & 3) == 0);
    if (vec4) kp_launch<4>(prob, mask, thr, (int*)workspace, kp, counts, batch, HW, W, cap, s);
    else kp_launch<1>(prob, mask, thr, (int*)workspace, kp, counts, batch, HW, W, cap, s);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_sample_descriptors(const int* kp, const int* counts, const float* desc_nhwc, float* out, int batch,
                                     int cap, int Hc, int Wc, int D, int H, int W, void* stream) {
    XP_CHECK_ARG(kp && counts && desc_nhwc && out, "xp_sample_descriptors: null pointer");
    XP_CHECK_ARG(D > 0 && D <= 512, "xp_sample_descriptors: D must be in [1,512] (got %d)", D);
    dim3 grid(xp_cdiv(cap, 4), batch);
    XpProfScope prof("sample_descriptors", (hipStream_t)stream, 0.0, 0.0);
    hipLaunchKernelGGL(sample_descriptors_kernel, grid, dim3(256), 0, (hipStream_t)stream, kp, counts, desc_nhwc, out, cap, Hc, Wc, D, H, W);
    XP_LAUNCH_CHECK();
    return XP_OK;
}
