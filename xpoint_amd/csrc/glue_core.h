// The HBM-bound glue operations that exist in more than one precision class, each stated ONCE: depthwise 3x3 + SiLU, the stem convolution
// (+ LayerNorm + GELU) and the 4-channel depth-to-space.  The __global__ kernels of elementwise.hip (f32 containers: the f32 class and,
// with R16, the "amp16" class of xp_set_amp_mode(1)) and of elementwise_f16.hip (fp16 storage, "amp16f") are thin wrappers around the
// bodies below; they keep their names because the profiling tags, tools/ and DESIGN.md section 3 refer to them.
//   T    storage type of the activations: float or _Float16.  It decides how a 4-channel vector is loaded and stored (and the stem's LDS
//        staging type and row stride) and nothing else: all arithmetic is f32 on the loaded values, in one order.
//   R16  round to fp16 at the points where autocast ends an operation in a half tensor.  With fp16 storage every store is such a point,
//        so T = _Float16 implies R16; <float, true> applies the same roundings at the same points, which makes the two mixed-precision
//        classes bit-identical for these operations (tests/test_gpu_glue_classes.py).
// LayerNorm is NOT here, on purpose: layernorm_vec_kernel gives a lane float4s summed as (x + y) + (z + w), layernorm_f16_kernel gives a lane
// 8 halves summed as a three-level tree, with a different lane-to-column mapping, and the amp16 class is the f32 kernel plus a separate
// xp_round_f16 launch.  One body would change result bits or need a width-generic reduction longer than the two kernels it replaces.
// nthr: blockDim.x, read by the __global__ wrapper and passed in.  Read inside a __device__ function it compiles to the form that allows a partial last
// workgroup (a compare against the grid size and a dependent 2-byte global load before the first useful instruction); in a kernel it is one scalar load.
#pragma once
#include "xp_common.h"

typedef _Float16 xp_h4 __attribute__((ext_vector_type(4)));
typedef _Float16 xp_h8 __attribute__((ext_vector_type(8)));

template <typename T> struct XpGlueVec;
template <> struct XpGlueVec<float> { typedef float4 v4; };
template <> struct XpGlueVec<_Float16> { typedef xp_h4 v4; };
template <typename T> constexpr bool xp_glue_half = sizeof(T) == 2;

__device__ __forceinline__ float4 xp_glue_f4(const float4 v) { return v; }
__device__ __forceinline__ float4 xp_glue_f4(const xp_h4 v) { return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]); }
__device__ __forceinline__ float4 xp_r16(const float4 v) { return make_float4(xp_r16(v.x), xp_r16(v.y), xp_r16(v.z), xp_r16(v.w)); }

// ---------------------------------------------------------------------------------------------
// Depthwise 3x3 (zero pad 1, no bias) + SiLU, NHWC.  Reference VMamba.py:655-658.
// weight layout [9][C] (tap-major, f32) so that a lane's 4 channels are one 16-B load.
// ---------------------------------------------------------------------------------------------
// Each thread produces a PH x PW = 4 x 4 block of pixels x 4 channels, streaming the PH + 2 input rows of its 6-column window
// once (36 vector loads per 16 outputs; a thread per output row re-reads two of its three rows: 72).  0.285 -> 0.244 ms per step (f32).  Every output still
// accumulates its taps in (kh, kw) order with padded taps skipped — input rows arrive in ascending order, and an input row ih
// is tap kh = ih - oh + 1 of output row oh — so results are bit-identical to the one-row form.
// R16: the convolution's output and the SiLU's output are half tensors under autocast: both rounded to fp16.  F32COPY (fp16 storage): y32 also gets the values.
// (fp16 storage: an 8-channel / 16-byte form with packed-half operands and mixed-precision FMAs was built and measured SLOWER: 0.245 vs 0.219 ms per step at
// 172 registers; the kernel is not load-width-bound.)
template <typename T, bool R16, bool F32COPY, int PH, int PW>
__device__ __forceinline__ void xp_dwconv3x3_silu_body(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ y, float* __restrict__ y32,
                                                       int B, int H, int W, int C, unsigned nthr) {
    static_assert(R16 || !xp_glue_half<T>, "fp16 storage rounds at every store");
    typedef typename XpGlueVec<T>::v4 V;
    const int C4 = C >> 2;
    const int WG = (W + PW - 1) / PW, HG = (H + PH - 1) / PH;
    const int64_t total = (int64_t)B * HG * WG * C4;
    // XCD-aware block order (workgroup ids go round-robin to the 8 XCDs, one L2 each): every XCD takes one contiguous run of blocks = a band of
    // image rows, so the halo rows that vertically adjacent blocks share are fetched once per band, not once per block (144 -> MB per launch mix)
    const unsigned nb = gridDim.x, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, q = nb >> 3, r = nb & 7;
    const unsigned blk = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    const int64_t idx = (int64_t)blk * nthr + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    const int64_t g = idx / C4;
    const int w0 = (int)(g % WG) * PW;
    const int h0 = (int)((g / WG) % HG) * PH;
    const int64_t b = g / ((int64_t)WG * HG);
    const V* xv = reinterpret_cast<const V*>(x);
    float4 wt[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[t] = reinterpret_cast<const float4*>(w)[t * C4 + c4];
    float4 acc[PH][PW];
#pragma unroll
    for (int rr = 0; rr < PH; ++rr)
#pragma unroll
        for (int p = 0; p < PW; ++p) acc[rr][p] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int ir = 0; ir < PH + 2; ++ir) {
        const int ih = h0 + ir - 1;
        if (ih < 0 || ih >= H) continue;          // zero padding: a skipped row adds nothing (same sum order for the rest)
        float4 col[PW + 2];
#pragma unroll
        for (int cx = 0; cx < PW + 2; ++cx) {
            const int iw = w0 + cx - 1;
            // the load is spelled per storage type, not through a helper: a shared `load(base, index, ok)` changes how the compiler predicates it (+60 instructions, +2 registers per instance)
            if constexpr (xp_glue_half<T>) {
                V t = {};
                if (iw >= 0 && iw < W) t = xv[((b * H + ih) * W + iw) * C4 + c4];
                col[cx] = xp_glue_f4(t);
            } else {
                col[cx] = (iw >= 0 && iw < W) ? xv[((b * H + ih) * W + iw) * C4 + c4] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int rr = 0; rr < PH; ++rr) {
            const int kh = ir - rr;               // this input row is tap kh of output row h0 + rr
            if (kh < 0 || kh > 2) continue;
#pragma unroll
            for (int p = 0; p < PW; ++p)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int iw = w0 + p + kw - 1;
                    if (iw < 0 || iw >= W) continue;   // keep the reference's accumulation order: padded taps are skipped, not added as 0
                    const float4 xin = col[p + kw], wv = wt[kh * 3 + kw];
                    acc[rr][p].x = fmaf(xin.x, wv.x, acc[rr][p].x); acc[rr][p].y = fmaf(xin.y, wv.y, acc[rr][p].y);
                    acc[rr][p].z = fmaf(xin.z, wv.z, acc[rr][p].z); acc[rr][p].w = fmaf(xin.w, wv.w, acc[rr][p].w);
                }
        }
    }
#pragma unroll
    for (int rr = 0; rr < PH; ++rr) {
        if (h0 + rr >= H) break;
#pragma unroll
        for (int p = 0; p < PW; ++p) {
            if (w0 + p >= W) break;
            float4 o = acc[rr][p];
            if (R16) o = xp_r16(o);
            o.x = xp_silu(o.x); o.y = xp_silu(o.y); o.z = xp_silu(o.z); o.w = xp_silu(o.w);
            if (R16) o = xp_r16(o);
            const int64_t oi = ((b * H + h0 + rr) * W + w0 + p) * C4 + c4;
            if constexpr (xp_glue_half<T>) reinterpret_cast<V*>(y)[oi] = V{(_Float16)o.x, (_Float16)o.y, (_Float16)o.z, (_Float16)o.w};     // exact: o is rounded
            else reinterpret_cast<V*>(y)[oi] = o;
            if (F32COPY) reinterpret_cast<float4*>(y32)[oi] = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Stem: gray image (B,1,H,W) -> conv3x3 stride 2 pad 1 (1 -> CO channels; the reference replicates gray
// to 3 channels, VMamba.py:1509-1510, so the 3 input-channel weights are pre-summed on the host)
// + bias + LayerNorm(CO) + GELU -> NHWC (B,H/2,W/2,CO).  Reference VMamba.py:1411-1416.
// One thread per output pixel, CO accumulators in registers; output staged through LDS (in the storage type; row stride CO + 1 floats or
// CO + 2 halves) for coalesced stores.
// ---------------------------------------------------------------------------------------------
// R16: the image is cast to half by autocast's convolution, and conv, LayerNorm and GELU each return a half tensor
// The stem's convolution of ONE output pixel: acc[c] = bias[c] + sum_t x[t] w[t][c] (s_w: [tap][CO], the bias in row 9), returns sum_c acc[c].  The fused
// kernel below and the training forward's xp_stem_conv share it: one summation order, the same bits.
template <int CO, bool R16>
__device__ __forceinline__ float xp_stem_conv_pixel(const float* __restrict__ img, const float* s_w, int64_t b, int oh, int ow, int H, int W, float (&acc)[CO]) {
    float xin[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ih = oh * 2 + kh - 1, iw = ow * 2 + kw - 1;
            xin[kh * 3 + kw] = (ih >= 0 && ih < H && iw >= 0 && iw < W) ? img[(b * H + ih) * W + iw] : 0.f;
            if (R16) xin[kh * 3 + kw] = xp_r16(xin[kh * 3 + kw]);
        }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CO; ++c) {
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) a = fmaf(xin[t], s_w[t * CO + c], a);
        a += s_w[9 * CO + c];
        if (R16) a = xp_r16(a);
        acc[c] = a; s += a;
    }
    return s;
}

template <int CO, typename T, bool R16>
__device__ __forceinline__ void xp_stem_conv_ln_gelu_body(const float* __restrict__ img, const float* __restrict__ w9, const float* __restrict__ bias,
                                                          const float* __restrict__ lnw, const float* __restrict__ lnb, T* __restrict__ y,
                                                          int B, int H, int W, float eps) {
    static_assert(R16 || !xp_glue_half<T>, "fp16 storage rounds at every store");
    constexpr int LDO = CO + (xp_glue_half<T> ? 2 : 1);
    __shared__ float s_w[12 * CO];
    __shared__ T s_o[64 * LDO];
    for (int i = threadIdx.x; i < 9 * CO; i += 64) s_w[i] = w9[i];          // [tap][CO]
    for (int i = threadIdx.x; i < CO; i += 64) { s_w[9 * CO + i] = bias[i]; s_w[10 * CO + i] = lnw[i]; s_w[11 * CO + i] = lnb[i]; }
    __syncthreads();
    const int Ho = H / 2 + (H & 1), Wo = W / 2 + (W & 1);   // floor((H+2-3)/2)+1
    const int64_t total = (int64_t)B * Ho * Wo;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int64_t pix = p0 + threadIdx.x;
    if (pix < total) {
        const int ow = (int)(pix % Wo), oh = (int)((pix / Wo) % Ho);
        const int64_t b = pix / ((int64_t)Wo * Ho);
        float acc[CO];
        const float s = xp_stem_conv_pixel<CO, R16>(img, s_w, b, oh, ow, H, W, acc);
        const float mean = s / (float)CO;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CO; ++c) { const float d = acc[c] - mean; q = fmaf(d, d, q); }
        const float rstd = 1.f / sqrtf(q / (float)CO + eps);
#pragma unroll
        for (int c = 0; c < CO; ++c) {
            float v = (acc[c] - mean) * rstd * s_w[10 * CO + c] + s_w[11 * CO + c];
            if (R16) v = xp_r16(v);
            v = xp_gelu_fast(v);
            if (R16) v = xp_r16(v);
            s_o[threadIdx.x * LDO + c] = (T)v;
        }
    }
    __syncthreads();
    const int64_t nvalid = (total - p0 < 64) ? (total - p0) : 64;
    for (int i = threadIdx.x; i < nvalid * CO; i += 64) {
        const int pl = i / CO, c = i - pl * CO;
        y[(p0 + pl) * CO + c] = s_o[pl * LDO + c];
    }
}

// The stem's convolution alone (f32): what the training forward keeps as the LayerNorm's input.  Same staging as the fused body.
template <int CO>
__device__ __forceinline__ void xp_stem_conv_body(const float* __restrict__ img, const float* __restrict__ w9, const float* __restrict__ bias,
                                                  float* __restrict__ y, int B, int H, int W) {
    constexpr int LDO = CO + 1;
    __shared__ float s_w[10 * CO];
    __shared__ float s_o[64 * LDO];
    for (int i = threadIdx.x; i < 9 * CO; i += 64) s_w[i] = w9[i];
    for (int i = threadIdx.x; i < CO; i += 64) s_w[9 * CO + i] = bias[i];
    __syncthreads();
    const int Ho = H / 2 + (H & 1), Wo = W / 2 + (W & 1);
    const int64_t total = (int64_t)B * Ho * Wo;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int64_t pix = p0 + threadIdx.x;
    if (pix < total) {
        const int ow = (int)(pix % Wo), oh = (int)((pix / Wo) % Ho);
        const int64_t b = pix / ((int64_t)Wo * Ho);
        float acc[CO];
        (void)xp_stem_conv_pixel<CO, false>(img, s_w, b, oh, ow, H, W, acc);
#pragma unroll
        for (int c = 0; c < CO; ++c) s_o[threadIdx.x * LDO + c] = acc[c];
    }
    __syncthreads();
    const int64_t nvalid = (total - p0 < 64) ? (total - p0) : 64;
    for (int i = threadIdx.x; i < nvalid * CO; i += 64) {
        const int pl = i / CO, c = i - pl * CO;
        y[(p0 + pl) * CO + c] = s_o[pl * LDO + c];
    }
}

// ---------------------------------------------------------------------------------------------
// depth_to_space(bs) in NHWC, 4-channel vector form (Cq % 4 == 0, aligned buffers, < 2^31 elements): a thread moves four channels of one block —
// 32-bit index arithmetic.  out[n, bs*h+i, bs*w+j, c] = x[n, h, w, (bs*i+j)*Cq + c]  (VMamba.py:1500-1505; block-major channel order, NOT PixelShuffle order).
// ---------------------------------------------------------------------------------------------
// status != NULL: bit XP_STATUS_ENC is OR-ed into *status when an element is non-finite or |x| >= limit (one atomic per wave that saw one).
// float: y32 is the output, y16 unused.  _Float16: the f32 output (the API's `encoder_output`) and a half copy (the head convolution's operand); limit = INFINITY (a half overflow is +-inf).
template <typename T>
__device__ __forceinline__ void xp_depth_to_space_vec_body(const typename XpGlueVec<T>::v4* __restrict__ x, float4* __restrict__ y32,
                                                           typename XpGlueVec<T>::v4* __restrict__ y16, int B, int H, int W, int C4, int bs,
                                                           float limit, int* __restrict__ status, unsigned nthr) {
    typedef typename XpGlueVec<T>::v4 V;
    const int Cq4 = C4 / (bs * bs);
    const unsigned total = (unsigned)B * H * W * C4;
    const unsigned idx = blockIdx.x * nthr + threadIdx.x;
    V v;
    if constexpr (xp_glue_half<T>) { v = V{}; if (idx < total) v = x[idx]; }
    else v = idx < total ? x[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 f = xp_glue_f4(v);
    if (status) {
        const bool bad = !(fabsf(f.x) < limit) || !(fabsf(f.y) < limit) || !(fabsf(f.z) < limit) || !(fabsf(f.w) < limit);        // NaN compares false
        if (__ballot(bad && idx < total) != 0ull && (threadIdx.x & 63) == 0) atomicOr(status, XP_STATUS_ENC);
    }
    if (idx >= total) return;
    const unsigned ch = idx % (unsigned)C4, pix = idx / (unsigned)C4;
    const unsigned w = pix % (unsigned)W, hn = pix / (unsigned)W, h = hn % (unsigned)H, n = hn / (unsigned)H;
    const unsigned blk = ch / (unsigned)Cq4, c = ch - blk * Cq4;
    const unsigned i = blk / (unsigned)bs, j = blk - i * bs;
    const unsigned o = ((n * (H * bs) + (h * bs + i)) * (unsigned)(W * bs) + (w * bs + j)) * Cq4 + c;
    y32[o] = f;
    if constexpr (xp_glue_half<T>) y16[o] = v;
}
