// Selective-scan forward at the reference operator boundary (drop-in for
// selective_scan_cuda_oflex.fwd: reference kernels/selective_scan/csrc/selective_scan/cusoflex/
// selective_scan_oflex.cpp:143-231 and selective_scan_fwd_kernel_oflex.cuh:67-181).
//
// Layout (all float32, L contiguous): u, delta (B, D, L) [delta may be (B, Dd, L), D % Dd == 0];
// A (D, N); Bm, Cm (B, G, N, L); Dv, delta_bias optional; out (B, D, L); last_state (B, D, N).
//
// CDNA4 mapping: one 64-lane wave owns one (batch, channel) row and walks it in 256-element
// chunks (4 contiguous floats per lane = one 16-B load per operand per lane, 1 KiB per wave
// instruction).  The linear recurrence h_l = a_l h_{l-1} + b_l is evaluated as a scan of
// (a, b) pairs with op (a1*a0, a1*b0 + b1): 4 items serially per lane, 6 shuffle steps across
// the wave, and a register carry between chunks.  No LDS, no barriers; HBM-bound.
#include <stdlib.h>

#include "xp_common.h"

namespace {

constexpr int kItems = 4;
constexpr int kChunk = 64 * kItems;

template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, int64_t off, int rem, float (&v)[kItems], float fill) {
    if (VEC && rem >= kItems) {
        float4 t = *reinterpret_cast<const float4*>(p + off);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < kItems; ++i) v[i] = (i < rem) ? p[off + i] : fill;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void selective_scan_fwd_kernel(
    const float* __restrict__ u, const float* __restrict__ delta, const float* __restrict__ A,
    const float* __restrict__ Bm, const float* __restrict__ Cm, const float* __restrict__ Dv,
    const float* __restrict__ delta_bias, float* __restrict__ out, float* __restrict__ last_state,
    int batch, int dim, int delta_dim, int L, int N, int G, int softplus) {
    __shared__ float carry[4][256];  // per-wave running state for N > 1 (MAX_DSTATE 256 as the reference)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= (int64_t)batch * dim) return;
    const int b = (int)(row / dim), d = (int)(row % dim);
    const int g = d / (dim / G);
    const int dd = d / (dim / delta_dim);
    const float* up = u + row * L;
    const float* dp = delta + ((int64_t)b * delta_dim + dd) * L;
    const float* Bp = Bm + ((int64_t)b * G + g) * N * L;
    const float* Cp = Cm + ((int64_t)b * G + g) * N * L;
    float* op = out + row * L;
    const float Dval = Dv ? Dv[d] : 0.f;
    const float bias = delta_bias ? delta_bias[dd] : 0.f;
    float h1 = 0.f;  // carry for N == 1
    for (int n = lane; n < N; n += 64) carry[wave][n] = 0.f;

    for (int c0 = 0; c0 < L; c0 += kChunk) {
        const int off = c0 + lane * kItems;
        const int rem = L - off;  // may be <= 0
        float uv[kItems], dv[kItems], ov[kItems];
        load4<VEC>(up, off, rem, uv, 0.f);
        load4<VEC>(dp, off, rem, dv, 0.f);
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            float t = dv[i] + bias;
            dv[i] = softplus ? xp_softplus_fast(t) : t;
            ov[i] = Dval * uv[i];
        }
        for (int n = 0; n < N; ++n) {
            const float An = A[(int64_t)d * N + n];
            float bv[kItems], cv[kItems];
            load4<VEC>(Bp + (int64_t)n * L, off, rem, bv, 0.f);
            load4<VEC>(Cp + (int64_t)n * L, off, rem, cv, 0.f);
            float la[kItems], lb[kItems];
            float pa = 1.f, pb = 0.f;
#pragma unroll
            for (int i = 0; i < kItems; ++i) {
                float a = (i < rem) ? xp_exp_fast(dv[i] * An) : 1.f;   // identity past the end keeps last_state right
                float bb = (i < rem) ? dv[i] * bv[i] * uv[i] : 0.f;
                pb = a * pb + bb;
                pa = a * pa;
                la[i] = pa; lb[i] = pb;
            }
            // inclusive wave scan of the per-lane totals
            float ta = pa, tb = pb;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                float ua = __shfl_up(ta, o, 64), ub = __shfl_up(tb, o, 64);
                if (lane >= o) { tb = ta * ub + tb; ta = ta * ua; }
            }
            float ea = __shfl_up(ta, 1, 64), eb = __shfl_up(tb, 1, 64);
            if (lane == 0) { ea = 1.f; eb = 0.f; }
            const float hprev = (N == 1) ? h1 : carry[wave][n];
            const float hin = ea * hprev + eb;          // state entering this lane's first item
#pragma unroll
            for (int i = 0; i < kItems; ++i) ov[i] += cv[i] * (la[i] * hin + lb[i]);
            const float hend = __shfl(ta, 63, 64) * hprev + __shfl(tb, 63, 64);
            if (N == 1) h1 = hend; else if (lane == 0) carry[wave][n] = hend;
        }
        if (VEC && rem >= kItems) {
            *reinterpret_cast<float4*>(op + off) = make_float4(ov[0], ov[1], ov[2], ov[3]);
        } else {
#pragma unroll
            for (int i = 0; i < kItems; ++i) if (i < rem) op[off + i] = ov[i];
        }
    }
    if (last_state) {
        if (N == 1) { if (lane == 0) last_state[row] = h1; }
        else for (int n = lane; n < N; n += 64) last_state[row * N + n] = carry[wave][n];
    }
}


// d_state == 1: the optional per-2048-element chunk state x (batch, dim, ceil(L / 2048), 2) of xp_selective_scan_fwd_x -- the running product
// of the decays and h at the end of every chunk, the layout of the general kernel's x output below.  Called after every step of `step` elements
// starting at c0 with the step's total decay; only bookkeeping, the output arithmetic is untouched.
__device__ __forceinline__ void xc_record(float* xchunks, int64_t row, int L, int c0, int step, int lane, float& pr, float step_a, float h) {
    pr *= step_a;
    if (lane == 0 && ((c0 + step) % 2048 == 0 || c0 + step >= L)) {
        float* xp = xchunks + (row * ((L + 2047) / 2048) + c0 / 2048) * 2;
        xp[0] = pr; xp[1] = h;
    }
}

// d_state == 1 (the XPoint configuration), software pipelined: the four 16-byte loads of chunk c+1 are issued before the
// arithmetic of chunk c, so a wave always has a chunk of HBM traffic in flight behind its transcendental work.
template <bool VEC>
__global__ __launch_bounds__(256) void selective_scan_fwd_n1_kernel(
    const float* __restrict__ u, const float* __restrict__ delta, const float* __restrict__ A,
    const float* __restrict__ Bm, const float* __restrict__ Cm, const float* __restrict__ Dv,
    const float* __restrict__ delta_bias, float* __restrict__ out, float* __restrict__ last_state,
    float* __restrict__ xchunks,
    int batch, int dim, int delta_dim, int L, int G, int softplus) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= (int64_t)batch * dim) return;
    const int b = (int)(row / dim), d = (int)(row % dim);
    const int g = d / (dim / G), dd = d / (dim / delta_dim);
    const float* up = u + row * L;
    const float* dp = delta + ((int64_t)b * delta_dim + dd) * L;
    const float* Bp = Bm + ((int64_t)b * G + g) * L;
    const float* Cp = Cm + ((int64_t)b * G + g) * L;
    float* op = out + row * L;
    const float Dval = Dv ? Dv[d] : 0.f, bias = delta_bias ? delta_bias[dd] : 0.f, An = A[d];
    float h = 0.f, pr = 1.f;
    float uv[kItems], dv[kItems], bv[kItems], cv[kItems];
    auto fetch = [&](int c0) {
        const int off = c0 + lane * kItems, rem = L - off;
        load4<VEC>(up, off, rem, uv, 0.f); load4<VEC>(dp, off, rem, dv, 0.f);
        load4<VEC>(Bp, off, rem, bv, 0.f); load4<VEC>(Cp, off, rem, cv, 0.f);
    };
    fetch(0);
    for (int c0 = 0; c0 < L; c0 += kChunk) {
        const int off = c0 + lane * kItems, rem = L - off;
        float cu[kItems], cd[kItems], cb[kItems], cc[kItems];
#pragma unroll
        for (int i = 0; i < kItems; ++i) { cu[i] = uv[i]; cd[i] = dv[i]; cb[i] = bv[i]; cc[i] = cv[i]; }
        if (c0 + kChunk < L) fetch(c0 + kChunk);           // next chunk in flight
        float la[kItems], lb[kItems];
        float pa = 1.f, pb = 0.f;
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            const float t = cd[i] + bias;
            float dl, aa;
            if (softplus) xp_softplus_decay(t, An, dl, aa);
            else { dl = t; aa = xp_exp_fast(t * An); }
            const float a = (i < rem) ? aa : 1.f;
            const float bb = (i < rem) ? dl * cb[i] * cu[i] : 0.f;
            pb = a * pb + bb; pa = a * pa;
            la[i] = pa; lb[i] = pb;
        }
        float ta = pa, tb = pb;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float ua = __shfl_up(ta, o, 64), ub = __shfl_up(tb, o, 64);
            if (lane >= o) { tb = ta * ub + tb; ta = ta * ua; }
        }
        float ea = __shfl_up(ta, 1, 64), eb = __shfl_up(tb, 1, 64);
        if (lane == 0) { ea = 1.f; eb = 0.f; }
        const float hin = ea * h + eb;
        float ov[kItems];
#pragma unroll
        for (int i = 0; i < kItems; ++i) ov[i] = Dval * cu[i] + cc[i] * (la[i] * hin + lb[i]);
        h = __shfl(ta, 63, 64) * h + __shfl(tb, 63, 64);
        if (xchunks) xc_record(xchunks, row, L, c0, kChunk, lane, pr, __shfl(ta, 63, 64), h);
        if (VEC && rem >= kItems) {
            *reinterpret_cast<float4*>(op + off) = make_float4(ov[0], ov[1], ov[2], ov[3]);
        } else {
#pragma unroll
            for (int i = 0; i < kItems; ++i) if (i < rem) op[off + i] = ov[i];
        }
    }
    if (last_state && lane == 0) last_state[row] = h;
}


// ---------------------------------------------------------------------------------------------------------------------
// d_state == 1, 16-byte aligned rows: 8 items per lane (512-element chunks), full chunks on a branch-free path (the per-lane
// `rem` tests of the generic kernel compile to exec-mask branches around every load and store), the 64-lane scan of the
// (a, b) pairs on DPP moves (row_shr 1/2/4/8, row_bcast 15/31; hipcc lowers __shfl_up to ds_bpermute: 16 LDS crossbar round
// trips per chunk on the serial path), delta and exp(delta*A) from one logarithm as in the fused SS2D core.
// ---------------------------------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float xp_dpp(float identity, float v) {      // lanes without a source (or outside ROW_MASK) get `identity`
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
// inclusive scan over the wave of h -> a h + b maps, earlier lanes first: (a, b) <- (a * ea, a * eb + b) with (ea, eb) the incoming prefix
__device__ __forceinline__ void xp_wave_scan_ab(float& a, float& b) {
#define XP_SCAN_STEP(CTRL, MASK) { const float ea = xp_dpp<CTRL, MASK>(1.f, a), eb = xp_dpp<CTRL, MASK>(0.f, b); b = fmaf(a, eb, b); a = a * ea; }
    XP_SCAN_STEP(0x111, 0xf)      // row_shr:1
    XP_SCAN_STEP(0x112, 0xf)      // row_shr:2
    XP_SCAN_STEP(0x114, 0xf)      // row_shr:4
    XP_SCAN_STEP(0x118, 0xf)      // row_shr:8
    XP_SCAN_STEP(0x142, 0xa)      // row_bcast:15 into rows 1 and 3
    XP_SCAN_STEP(0x143, 0xc)      // row_bcast:31 into rows 2 and 3
#undef XP_SCAN_STEP
}

constexpr int kItems8 = 8, kChunk8 = 64 * kItems8;
__global__ __launch_bounds__(256) void selective_scan_fwd_n1v2_kernel(
    const float* __restrict__ u, const float* __restrict__ delta, const float* __restrict__ A,
    const float* __restrict__ Bm, const float* __restrict__ Cm, const float* __restrict__ Dv,
    const float* __restrict__ delta_bias, float* __restrict__ out, float* __restrict__ last_state,
    float* __restrict__ xchunks,
    int batch, int dim, int delta_dim, int L, int G, int softplus) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= (int64_t)batch * dim) return;
    const int b = (int)(row / dim), d = (int)(row % dim);
    const int g = d / (dim / G), dd = d / (dim / delta_dim);
    const float* up = u + row * L + lane * kItems8;
    const float* dp = delta + ((int64_t)b * delta_dim + dd) * L + lane * kItems8;
    const float* Bp = Bm + ((int64_t)b * G + g) * L + lane * kItems8;
    const float* Cp = Cm + ((int64_t)b * G + g) * L + lane * kItems8;
    float* op = out + row * L + lane * kItems8;
    const float Dval = Dv ? Dv[d] : 0.f, bias = delta_bias ? delta_bias[dd] : 0.f, An = A[d];
    float h = 0.f, pr = 1.f;
    // one step's (a, b): delta = softplus(x) (torch threshold 20), a = exp(delta * A); below the threshold both from ONE logarithm:
    // delta = ln(1 + e^x), a = (1 + e^x)^A = 2^(A log2(1 + e^x))   (same arithmetic as step_vals in ss2d_core.h)
    auto step = [&](float x, float Bu, float& a, float& bb) {
        float dl;
        if (softplus) xp_softplus_decay(x, An, dl, a);
        else { dl = x; a = xp_exp_fast(x * An); }
        bb = dl * Bu;
    };
    const int nfull = L / kChunk8;
    float4 nu[2], nd[2], nb[2], nc[2];
    auto fetch = [&](int c) {
        const int o = c * kChunk8;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            nu[q] = *reinterpret_cast<const float4*>(up + o + 4 * q); nd[q] = *reinterpret_cast<const float4*>(dp + o + 4 * q);
            nb[q] = *reinterpret_cast<const float4*>(Bp + o + 4 * q); nc[q] = *reinterpret_cast<const float4*>(Cp + o + 4 * q);
        }
    };
    if (nfull > 0) fetch(0);
    for (int c = 0; c < nfull; ++c) {
        float cu[8] = {nu[0].x, nu[0].y, nu[0].z, nu[0].w, nu[1].x, nu[1].y, nu[1].z, nu[1].w};
        float cd[8] = {nd[0].x, nd[0].y, nd[0].z, nd[0].w, nd[1].x, nd[1].y, nd[1].z, nd[1].w};
        float cb[8] = {nb[0].x, nb[0].y, nb[0].z, nb[0].w, nb[1].x, nb[1].y, nb[1].z, nb[1].w};
        float cc[8] = {nc[0].x, nc[0].y, nc[0].z, nc[0].w, nc[1].x, nc[1].y, nc[1].z, nc[1].w};
        if (c + 1 < nfull) fetch(c + 1);                   // next chunk in flight behind the arithmetic
        float la[8], lb[8];
        float pa = 1.f, pb = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float a, bb;
            step(cd[i] + bias, cb[i] * cu[i], a, bb);
            pb = a * pb + bb; pa = a * pa;
            la[i] = pa; lb[i] = pb;
        }
        float ta = pa, tb = pb;
        xp_wave_scan_ab(ta, tb);
        // prefix of the lanes before this one (wave_shr:1; lane 0 gets the identity), applied to the carried state
        const float ea = xp_dpp<0x138, 0xf>(1.f, ta), eb = xp_dpp<0x138, 0xf>(0.f, tb);
        const float hin = ea * h + eb;
        float ov[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ov[i] = Dval * cu[i] + cc[i] * (la[i] * hin + lb[i]);
        h = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ta), 63)) * h + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tb), 63));
        if (xchunks) xc_record(xchunks, row, L, c * kChunk8, kChunk8, lane, pr, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ta), 63)), h);
        const int o = c * kChunk8;
        *reinterpret_cast<float4*>(op + o) = make_float4(ov[0], ov[1], ov[2], ov[3]);
        *reinterpret_cast<float4*>(op + o + 4) = make_float4(ov[4], ov[5], ov[6], ov[7]);
    }
    // tail (L % 512 elements): the generic masked path, one 8-item group per lane
    const int t0 = nfull * kChunk8;
    if (t0 < L) {
        const int rem = L - t0 - lane * kItems8;        // may be <= 0
        float la[8], lb[8], cu[8], cc[8];
        float pa = 1.f, pb = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = i < rem;
            cu[i] = ok ? up[t0 + i] : 0.f; cc[i] = ok ? Cp[t0 + i] : 0.f;
            const float dvv = ok ? dp[t0 + i] : 0.f, bvv = ok ? Bp[t0 + i] : 0.f;
            float a, bb;
            step(dvv + bias, bvv * cu[i], a, bb);
            a = ok ? a : 1.f; bb = ok ? bb : 0.f;          // identity past the end keeps last_state right
            pb = a * pb + bb; pa = a * pa;
            la[i] = pa; lb[i] = pb;
        }
        float ta = pa, tb = pb;
        xp_wave_scan_ab(ta, tb);
        const float ea = xp_dpp<0x138, 0xf>(1.f, ta), eb = xp_dpp<0x138, 0xf>(0.f, tb);
        const float hin = ea * h + eb;
#pragma unroll
        for (int i = 0; i < 8; ++i) if (i < rem) op[t0 + i] = Dval * cu[i] + cc[i] * (la[i] * hin + lb[i]);
        h = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ta), 63)) * h + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tb), 63));
        if (xchunks) xc_record(xchunks, row, L, t0, kChunk8, lane, pr, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ta), 63)), h);
    }
    if (last_state && lane == 0) last_state[row] = h;
}


// ---------------------------------------------------------------------------------------------------------------------
// General form: any d_state <= 256, inputs u / delta / B / C in f32, f16 or bf16 (the reference's input_t instantiations,
// cusoflex/selective_scan_core_fwd.cu:6-10; A, D, delta_bias stay f32 and the state is always f32), output f32 ("oflex",
// out_float) or the input type, and the per-chunk scan state x (batch, dim, ceil(L / 2048), 2 N) of selective_scan_oflex.cpp:206-208:
// x[.., c, 2n] = product of exp(delta A_n) from the start of the row to the end of 2048-element chunk c, x[.., c, 2n + 1] = h_n there
// (the running prefix of the reference's block scan, selective_scan_fwd_kernel_oflex.cuh:154-162; last state = x[:, :, -1, 1::2]).
// One wave per (batch, channel) row, 512-element steps (8 items per lane: one 16-byte load per operand for the 16-bit types,
// two for f32), the (a, b) scan across the wave on DPP moves, the per-state carries (h, running product) in LDS.
// ---------------------------------------------------------------------------------------------------------------------
template <class T> struct ScanIO;
template <> struct ScanIO<float> {
    __device__ static __forceinline__ void load8(const float* p, float (&v)[8]) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    __device__ static __forceinline__ float get(const float* p) { return *p; }
    __device__ static __forceinline__ void store8(float* p, const float (&v)[8]) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    __device__ static __forceinline__ void put(float* p, float v) { *p = v; }
};
template <class H> struct ScanIO16 {
    typedef H hvec8 __attribute__((ext_vector_type(8)));
    __device__ static __forceinline__ void load8(const H* p, float (&v)[8]) {
        const hvec8 a = *reinterpret_cast<const hvec8*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)a[i];
    }
    __device__ static __forceinline__ float get(const H* p) { return (float)*p; }
    __device__ static __forceinline__ void store8(H* p, const float (&v)[8]) {
        hvec8 a;
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = (H)v[i];
        *reinterpret_cast<hvec8*>(p) = a;
    }
    __device__ static __forceinline__ void put(H* p, float v) { *p = (H)v; }
};
template <> struct ScanIO<_Float16> : ScanIO16<_Float16> {};
template <> struct ScanIO<__bf16> : ScanIO16<__bf16> {};

constexpr int kXChunk = 2048;      // the reference's chunk of the x output (selective_scan_oflex.cpp:206)

template <class T, class OT, bool EXACT_EXP>
__global__ __launch_bounds__(256) void selective_scan_fwd_gen_kernel(
    const T* __restrict__ u, const T* __restrict__ delta, const float* __restrict__ A, const T* __restrict__ Bm, const T* __restrict__ Cm,
    const float* __restrict__ Dv, const float* __restrict__ delta_bias, OT* __restrict__ out, float* __restrict__ last_state,
    float* __restrict__ xchunks, int batch, int dim, int delta_dim, int L, int N, int G, int softplus, int vec) {
    __shared__ float carry_h[4][256], carry_a[4][256];      // per wave and state: h and the running product of a (reference MAX_DSTATE 256)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= (int64_t)batch * dim) return;
    const int b = (int)(row / dim), d = (int)(row % dim);
    const int g = d / (dim / G), dd = d / (dim / delta_dim);
    const T* up = u + row * L;
    const T* dp = delta + ((int64_t)b * delta_dim + dd) * L;
    const T* Bp = Bm + ((int64_t)b * G + g) * N * L;
    const T* Cp = Cm + ((int64_t)b * G + g) * N * L;
    OT* op = out + row * L;
    const float Dval = Dv ? Dv[d] : 0.f, bias = delta_bias ? delta_bias[dd] : 0.f;
    const int nxc = (L + kXChunk - 1) / kXChunk;
    for (int n = lane; n < N; n += 64) { carry_h[wave][n] = 0.f; carry_a[wave][n] = 1.f; }
    auto ld = [&](const T* p, int off, int rem, float (&v)[8]) {
        if (vec && rem >= 8) ScanIO<T>::load8(p + off, v);
        else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = i < rem ? ScanIO<T>::get(p + off + i) : 0.f;
        }
    };
    for (int c0 = 0; c0 < L; c0 += kChunk8) {
        const int off = c0 + lane * 8, rem = L - off;       // rem may be <= 0
        float uv[8], dl[8], du[8], ov[8];
        ld(up, off, rem, uv); ld(dp, off, rem, dl);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float t = dl[i] + bias;
            dl[i] = softplus ? (EXACT_EXP ? xp_softplus_fast(t) : (t <= 20.f ? xp_log1p_fast(__builtin_amdgcn_exp2f(t * 1.44269504088896340736f)) : t)) : t;
            du[i] = dl[i] * uv[i];
            ov[i] = Dval * uv[i];
        }
        const bool xc_end = ((c0 + kChunk8) % kXChunk == 0) || (c0 + kChunk8 >= L);     // this step closes a 2048-element chunk of x
        for (int n = 0; n < N; ++n) {
            const float An = A[(int64_t)d * N + n];
            float bv[8], cv[8], la[8], lb[8];
            ld(Bp + (int64_t)n * L, off, rem, bv); ld(Cp + (int64_t)n * L, off, rem, cv);
            float pa = 1.f, pb = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float a = EXACT_EXP ? xp_exp_fast(dl[i] * An) : __builtin_amdgcn_exp2f(dl[i] * (An * 1.44269504088896340736f));
                float bb = bv[i] * du[i];
                if (i >= rem) { a = 1.f; bb = 0.f; }              // identity past the end keeps the carried state right
                pb = a * pb + bb; pa = a * pa;
                la[i] = pa; lb[i] = pb;
            }
            float ta = pa, tb = pb;
            xp_wave_scan_ab(ta, tb);
            const float ea = xp_dpp<0x138, 0xf>(1.f, ta), eb = xp_dpp<0x138, 0xf>(0.f, tb);      // prefix of the lanes before this one
            const float hprev = carry_h[wave][n], aprev = carry_a[wave][n];
            const float hin = ea * hprev + eb;
#pragma unroll
            for (int i = 0; i < 8; ++i) ov[i] += cv[i] * (la[i] * hin + lb[i]);
            const float tot_a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ta), 63));
            const float hend = tot_a * hprev + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tb), 63));
            if (lane == 0) {
                carry_h[wave][n] = hend; carry_a[wave][n] = aprev * tot_a;
                if (xchunks && xc_end) {
                    float* xp = xchunks + ((row * nxc + c0 / kXChunk) * N + n) * 2;
                    xp[0] = aprev * tot_a; xp[1] = hend;
                }
            }
        }
        if (vec && rem >= 8) ScanIO<OT>::store8(op + off, ov);
        else {
#pragma unroll
            for (int i = 0; i < 8; ++i) if (i < rem) ScanIO<OT>::put(op + off + i, ov[i]);
        }
    }
    if (last_state) for (int n = lane; n < N; n += 64) last_state[row * N + n] = carry_h[wave][n];
}

template <class T, class OT, bool EXACT>
static void launch_gen(const void* u, const void* delta, const float* A, const void* Bm, const void* Cm, const float* Dv, const float* delta_bias,
                       void* out, float* last_state, float* xchunks, int batch, int dim, int delta_dim, int L, int N, int G, int softplus, hipStream_t s) {
    const int64_t rows = (int64_t)batch * dim;
    const size_t al = 8 * sizeof(T) - 1;
    const int vec = (L % 8 == 0) && ((((uintptr_t)u | (uintptr_t)delta | (uintptr_t)Bm | (uintptr_t)Cm) & al) == 0) && (((uintptr_t)out & (8 * sizeof(OT) - 1)) == 0);
    hipLaunchKernelGGL((selective_scan_fwd_gen_kernel<T, OT, EXACT>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, (const T*)u, (const T*)delta, A,
                       (const T*)Bm, (const T*)Cm, Dv, delta_bias, (OT*)out, last_state, xchunks, batch, dim, delta_dim, L, N, G, softplus, vec);
}

// d_state = 1: rows at least this long run the 8-item DPP-scan kernel, shorter ones the 4-item kernel.  Measured (tools/scan_bench.py shapes and single
// images, 4-item vs 8-item): one image 384 x 19 200 rows 92.8 vs 52.7 us, 768 x 4 800 36.5 vs 23.1 us, 1 536 x 1 200 16.2 vs 16.1 us; 16 images
// 6 144 x 19 200 293.2 vs 306.8 us, 12 288 x 4 800 146.5 vs 152.9 us, 24 576 x 1 200 78.2 vs 112.5 us.  Long rows: the 8-item kernel (large wins for
// one or two images, <= 5 % lost at 16); short rows: the 4-item kernel
constexpr int kScanV2MinLen = 4096;

}  // namespace

// x_chunks (batch, dim, ceil(seqlen / 2048), 2 dstate) or NULL: xp_selective_scan_fwd_x
static int selective_scan_fwd_f32(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm, const float* Dv,
                                  const float* delta_bias, float* out, float* last_state, float* x_chunks, int batch, int dim, int delta_dim,
                                  int seqlen, int dstate, int ngroups, int delta_softplus, void* stream) {
    XP_CHECK_ARG(u && delta && A && Bm && Cm && out, "xp_selective_scan_fwd: null tensor pointer");
    XP_CHECK_ARG(batch > 0 && dim > 0 && seqlen > 0, "xp_selective_scan_fwd: batch/dim/seqlen must be positive");
    XP_CHECK_ARG(dstate > 0 && dstate <= 256, "xp_selective_scan_fwd: dstate must be in [1,256] (got %d)", dstate);
    XP_CHECK_ARG(ngroups > 0 && dim % ngroups == 0, "xp_selective_scan_fwd: dim %% ngroups != 0");
    XP_CHECK_ARG(delta_dim > 0 && dim % delta_dim == 0, "xp_selective_scan_fwd: dim %% delta_dim != 0");
    const int64_t rows = (int64_t)batch * dim;
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (seqlen % 4 == 0) && ((((uintptr_t)u | (uintptr_t)delta | (uintptr_t)Bm | (uintptr_t)Cm | (uintptr_t)out) & 15) == 0);
    // d_state = 1: both kernels are VALU-co-limited (52 VALU + 4 transcendentals per element, 70 % VALU-busy at 4.5 TB/s); the 8-item
    // DPP-scan kernel wins where few rows leave the SIMDs under-occupied (long rows, small batch: 3.9 vs 3.3 TB/s at 1536 rows x 65536),
    // the 4-item kernel where >= 3 waves per SIMD hide its LDS-crossbar scan (XP_SCAN_V1 / XP_SCAN_V2 force one for A/B runs).
    // The two kernels associate the scan differently and so differ in the last bits: the choice is made from seqlen only, never from batch * dim,
    // so a row's output does not depend on the other rows of the call (tests/test_gpu_batch_invariance.py).
    static const bool v1 = getenv("XP_SCAN_V1") != nullptr, v2 = getenv("XP_SCAN_V2") != nullptr;
    const bool use_v2 = v2 || (!v1 && seqlen >= kScanV2MinLen);
    static const bool old_gen = getenv("XP_SCAN_OLD_GEN") != nullptr;
    XP_CHECK_ARG(!(x_chunks && old_gen && dstate > 1), "xp_selective_scan_fwd_x: XP_SCAN_OLD_GEN has no chunk-state output");
    // one profiling tag per kernel, so a test can tell which one ran
    const char* tag = dstate == 1 ? (!vec ? "selective_scan_fwd_n1s" : use_v2 ? "selective_scan_fwd_n1v2" : "selective_scan_fwd_n1")
                                  : (old_gen ? "selective_scan_fwd_old" : "selective_scan_fwd_gen");
    XpProfScope prof(tag, s, (9.0 * dstate + 1.0) * batch * dim * (double)seqlen,
                     12.0 * batch * dim * (double)seqlen + 8.0 * batch * ngroups * dstate * (double)seqlen);
    if (dstate == 1) {
        if (vec && use_v2)
            hipLaunchKernelGGL(selective_scan_fwd_n1v2_kernel, grid, block, 0, s, u, delta, A, Bm, Cm, Dv, delta_bias, out, last_state, x_chunks,
                               batch, dim, delta_dim, seqlen, ngroups, delta_softplus);
        else if (vec)
            hipLaunchKernelGGL(selective_scan_fwd_n1_kernel<true>, grid, block, 0, s, u, delta, A, Bm, Cm, Dv, delta_bias, out, last_state, x_chunks,
                               batch, dim, delta_dim, seqlen, ngroups, delta_softplus);
        else
            hipLaunchKernelGGL(selective_scan_fwd_n1_kernel<false>, grid, block, 0, s, u, delta, A, Bm, Cm, Dv, delta_bias, out, last_state, x_chunks,
                               batch, dim, delta_dim, seqlen, ngroups, delta_softplus);
    } else {
        // d_state > 1: the 8-item DPP-scan kernel (the 4-item shuffle-scan kernel above ran at 0.08 of HBM at N = 16)
        if (!old_gen) launch_gen<float, float, true>(u, delta, A, Bm, Cm, Dv, delta_bias, out, last_state, x_chunks, batch, dim, delta_dim, seqlen, dstate, ngroups, delta_softplus, s);
        else if (vec)
            hipLaunchKernelGGL(selective_scan_fwd_kernel<true>, grid, block, 0, s, u, delta, A, Bm, Cm, Dv, delta_bias, out,
                               last_state, batch, dim, delta_dim, seqlen, dstate, ngroups, delta_softplus);
        else
            hipLaunchKernelGGL(selective_scan_fwd_kernel<false>, grid, block, 0, s, u, delta, A, Bm, Cm, Dv, delta_bias, out,
                               last_state, batch, dim, delta_dim, seqlen, dstate, ngroups, delta_softplus);
    }
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_selective_scan_fwd(const float* u, const float* delta, const float* A, const float* Bm,
                                     const float* Cm, const float* Dv, const float* delta_bias, float* out,
                                     float* last_state, int batch, int dim, int delta_dim, int seqlen, int dstate,
                                     int ngroups, int delta_softplus, void* stream) {
    return selective_scan_fwd_f32(u, delta, A, Bm, Cm, Dv, delta_bias, out, last_state, nullptr, batch, dim, delta_dim, seqlen, dstate, ngroups,
                                  delta_softplus, stream);
}

extern "C" int xp_selective_scan_fwd_x(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm, const float* Dv,
                                       const float* delta_bias, float* out, float* last_state, float* x_chunks, int batch, int dim, int delta_dim,
                                       int seqlen, int dstate, int ngroups, int delta_softplus, void* stream) {
    XP_CHECK_ARG(x_chunks, "xp_selective_scan_fwd_x: null x_chunks");
    return selective_scan_fwd_f32(u, delta, A, Bm, Cm, Dv, delta_bias, out, last_state, x_chunks, batch, dim, delta_dim, seqlen, dstate, ngroups,
                                  delta_softplus, stream);
}

// itype: 0 f32, 1 f16, 2 bf16 (u, delta, B, C); out_float != 0: out is f32 ("oflex"), else out has the input type.
extern "C" int xp_selective_scan_fwd_typed(const void* u, const void* delta, const float* A, const void* Bm, const void* Cm, const float* Dv,
                                           const float* delta_bias, void* out, float* x_chunks, int itype, int out_float, int batch, int dim,
                                           int delta_dim, int seqlen, int dstate, int ngroups, int delta_softplus, void* stream) {
    XP_CHECK_ARG(u && delta && A && Bm && Cm && out, "xp_selective_scan_fwd_typed: null tensor pointer");
    XP_CHECK_ARG(itype >= 0 && itype <= 2, "xp_selective_scan_fwd_typed: itype 0 (f32), 1 (f16) or 2 (bf16)");
    XP_CHECK_ARG(batch > 0 && dim > 0 && seqlen > 0, "xp_selective_scan_fwd_typed: batch/dim/seqlen must be positive");
    XP_CHECK_ARG(dstate > 0 && dstate <= 256, "xp_selective_scan_fwd_typed: dstate must be in [1,256] (got %d)", dstate);
    XP_CHECK_ARG(ngroups > 0 && dim % ngroups == 0, "xp_selective_scan_fwd_typed: dim %% ngroups != 0");
    XP_CHECK_ARG(delta_dim > 0 && dim % delta_dim == 0, "xp_selective_scan_fwd_typed: dim %% delta_dim != 0");
    hipStream_t s = (hipStream_t)stream;
    const double isz = itype == 0 ? 4.0 : 2.0, osz = (out_float || itype == 0) ? 4.0 : 2.0;
    XpProfScope prof(itype == 0 ? "selective_scan_fwd_gen_f32" : (itype == 1 ? "selective_scan_fwd_gen_f16" : "selective_scan_fwd_gen_bf16"), s,
                     (9.0 * dstate + 1.0) * batch * dim * (double)seqlen,
                     (2.0 * isz + osz) * batch * dim * (double)seqlen + 2.0 * isz * batch * ngroups * dstate * (double)seqlen);
#define XP_GEN(T, OT, EX) launch_gen<T, OT, EX>(u, delta, A, Bm, Cm, Dv, delta_bias, out, nullptr, x_chunks, batch, dim, delta_dim, seqlen, dstate, ngroups, delta_softplus, s)
    if (itype == 0) XP_GEN(float, float, true);
    else if (itype == 1) { if (out_float) XP_GEN(_Float16, float, false); else XP_GEN(_Float16, _Float16, false); }
    else { if (out_float) XP_GEN(__bf16, float, false); else XP_GEN(__bf16, __bf16, false); }
#undef XP_GEN
    XP_LAUNCH_CHECK();
    return XP_OK;
}
