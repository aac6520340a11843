// INPUT gradients of the 3x3 convolutions that training differentiates, each an implicit GEMM on the split-fp16 engines of
// gemm_h2_core.h over a weight that is rearranged and split once per call: the zero-padded stride-1 convolution (the RegNet head; the forward engine on the
// rotated weight), the zero-padded STRIDE-2 convolution (patch embed, the downsamplers; four parity classes, in the tile-engine and the row-stationary form),
// and the REFLECTION-padded stride-1 convolution (the head trunk; the zero-padded gradient plus a thin frame GEMM and a fold).  The weight gradients of the
// same convolutions reduce over rows and are in train_dense.hip.
//
// dy is the gradient operand: the engines read S x dy with {S, 1 / S} one power of two per call (train_scale.h) — the caller's pair (dy_scale), or the
// call's own, taken from the largest magnitude of dy, with a scaled copy in the workspace — and 1 / S is undone, exactly, in the epilogue.  No atomics
// anywhere: two calls are bit-identical.
#include "gemm_h2_core.h"
#include "train_scale.h"
#include "xpoint_hip.h"

namespace {

// ---- host side shared by the three families ----
// A workspace handed out front to back in 256-byte steps.  Over a null base it only measures: every family carves its regions in the one function that also
// launches its kernels, and the *_workspace_bytes query runs that function without a workspace, so the query and the entry point cannot disagree.
struct WsCursor {
    char* base;
    size_t used = 0;
    template <class T> T* take(size_t bytes) { T* p = base ? (T*)(base + used) : nullptr; used += xp_up256(bytes); return p; }
    bool measuring() const { return !base; }
};

// the refusals the entry points share, in the order they are made; `need` is the family's workspace query (0 for a refused shape: not reached)
static int td_dgrad_check(const char* who, bool pointers, bool shape_ok, const char* shape_note, bool dy_aligned, int batch, int H, int W, int Ci, int Co,
                          const void* ws, size_t ws_bytes, size_t need) {
    XP_CHECK_ARG(pointers, "%s: null pointer", who);
    XP_CHECK_ARG(shape_ok, "%s: bad shape batch=%d H=%d W=%d Ci=%d Co=%d%s", who, batch, H, W, Ci, Co, shape_note);
    XP_CHECK_ARG(Co % 4 == 0, "%s: Co must be a multiple of 4 (got %d): the engine loads dy in 4-element channel groups", who, Co);
    XP_CHECK_ARG(dy_aligned, "%s: dy must be 16-byte aligned", who);
    XP_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0 && ws_bytes >= need, "%s: workspace of %zu bytes, 256-byte aligned, needed (got %zu)", who, need, ws_bytes);
    return XP_OK;
}

// What the engines read: S x dy and {S, 1 / S}.  The caller's dy and pair as they are, or (dy_scale NULL) S from the largest magnitude of dy and the scaled
// copy, both in the workspace: its head and a (rows, Co) copy are set aside either way (the query does not know which call follows).
struct ScaledDy { const float* dy; const float2* scale; };
static int td_scaled_dy(WsCursor& ws, const float* dy, const float* dy_scale, int64_t rows, int Co, hipStream_t s, ScaledDy& g) {
    float* parts = ws.take<float>(XP_SCALE_HEAD_BYTES);
    float* dys = ws.take<float>((size_t)rows * Co * sizeof(float));
    g = ScaledDy{dy, (const float2*)dy_scale};
    if (ws.measuring() || dy_scale) return XP_OK;
    g = ScaledDy{dys, xp_head_scale(parts)};
    return xp_own_scale(dy, xp_walk_rows(rows, Co, Co), parts, xp_head_scale(parts), XP_SCALE_COPY, dys, s);
}

// Epilogue of the GEMMs over a K-slice of a rearranged weight: out = accumulator x the weight row's power of two x 1 / S, both exact, into the output row
// that row_ptr gives for row m of the GEMM (rows past Mc are not stored, columns past N neither)
template <class T, int TN, class RowPtr>
__device__ __forceinline__ void td_sliced_store(const f32x16 (&acc)[1][TN], int m0, int n0, int Mc, int N, const float* wscale, const float2* scale,
                                                RowPtr row_ptr) {
    const float inv_s = scale->y;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + T::row_of(0, r);
        if (m >= Mc) continue;
        float* row = row_ptr(m);
#pragma unroll
        for (int jn = 0; jn < TN; ++jn) {
            const int n = n0 + T::col_of(jn);
            if (n < N) row[n] = acc[0][jn][r] * wscale[n] * inv_s;
        }
    }
}

// ---- the zero-padded 3x3 convolution of the RegNet head (RegNet.py:13-18) ----
// wr[ci][ky][kx][co] = w[co][2 - ky][2 - kx][ci]: the weight whose FORWARD zero-pad convolution of dy is the input gradient
__global__ __launch_bounds__(256) void td_rot_weights_kernel(const float* __restrict__ w, float* __restrict__ wr, int Ci, int Co) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Ci * 9 * Co) return;
    const int co = idx % Co, tap = (idx / Co) % 9, ci = idx / (9 * Co);
    wr[idx] = w[((int64_t)co * 9 + (8 - tap)) * Ci + ci];
}
// the epilogue's affine of the input gradient: scale[c] = 1 / S, shift[c] = 0
__global__ __launch_bounds__(256) void td_unscale_vec_kernel(const float2* __restrict__ s, float* __restrict__ scale, float* __restrict__ shift, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) { scale[c] = s->y; shift[c] = 0.f; }
}

// dx = conv3x3(zero_pad(S dy), wrot) / S on the forward's implicit-GEMM engine, from an already scaled dy: no atomics, the engine's fixed summation order.
// The body of the zero-padded input gradient and the interior term of the reflection-padded one.
static int td_zp_dgrad(WsCursor& ws, const ScaledDy& g, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, void* stream) {
    float* vscale = ws.take<float>((size_t)2 * Ci * sizeof(float));          // the epilogue's affine: Ci scales, then Ci shifts
    float* wrot = ws.take<float>((size_t)9 * Ci * Co * sizeof(float));
    void* wsplit = ws.take<char>(xp_split_weights_h2_bytes(Ci, 9 * Co));
    if (ws.measuring()) return XP_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(td_unscale_vec_kernel, dim3(xp_cdiv(Ci, 256)), dim3(256), 0, s, g.scale, vscale, vscale + Ci, Ci);
    XP_LAUNCH_CHECK();
    hipLaunchKernelGGL(td_rot_weights_kernel, dim3(xp_cdiv(9 * Ci * Co, 256)), dim3(256), 0, s, w, wrot, Ci, Co);
    XP_LAUNCH_CHECK();
    XP_TRY(xp_split_weights_h2(wrot, wsplit, Ci, 9 * Co, stream));
    return xp_conv3x3_nhwc_h2(g.dy, wsplit, dx, nullptr, vscale, vscale + Ci, batch, H, W, Co, Ci, 1, 0, 0, stream);
}

static int td_zp(WsCursor& ws, const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale, void* stream) {
    ScaledDy g;
    XP_TRY(td_scaled_dy(ws, dy, dy_scale, (int64_t)batch * H * W, Co, (hipStream_t)stream, g));
    return td_zp_dgrad(ws, g, w, dx, batch, H, W, Ci, Co, stream);
}

// ---- the zero-padded STRIDE-2 3x3 convolution of patch embed and the downsamplers (VMamba.py:1405-1440) ----
// dx pixel (y, x) receives tap (ky, kx) only when y + 1 - ky and x + 1 - kx are even, from dy at ((y + 1 - ky) / 2, (x + 1 - kx) / 2):
// the pixels fall into four classes by the parity (py, px) of (y, x) with (1 + py)(1 + px) = 1, 2, 2, 4 taps — ky = 1 for an even y, ky = 0 (dy row
// i + 1) and ky = 2 (dy row i) for the odd y = 2 i + 1, the same along x.  Each class is an implicit GEMM of its own on the split-fp16 engine:
// M = its pixels, N = Ci, K = taps Co, the A row of a pixel gathered from dy tap by tap, the weight a K-slice of ONE rearranged (Ci, Ktot) matrix that
// is split once per call (every class's slice padded to whole 32-wide slabs).  No zero-stuffed dy, no products with structural zeros.
struct S2Class { int py, px, Hc, Wc, taps, slab0, nslab; };
static S2Class td_s2_class(int c, int H, int W, int Co) {
    S2Class k{};
    k.py = c >> 1; k.px = c & 1;
    k.Hc = (H + 1 - k.py) / 2; k.Wc = (W + 1 - k.px) / 2;
    k.taps = (1 + k.py) * (1 + k.px);
    for (int q = 0; q <= c; ++q) {
        const int n = xp_cdiv((1 + (q >> 1)) * (1 + (q & 1)) * Co, H2_BK);
        if (q < c) k.slab0 += n; else k.nslab = n;
    }
    return k;
}
static int td_s2_ktot(int Co) { const S2Class k = td_s2_class(3, 1, 1, Co); return (k.slab0 + k.nslab) * H2_BK; }

// wc[ci][32 slab0(c) + (ty nx + tx) Co + co] = w[co][ky][kx][ci], ky = py ? 2 ty : 1, kx = px ? 2 tx : 1; zeros in the pad of every slice
__global__ __launch_bounds__(256) void td_s2_weights_kernel(const float* __restrict__ w, float* __restrict__ wc, int Ci, int Co, int Ktot) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Ci * Ktot) return;
    const int ci = idx / Ktot;
    int k = idx - ci * Ktot;
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int py = c >> 1, px = c & 1, taps = (1 + py) * (1 + px), span = (taps * Co + H2_BK - 1) / H2_BK * H2_BK;
        if (k >= 0 && k < taps * Co) {
            const int tap = k / Co, co = k - tap * Co;
            const int ty = px ? tap >> 1 : tap, tx = px ? tap & 1 : 0;
            v = w[((int64_t)co * 9 + (py ? 2 * ty : 1) * 3 + (px ? 2 * tx : 1)) * Ci + ci];
        }
        k = k < 0 ? k : (k < span ? -1 : k - span);          // consumed by this class, or moved on to the next
    }
    wc[idx] = v;
}

struct S2DgParams {
    const float* dy;         // S x the gradient, (batch, Ho, Wo, Co)
    const uint4* wsplit;     // xp_split_weights_h2 of wc (Ci, Ktot)
    const float* wscale;     // its Ci inverse row scales
    const float2* scale;     // {S, 1 / S}
    float* dx;               // (batch, H, W, Ci)
    int batch, H, W, Ci, Co, Ho, Wo;
    int slab0[4];            // first slab of class c's K-slice
};

template <int TN>
__global__ __launch_bounds__(256) void td_s2_dgrad_kernel(const S2DgParams p) {
    using T = GemmTileH2<2, 2, 1, TN>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[T::kLdsBytes];
    const int cls = blockIdx.z, py = cls >> 1, px = cls & 1;
    const int Hc = (p.H + 1 - py) / 2, Wc = (p.W + 1 - px) / 2;
    const int Mc = p.batch * Hc * Wc, Kc = (1 + py) * (1 + px) * p.Co;
    const int m0 = blockIdx.x * T::BM, n0 = blockIdx.y * T::BN;
    if (m0 >= Mc) return;                          // block-uniform, before any barrier: this class has fewer row tiles (or no pixel at all)

    const float* a_ptr[T::A_LD];
    int a_i[T::A_LD], a_j[T::A_LD], a_tap[T::A_LD], a_co[T::A_LD];
#pragma unroll
    for (int s = 0; s < T::A_LD; ++s) {
        const int m = m0 + T::a_row(s);
        const int mc = m < Mc ? m : 0;           // rows past Mc only feed output rows that are never stored
        const int b = mc / (Hc * Wc), rr = mc - b * (Hc * Wc);
        a_i[s] = rr / Wc; a_j[s] = rr - a_i[s] * Wc;
        a_ptr[s] = p.dy + (int64_t)b * p.Ho * p.Wo * p.Co;
        const int k = T::a_quad(s) * 4;          // (tap, co) advance by one slab per call: no division in the K loop
        a_tap[s] = k / p.Co; a_co[s] = k - a_tap[s] * p.Co;
    }
    const H2WeightSlice<T> ldB(p.wsplit, p.Ci, n0, p.slab0[cls], (Kc + H2_BK - 1) / H2_BK);
    auto ldA = [&](int s, int k, float4& v) -> bool {
        bool ok = k < Kc;
        int tap = a_tap[s], co = a_co[s];
        if (!ok) { tap = 0; co = 0; }
        a_co[s] += H2_BK;                                  // Co >= 4: at most eight wraps per 32-wide slab, as selects
#pragma unroll
        for (int w = 0; w < 8; ++w) { const bool wrap = a_co[s] >= p.Co; a_co[s] -= wrap ? p.Co : 0; a_tap[s] += wrap ? 1 : 0; }
        const int ty = px ? tap >> 1 : tap, tx = px ? tap & 1 : 0;
        int yo = a_i[s] + ((py && ty == 0) ? 1 : 0), xo = a_j[s] + ((px && tx == 0) ? 1 : 0);      // never negative
        ok = ok && yo < p.Ho && xo < p.Wo;
        yo = yo < p.Ho ? yo : p.Ho - 1; xo = xo < p.Wo ? xo : p.Wo - 1;      // a valid address: the load is unconditional, the slot is staged as zeros
        v = *reinterpret_cast<const float4*>(a_ptr[s] + ((int64_t)yo * p.Wo + xo) * p.Co + co);
        return ok;
    };

    f32x16 acc[1][TN];
    T::run(lds, Kc, ldA, ldB, acc);

    // row m of class (py, px) is dx pixel (2 i + py, 2 j + px) of sample b
    td_sliced_store<T, TN>(acc, m0, n0, Mc, p.Ci, p.wscale, p.scale, [&](int m) {
        const int b = m / (Hc * Wc), rr = m - b * (Hc * Wc), i = rr / Wc, j = rr - i * Wc;
        return p.dx + (((int64_t)b * p.H + 2 * i + py) * p.W + 2 * j + px) * p.Ci;
    });
}

// The same GEMMs on the row-stationary engine (GemmTileH2R: every lane loads its own row's fragment straight from global memory, only the weights go
// through the LDS), for Co % 16 == 0 and a dy below 2 GB: a 16-wide k-step then lies inside ONE tap, the same for the whole wave, so (tap, co) advance as
// scalars and the lane's geometry — which dy pixel the tap reads, whether it exists — is worked out once per tap, at most four times per launch, as a
// 32-bit byte offset into a buffer resource over dy; a tap outside dy and a k-step past the class's K carry an offset beyond its end and the hardware
// returns zeros (the scheme of gemm_h2r_kernel's convolution form).  Same values in the same order as the tile-engine form above: the same bits.
template <int TN>
__global__ __launch_bounds__(256) void td_s2_dgrad_r_kernel(const S2DgParams p) {
    using T = GemmTileH2R<TN>;
    extern __shared__ __align__(16) unsigned char lds[];
    const int cls = blockIdx.z, py = cls >> 1, px = cls & 1;
    const int Hc = (p.H + 1 - py) / 2, Wc = (p.W + 1 - px) / 2;
    const int Mc = p.batch * Hc * Wc, taps = (1 + py) * (1 + px), Kc = taps * p.Co;
    const int m0 = blockIdx.x * T::BM, n0 = blockIdx.y * T::BN;
    if (m0 >= Mc) return;                          // block-uniform, before any barrier

    const int fh = (threadIdx.x & 63) >> 5;
    const int m = m0 + T::a_row();
    const int mc = m < Mc ? m : 0;               // rows past Mc only feed output rows that are never stored
    const int b = mc / (Hc * Wc), rr = mc - b * (Hc * Wc), ai = rr / Wc, aj = rr - ai * Wc;
    const H2WeightSlice<T> ldB(p.wsplit, p.Ci, n0, p.slab0[cls], (Kc + H2_BK - 1) / H2_BK);

    constexpr unsigned kPastEnd = 0x80000000u;                 // >= the bytes of dy (the host checks), and no 32-bit wrap when the channel offset is added
    const unsigned dy_bytes = (unsigned)p.batch * p.Ho * p.Wo * p.Co * 4u;
    const unsigned lane_base = (unsigned)b * p.Ho * p.Wo * p.Co * 4u + (unsigned)fh * 32u;       // the lane's sample and its half of the k-step
    auto tap_offset = [&](int tap) -> unsigned {
        if (tap >= taps) return kPastEnd;
        const int ty = px ? tap >> 1 : tap, tx = px ? tap & 1 : 0;
        const int yo = ai + ((py && ty == 0) ? 1 : 0), xo = aj + ((px && tx == 0) ? 1 : 0);      // never negative
        return (yo < p.Ho && xo < p.Wo) ? lane_base + (unsigned)((yo * p.Wo + xo) * p.Co) * 4u : kPastEnd;
    };
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, 0, (int)dy_bytes, 0x00020000);
    int tap = 0, co4 = 0;                                       // of the next k-step: wave-uniform (co4 = byte offset of its first channel)
    unsigned cur = tap_offset(0);
    typedef unsigned raw4 __attribute__((ext_vector_type(4)));
    auto ldA8 = [&](int, float4& lo, float4& hi) -> bool {
        const raw4 a = __builtin_bit_cast(raw4, __builtin_amdgcn_raw_buffer_load_b128(rs, cur, co4, 0));
        const raw4 c = __builtin_bit_cast(raw4, __builtin_amdgcn_raw_buffer_load_b128(rs, cur + 16, co4, 0));
        lo = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w));
        hi = make_float4(__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z), __uint_as_float(c.w));
        co4 += 64;
        if (co4 == p.Co * 4) { co4 = 0; ++tap; cur = tap_offset(tap); }
        return true;
    };
    f32x16 acc[1][TN];
    T::template run<false>(lds, Kc, ldA8, ldB, acc);

    // row m of class (py, px) is dx pixel (2 i + py, 2 j + px) of sample b
    td_sliced_store<T, TN>(acc, m0, n0, Mc, p.Ci, p.wscale, p.scale, [&](int m) {
        const int b = m / (Hc * Wc), rr = m - b * (Hc * Wc), i = rr / Wc, j = rr - i * Wc;
        return p.dx + (((int64_t)b * p.H + 2 * i + py) * p.W + 2 * j + px) * p.Ci;
    });
}

template <int TN>
static int td_s2_dgrad_r_launch(const S2DgParams& p, int64_t m_even, hipStream_t s) {
    using T = GemmTileH2R<TN>;
    hipLaunchKernelGGL(td_s2_dgrad_r_kernel<TN>, dim3((unsigned)xp_cdiv(m_even, (int64_t)T::BM), xp_cdiv(p.Ci, T::BN), 4), dim3(256), T::kLdsBytes, s, p);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

template <int TN>
static int td_s2_dgrad_launch(const S2DgParams& p, int64_t m_even, hipStream_t s) {
    using T = GemmTileH2<2, 2, 1, TN>;
    hipLaunchKernelGGL(td_s2_dgrad_kernel<TN>, dim3((unsigned)xp_cdiv(m_even, (int64_t)T::BM), xp_cdiv(p.Ci, T::BN), 4), dim3(256), 0, s, p);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

static int td_s2(WsCursor& ws, const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, Ktot = td_s2_ktot(Co);
    const int64_t rows = (int64_t)batch * Ho * Wo;
    ScaledDy g;
    XP_TRY(td_scaled_dy(ws, dy, dy_scale, rows, Co, s, g));
    float* wc = ws.take<float>((size_t)Ci * Ktot * sizeof(float));
    void* wsplit = ws.take<char>(xp_split_weights_h2_bytes(Ci, Ktot));
    if (ws.measuring()) return XP_OK;
    hipLaunchKernelGGL(td_s2_weights_kernel, dim3(xp_cdiv(Ci * Ktot, 256)), dim3(256), 0, s, w, wc, Ci, Co, Ktot);
    XP_LAUNCH_CHECK();
    XP_TRY(xp_split_weights_h2(wc, wsplit, Ci, Ktot, stream));
    S2DgParams p{};
    p.dy = g.dy; p.wsplit = (const uint4*)wsplit; p.wscale = h2_scales(wsplit, Ci, Ktot); p.scale = g.scale; p.dx = dx;
    p.batch = batch; p.H = H; p.W = W; p.Ci = Ci; p.Co = Co; p.Ho = Ho; p.Wo = Wo;
    for (int c = 0; c < 4; ++c) p.slab0[c] = td_s2_class(c, H, W, Co).slab0;
    const int64_t m_even = (int64_t)batch * ((H + 1) / 2) * ((W + 1) / 2);        // the largest class
    XpProfScope prof("conv3x3_s2_dgrad_h2", s, 6.0 * rows * 9.0 * Ci * Co, 4.0 * (rows * Co + (double)batch * H * W * Ci));
    // Row-stationary form where a k-step lies inside one tap and 32-bit offsets reach all of dy; the tile-engine form otherwise.  Both walk K in the same
    // order, so the choice never changes a result bit (measured at the three downsampler shapes, batch 16: 40 / 42 / 68 us against 65 / 58 / 87 us).
    if (Co % 16 == 0 && rows * Co * 4 < ((int64_t)1 << 31)) {
        if (Ci <= 32) return td_s2_dgrad_r_launch<1>(p, m_even, s);
        if (Ci <= 64) return td_s2_dgrad_r_launch<2>(p, m_even, s);
        if (Ci <= 96 || Ci % 96 == 0) return td_s2_dgrad_r_launch<3>(p, m_even, s);          // 96, 192, 384: no column of the tile is wasted
        return td_s2_dgrad_r_launch<4>(p, m_even, s);
    }
    return Ci <= 64 ? td_s2_dgrad_launch<1>(p, m_even, s) : td_s2_dgrad_launch<2>(p, m_even, s);
}

// ---- the REFLECTION-padded 3x3 convolution of the head trunk (XPoint.py:112-138): input gradient ----
// With g the zero-padded input gradient on the PADDED frame (rows -1 .. H, columns -1 .. W; g[v][u] = sum_k w[k]^T dy[v - ky + 1][u - kx + 1], taps
// outside dy absent), reflection folds the frame back: dx[y][x] = sum of g[v][u] over v in {y} + {-1 if y == 1} + {H if y == H - 2} and u likewise.
// The interior term g[y][x] is the zero-padded input gradient (td_zp_dgrad) as it stands.  The frame — 2 (W + 2) + 2 H pixels per image — is a thin implicit GEMM of
// its own in four classes (top row v = -1: only ky = 0, from dy row 0; bottom row v = H: only ky = 2, from dy row H - 1; left column u = -1: only kx = 0;
// right column u = W: only kx = 2), each cut by its three taps along the line: twelve GEMMs with M = the class's frame pixels, N = Ci, K = Co over
// their slice of ONE rearranged weight that is split once per call (every slice padded to whole 32-wide slabs), the scheme of the stride-2 input
// gradient above.  The cut by tap keeps the reduction short — the frame has few rows, so one workgroup per (row tile, class) walking K = 3 Co alone
// would be a long serial loop on a few CUs — and the three partial results go to three planes that the last kernel adds in tap order, together with
// the fold: it adds the frame terms to the at most 2 (H + W) - 4 pixels of rows / columns 1 and n - 2 in a fixed order.  No (H + 2) x (W + 2) copy
// of dy or dx, no atomics.
static int td_rp_span(int Co) { return xp_cdiv(Co, H2_BK) * H2_BK; }          // K of one (class, tap) slice
static int td_rp_frame(int H, int W) { return 2 * (W + 2) + 2 * H; }          // per image: top (W + 2), bottom (W + 2), left (H), right (H)

// wf[ci][span (3 cls + t) + co] = w[co][ky][kx][ci]: cls 0 (ky, kx) = (0, t), 1: (2, t), 2: (t, 0), 3: (t, 2); zeros in the pad of every slice
__global__ __launch_bounds__(256) void td_rp_weights_kernel(const float* __restrict__ w, float* __restrict__ wf, int Ci, int Co, int span) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Ci * 12 * span) return;
    const int ci = idx / (12 * span), rem = idx - ci * 12 * span, slice = rem / span, co = rem - slice * span;
    float v = 0.f;
    if (co < Co) {
        const int cls = slice / 3, t = slice - 3 * cls;
        const int ky = cls == 0 ? 0 : (cls == 1 ? 2 : t), kx = cls == 2 ? 0 : (cls == 3 ? 2 : t);
        v = w[((int64_t)co * 9 + ky * 3 + kx) * Ci + ci];
    }
    wf[idx] = v;
}

struct RpDgParams {
    const float* dy;         // S x the gradient, (batch, H, W, Co)
    const uint4* wsplit;     // xp_split_weights_h2 of wf (Ci, 12 span)
    const float* wscale;     // its Ci inverse row scales
    const float2* scale;     // {S, 1 / S}
    float* gf;               // (3, batch, frame, Ci): the unscaled g on the frame, one plane per tap
    float* dx;               // (batch, H, W, Ci): holds the interior term, receives the frame terms
    int batch, H, W, Ci, Co;
    int slabs;               // slabs per (class, tap) slice
};

// Row m of class cls is frame pixel i of sample b: i = u + 1 along the top / bottom row, i = v along the left / right column.  Tap t reads the dy
// pixel at line position i - t (rows: the column u - kx + 1) or i - t + 1 (columns: the row v - ky + 1) of dy's first / last row or column.
template <int TN>
__global__ __launch_bounds__(256) void td_rp_frame_kernel(const RpDgParams p) {
    using T = GemmTileH2<2, 2, 1, TN>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[T::kLdsBytes];
    const int cls = blockIdx.z / 3, tap = blockIdx.z - 3 * cls;
    const bool horiz = cls < 2;
    const int Lc = horiz ? p.W + 2 : p.H, n_line = horiz ? p.W : p.H;
    const int Mc = p.batch * Lc, Kc = p.Co;
    const int m0 = blockIdx.x * T::BM, n0 = blockIdx.y * T::BN;
    if (m0 >= Mc) return;                          // block-uniform, before any barrier: this class has fewer row tiles
    // dy pixel of line position j: pix0 + j * step
    const int pix0 = cls == 1 ? (p.H - 1) * p.W : (cls == 3 ? p.W - 1 : 0), step = horiz ? 1 : p.W, shift = horiz ? 0 : 1;

    const float* a_ptr[T::A_LD];
    bool a_ok[T::A_LD];
#pragma unroll
    for (int s = 0; s < T::A_LD; ++s) {
        const int m = m0 + T::a_row(s);
        const int mc = m < Mc ? m : 0;           // rows past Mc only feed output rows that are never stored
        const int b = mc / Lc;
        int j = mc - b * Lc + shift - tap;      // the line position this row's tap reads: fixed for the whole K loop
        a_ok[s] = j >= 0 && j < n_line;
        j = j < 0 ? 0 : (j < n_line ? j : n_line - 1);     // a valid address: the load is unconditional, the slot is staged as zeros
        a_ptr[s] = p.dy + ((int64_t)b * p.H * p.W + pix0 + (int64_t)j * step) * p.Co;
    }
    const H2WeightSlice<T> ldB(p.wsplit, p.Ci, n0, (int)blockIdx.z * p.slabs, (Kc + H2_BK - 1) / H2_BK);
    auto ldA = [&](int s, int k, float4& v) -> bool {
        const bool ok = k < Kc;                            // k is the channel: a multiple of 4, so k < Co leaves four channels
        v = *reinterpret_cast<const float4*>(a_ptr[s] + (ok ? k : 0));
        return ok && a_ok[s];
    };

    f32x16 acc[1][TN];
    T::run(lds, Kc, ldA, ldB, acc);

    const int F = 2 * (p.W + 2) + 2 * p.H;
    const int off = cls == 0 ? 0 : (cls == 1 ? p.W + 2 : (cls == 2 ? 2 * (p.W + 2) : 2 * (p.W + 2) + p.H));
    float* const side = p.gf + ((int64_t)tap * p.batch * F + off) * p.Ci;          // the tap's plane: this side's first pixel of sample 0
    td_sliced_store<T, TN>(acc, m0, n0, Mc, p.Ci, p.wscale, p.scale, [&](int m) {
        const int b = m / Lc, i = m - b * Lc;
        return side + ((int64_t)b * F + i) * p.Ci;
    });
}

// dx[y][x] += the frame terms (each the sum of its three tap planes, in tap order), rows of the frame first (top, bottom: u = x, then -1, then W), then the columns (left, right) at v = y.  The pixels of
// rows 1 and H - 2 come first (nry W of them), then those of columns 1 and W - 2 in the remaining rows.
__global__ __launch_bounds__(256) void td_rp_fold_kernel(const RpDgParams p, int nry, int ry0, int ry1, int ncx, int cx0, int cx1, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int na = nry * p.W + (p.H - nry) * ncx;           // affected pixels per image
    const int c = (int)(idx % p.Ci);
    const int64_t pa = idx / p.Ci;
    const int b = (int)(pa / na), a = (int)(pa - (int64_t)b * na);
    int y, x;
    if (a < nry * p.W) { const int q = a / p.W; y = q ? ry1 : ry0; x = a - q * p.W; }
    else {
        const int r = a - nry * p.W, q = r / ncx;
        x = (r - q * ncx) ? cx1 : cx0;
        y = q; if (y >= ry0) ++y; if (nry == 2 && y >= ry1) ++y;
    }
    const int F = 2 * (p.W + 2) + 2 * p.H;
    const int64_t plane = (int64_t)p.batch * F * p.Ci;
    auto term = [&](const float* q) { return (q[0] + q[plane]) + q[2 * plane]; };
    const float* g = p.gf + (int64_t)b * F * p.Ci + c;
    const float* top = g, *bot = g + (int64_t)(p.W + 2) * p.Ci, *lef = g + (int64_t)2 * (p.W + 2) * p.Ci, *rig = lef + (int64_t)p.H * p.Ci;
    float* d = p.dx + (((int64_t)b * p.H + y) * p.W + x) * p.Ci + c;
    const bool xl = x == 1, xr = x == p.W - 2;
    float s = *d;
    if (y == 1) {
        s += term(top + (int64_t)(x + 1) * p.Ci);
        if (xl) s += term(top);
        if (xr) s += term(top + (int64_t)(p.W + 1) * p.Ci);
    }
    if (y == p.H - 2) {
        s += term(bot + (int64_t)(x + 1) * p.Ci);
        if (xl) s += term(bot);
        if (xr) s += term(bot + (int64_t)(p.W + 1) * p.Ci);
    }
    if (xl) s += term(lef + (int64_t)y * p.Ci);
    if (xr) s += term(rig + (int64_t)y * p.Ci);
    *d = s;
}

template <int TN>
static int td_rp_frame_launch(const RpDgParams& p, hipStream_t s) {
    using T = GemmTileH2<2, 2, 1, TN>;
    const int64_t m_max = (int64_t)p.batch * max(p.W + 2, p.H);
    hipLaunchKernelGGL(td_rp_frame_kernel<TN>, dim3((unsigned)xp_cdiv(m_max, (int64_t)T::BM), xp_cdiv(p.Ci, T::BN), 12), dim3(256), 0, s, p);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

static bool td_rp_shape_ok(int batch, int H, int W, int Ci, int Co) {
    // the limits of the zero-padded input gradient, reflection's two pixels, and the rearranged weight's 12 Ci pad32(Co) elements indexed as int
    return xp_conv_grad_shape_ok(batch, H, W, Ci, Co, 26) && H >= 2 && W >= 2 && (int64_t)12 * Ci * td_rp_span(Co) < ((int64_t)1 << 31);
}

static int td_rp(WsCursor& ws, const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int span = td_rp_span(Co), Ktot = 12 * span;
    const int64_t frame_rows = (int64_t)batch * td_rp_frame(H, W);
    ScaledDy g;
    XP_TRY(td_scaled_dy(ws, dy, dy_scale, (int64_t)batch * H * W, Co, s, g));
    XP_TRY(td_zp_dgrad(ws, g, w, dx, batch, H, W, Ci, Co, stream));          // the interior term g[y][x], from the same S x dy
    float* wf = ws.take<float>((size_t)Ci * Ktot * sizeof(float));
    void* wsplit = ws.take<char>(xp_split_weights_h2_bytes(Ci, Ktot));
    float* gf = ws.take<float>((size_t)3 * frame_rows * Ci * sizeof(float));
    if (ws.measuring()) return XP_OK;
    hipLaunchKernelGGL(td_rp_weights_kernel, dim3(xp_cdiv(Ci * Ktot, 256)), dim3(256), 0, s, w, wf, Ci, Co, span);
    XP_LAUNCH_CHECK();
    XP_TRY(xp_split_weights_h2(wf, wsplit, Ci, Ktot, stream));
    RpDgParams p{};
    p.dy = g.dy; p.wsplit = (const uint4*)wsplit; p.wscale = h2_scales(wsplit, Ci, Ktot); p.scale = g.scale;
    p.gf = gf; p.dx = dx;
    p.batch = batch; p.H = H; p.W = W; p.Ci = Ci; p.Co = Co; p.slabs = span / H2_BK;
    {
        XpProfScope prof("conv3x3_rp_dgrad_frame_h2", s, 6.0 * frame_rows * 3.0 * Ci * Co, 4.0 * frame_rows * (3.0 * Co + Ci));
        XP_TRY(Ci <= 64 ? td_rp_frame_launch<1>(p, s) : td_rp_frame_launch<2>(p, s));
    }
    // rows {1, H - 2} and columns {1, W - 2} as sets: H = 2 gives {0, 1} (H - 2 first does not matter: the order inside a pixel's sum is fixed), H = 3 {1}
    const int ry0 = min(1, H - 2), ry1 = max(1, H - 2), nry = ry0 == ry1 ? 1 : 2;
    const int cx0 = min(1, W - 2), cx1 = max(1, W - 2), ncx = cx0 == cx1 ? 1 : 2;
    const int64_t total = (int64_t)batch * (nry * W + (H - nry) * ncx) * Ci;
    XpProfScope prof("conv3x3_rp_dgrad_fold", s, 0.0, 16.0 * total);
    hipLaunchKernelGGL(td_rp_fold_kernel, dim3((unsigned)xp_cdiv(total, (int64_t)256)), dim3(256), 0, s, p, nry, ry0, ry1, ncx, cx0, cx1, total);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

}  // namespace

// Every family: the query measures with the function that runs (a null workspace), the entry point checks and runs it.
extern "C" size_t xp_conv3x3_dgrad_h2_workspace_bytes(int batch, int H, int W, int Ci, int Co) {
    if (!xp_conv_grad_shape_ok(batch, H, W, Ci, Co, 26)) return 0;
    WsCursor ws{nullptr};
    td_zp(ws, nullptr, nullptr, nullptr, batch, H, W, Ci, Co, nullptr, nullptr);
    return ws.used;
}

extern "C" int xp_conv3x3_dgrad_h2(const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    XP_TRY(td_dgrad_check("xp_conv3x3_dgrad_h2", dy && w && dx, xp_conv_grad_shape_ok(batch, H, W, Ci, Co, 26), "", true, batch, H, W, Ci, Co, workspace,
                          workspace_bytes, xp_conv3x3_dgrad_h2_workspace_bytes(batch, H, W, Ci, Co)));
    WsCursor ws{(char*)workspace};
    return td_zp(ws, dy, w, dx, batch, H, W, Ci, Co, dy_scale, stream);
}

extern "C" size_t xp_conv3x3_s2_dgrad_h2_workspace_bytes(int batch, int H, int W, int Ci, int Co) {
    if (!xp_conv_grad_shape_ok(batch, H, W, Ci, Co, 24)) return 0;
    WsCursor ws{nullptr};
    td_s2(ws, nullptr, nullptr, nullptr, batch, H, W, Ci, Co, nullptr, nullptr);
    return ws.used;
}

extern "C" int xp_conv3x3_s2_dgrad_h2(const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    XP_TRY(td_dgrad_check("xp_conv3x3_s2_dgrad_h2", dy && w && dx, xp_conv_grad_shape_ok(batch, H, W, Ci, Co, 24), "", ((uintptr_t)dy & 15) == 0, batch, H, W, Ci,
                          Co, workspace, workspace_bytes, xp_conv3x3_s2_dgrad_h2_workspace_bytes(batch, H, W, Ci, Co)));
    WsCursor ws{(char*)workspace};
    return td_s2(ws, dy, w, dx, batch, H, W, Ci, Co, dy_scale, stream);
}

extern "C" size_t xp_conv3x3_rp_dgrad_h2_workspace_bytes(int batch, int H, int W, int Ci, int Co) {
    if (!td_rp_shape_ok(batch, H, W, Ci, Co)) return 0;
    WsCursor ws{nullptr};
    td_rp(ws, nullptr, nullptr, nullptr, batch, H, W, Ci, Co, nullptr, nullptr);
    return ws.used;
}

extern "C" int xp_conv3x3_rp_dgrad_h2(const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    XP_TRY(td_dgrad_check("xp_conv3x3_rp_dgrad_h2", dy && w && dx, td_rp_shape_ok(batch, H, W, Ci, Co), " (reflection needs H, W >= 2)", ((uintptr_t)dy & 15) == 0,
                          batch, H, W, Ci, Co, workspace, workspace_bytes, xp_conv3x3_rp_dgrad_h2_workspace_bytes(batch, H, W, Ci, Co)));
    WsCursor ws{(char*)workspace};
    return td_rp(ws, dy, w, dx, batch, H, W, Ci, Co, dy_scale, stream);
}
