// Selective-scan backward at the reference operator boundary (drop-in for selective_scan_cuda_oflex.bwd:
// reference kernels/selective_scan/csrc/selective_scan/cusoflex/selective_scan_oflex.cpp:233-350).
//
// Forward (per batch b, channel d, state n; dl = softplus(delta + bias) or delta + bias):
//     a_l = exp(dl_l A_n),  h_l = a_l h_{l-1} + dl_l B_l u_l,  y_l = sum_n C_l h_l + D u_l.
// Backward with g_l = dL/dh_l = dy_l C_l + a_{l+1} g_{l+1}, carried leftwards as q_l = a_l g_l (q_l = a_l (q_{l+1} + dy_l C_l)):
//     dC_l += dy_l h_l,  dB_l += g_l dl_l u_l,  du_l = D dy_l + sum_n g_l dl_l B_l,  dA_n += sum_l g_l h_{l-1} a_l dl_l,
//     ddl_l = sum_n g_l (h_{l-1} a_l A_n + B_l u_l),  ddelta_l = ddl_l sigmoid(delta_l + bias) (softplus) or ddl_l,  dD += dy u,
//     ddelta_bias += ddelta.
//
// CDNA4 mapping.  One wave per (batch, channel) row, W waves per workgroup = W consecutive channels of ONE (batch, group), so that
// dB / dC (summed over the channels of a group) reduce across the waves in LDS in a fixed order and leave one f32 partial per
// workgroup in a slab; a second kernel sums the ceil(channels per group / W) partials in order and casts to B's dtype.  The row is
// walked backwards in the forward's 2048-element x chunks: pass F rebuilds, from the chunk's entering state x[.., c - 1, 2n + 1], the
// state entering each of its 512-element steps (8 items per lane, the (a, b) scan across the wave on DPP moves as in the forward);
// pass B walks the steps right to left, recomputes h inside the step and runs the reverse scan of q across the wave (shuffles).
// dA, dD and ddelta_bias are per-lane sums in a fixed order, a butterfly across the wave, one partial per row, and a batch-ordered sum
// in the reduce kernel.  No float atomics: two identical calls are bit-identical, and du / ddelta / dB / dC of a sample do not depend
// on the other samples of the call.
#include "xp_common.h"
#include "../../include/xpoint_hip.h"

namespace {

constexpr int kStep = 512;          // elements per wave step (8 per lane)
constexpr int kXChunk = 2048;       // the forward's x chunk (selective_scan_oflex.cpp:206)
constexpr int kSteps = kXChunk / kStep;

template <class T> struct BwdIO;
template <> struct BwdIO<float> {
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
template <class H> struct BwdIO16 {
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
template <> struct BwdIO<_Float16> : BwdIO16<_Float16> {};
template <> struct BwdIO<__bf16> : BwdIO16<__bf16> {};

template <class T>
__device__ __forceinline__ void ld8(const T* p, int off, int rem, int vec, float (&v)[8]) {
    if (vec && rem >= 8) BwdIO<T>::load8(p + off, v);
    else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = i < rem ? BwdIO<T>::get(p + off + i) : 0.f;
    }
}
template <class T>
__device__ __forceinline__ void st8(T* p, int off, int rem, int vec, const float (&v)[8]) {
    if (vec && rem >= 8) BwdIO<T>::store8(p + off, v);
    else {
#pragma unroll
        for (int i = 0; i < 8; ++i) if (i < rem) BwdIO<T>::put(p + off + i, v[i]);
    }
}

// inclusive scan of h -> a h + b maps over the wave, earlier lanes first (the forward's DPP scan, selective_scan.hip)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float bwd_dpp(float identity, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ void bwd_wave_scan_fwd(float& a, float& b) {
#define XP_SCAN_STEP(CTRL, MASK) { const float ea = bwd_dpp<CTRL, MASK>(1.f, a), eb = bwd_dpp<CTRL, MASK>(0.f, b); b = fmaf(a, eb, b); a = a * ea; }
    XP_SCAN_STEP(0x111, 0xf)      // row_shr:1
    XP_SCAN_STEP(0x112, 0xf)      // row_shr:2
    XP_SCAN_STEP(0x114, 0xf)      // row_shr:4
    XP_SCAN_STEP(0x118, 0xf)      // row_shr:8
    XP_SCAN_STEP(0x142, 0xa)      // row_bcast:15 into rows 1 and 3
    XP_SCAN_STEP(0x143, 0xc)      // row_bcast:31 into rows 2 and 3
#undef XP_SCAN_STEP
}
// inclusive scan of q -> a q + b maps over the wave, LATER lanes first: lane l ends with M_l o M_{l+1} o ... o M_63
__device__ __forceinline__ void bwd_wave_scan_rev(float& a, float& b, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float ua = __shfl_down(a, o, 64), ub = __shfl_down(b, o, 64);
        if (lane + o < 64) { b = fmaf(a, ub, b); a = a * ua; }
    }
}
__device__ __forceinline__ float bwd_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float bwd_lane0(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ float bwd_lane63(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }

struct BwdParams {
    const void* u; const void* delta; const float* A; const void* Bm; const void* Cm; const float* Dv; const float* delta_bias;
    const void* dout; const float* x;
    void* du; void* ddelta;              // du (batch, dim, L), ddelta (batch, delta_dim, L): input dtype
    float* ddelta_part;                  // (batch, dim, L) f32 when delta_dim < dim, else unused
    float* bc_part;                      // (2, batch, G, tiles, N, L) f32: per-workgroup dB / dC partials
    float* pA; float* pD; float* pdb;    // per-row partials: (batch, dim, N), (batch, dim), (batch, dim)
    int batch, dim, delta_dim, L, N, G, softplus, tiles, vec;
};

// delta of one step from the raw delta + bias (the forward's softplus; its derivative, the sigmoid, is applied in pass B)
__device__ __forceinline__ float bwd_delta(float t, int softplus) { return softplus ? xp_softplus_fast(t) : t; }

template <class T, class OT, int NFIX, int W>
__global__ __launch_bounds__(W * 64) void selective_scan_bwd_kernel(BwdParams p) {
    constexpr int NS = NFIX ? NFIX : 256;
    __shared__ float hsub[W][kSteps][NS];     // state entering each 512-step of the current x chunk
    __shared__ float gcar[W][NS];             // q carried in from the right
    __shared__ float accA[W][NS];             // dA partial of the row (general N)
    __shared__ float red[2][W][kStep];        // dB / dC of the wave's channel, reduced across the workgroup
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int N = NFIX ? NFIX : p.N, L = p.L, G = p.G, dim = p.dim;
    const int tile = blockIdx.x % p.tiles, bg = blockIdx.x / p.tiles, g = bg % G, b = bg / G;
    const int cpg = dim / G, cl = tile * W + wave;
    const bool valid = cl < cpg;
    const int d = g * cpg + (valid ? cl : 0);           // an idle wave reads a real row and writes nothing
    const int rep = dim / p.delta_dim, dd = d / rep;
    const int64_t row = (int64_t)b * dim + d;
    const T* up = static_cast<const T*>(p.u) + row * L;
    const T* dp = static_cast<const T*>(p.delta) + ((int64_t)b * p.delta_dim + dd) * L;
    const T* Bp = static_cast<const T*>(p.Bm) + ((int64_t)b * G + g) * N * L;
    const T* Cp = static_cast<const T*>(p.Cm) + ((int64_t)b * G + g) * N * L;
    const OT* yp = static_cast<const OT*>(p.dout) + row * L;
    const float* Ap = p.A + (int64_t)d * N;
    const float Dval = p.Dv ? p.Dv[d] : 0.f, bias = p.delta_bias ? p.delta_bias[dd] : 0.f;
    const int softplus = p.softplus, vec = p.vec;
    const int nxc = (L + kXChunk - 1) / kXChunk;
    float* bcB = p.bc_part + (((int64_t)b * G + g) * p.tiles + tile) * N * L;
    float* bcC = bcB + (int64_t)p.batch * G * p.tiles * N * L;
    for (int n = lane; n < N; n += 64) { gcar[wave][n] = 0.f; accA[wave][n] = 0.f; }
    float accA1 = 0.f, accD = 0.f, accDB = 0.f;

    for (int c = nxc - 1; c >= 0; --c) {
        const int c0 = c * kXChunk, clen = min(kXChunk, L - c0), nsub = (clen + kStep - 1) / kStep;
        // ---- pass F: the state entering every 512-step of the chunk
        for (int n = lane; n < N; n += 64) hsub[wave][0][n] = c > 0 ? p.x[((row * nxc + c - 1) * N + n) * 2 + 1] : 0.f;
        for (int s = 0; s + 1 < nsub; ++s) {
            const int off = c0 + s * kStep + lane * 8, rem = L - off;
            float uv[8], dl[8];
            ld8(up, off, rem, vec, uv); ld8(dp, off, rem, vec, dl);
#pragma unroll
            for (int i = 0; i < 8; ++i) { dl[i] = bwd_delta(dl[i] + bias, softplus); uv[i] *= dl[i]; }
            for (int n = 0; n < N; ++n) {
                const float An = Ap[n];
                float bv[8];
                ld8(Bp + (int64_t)n * L, off, rem, vec, bv);
                float pa = 1.f, pb = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float a = xp_exp_fast(dl[i] * An), bb = bv[i] * uv[i];
                    if (i >= rem) { a = 1.f; bb = 0.f; }
                    pb = a * pb + bb; pa = a * pa;
                }
                bwd_wave_scan_fwd(pa, pb);
                const float hprev = hsub[wave][s][n];
                const float hend = bwd_lane63(pa) * hprev + bwd_lane63(pb);
                if (lane == 0) hsub[wave][s + 1][n] = hend;
            }
        }
        // ---- pass B: the steps right to left
        for (int s = nsub - 1; s >= 0; --s) {
            const int l0 = c0 + s * kStep, off = l0 + lane * 8, rem = L - off;
            float uv[8], tr[8], dl[8], dy[8], ddl[8], dus[8];
            ld8(up, off, rem, vec, uv); ld8(dp, off, rem, vec, tr); ld8(yp, off, rem, vec, dy);
#pragma unroll
            for (int i = 0; i < 8; ++i) { tr[i] += bias; dl[i] = bwd_delta(tr[i], softplus); ddl[i] = 0.f; dus[i] = 0.f; }
            for (int n = 0; n < N; ++n) {
                const float An = Ap[n];
                float bv[8], cv[8], av[8], la[8], lb[8];
                ld8(Bp + (int64_t)n * L, off, rem, vec, bv); ld8(Cp + (int64_t)n * L, off, rem, vec, cv);
                // forward recompute of h inside the step
                float pa = 1.f, pb = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float a = xp_exp_fast(dl[i] * An), bb = dl[i] * bv[i] * uv[i];
                    if (i >= rem) { a = 1.f; bb = 0.f; }
                    av[i] = a;
                    pb = a * pb + bb; pa = a * pa;
                    la[i] = pa; lb[i] = pb;
                }
                float ta = pa, tb = pb;
                bwd_wave_scan_fwd(ta, tb);
                const float ea = bwd_dpp<0x138, 0xf>(1.f, ta), eb = bwd_dpp<0x138, 0xf>(0.f, tb);     // prefix of the lanes before this one
                const float hin = ea * hsub[wave][s][n] + eb;
                // reverse scan of q_l = a_l (q_{l+1} + dy_l C_l)
                float ra[8], rb[8], cc[8];
                float qa = 1.f, qb = 0.f;
#pragma unroll
                for (int i = 7; i >= 0; --i) {
                    cc[i] = i < rem ? dy[i] * cv[i] : 0.f;
                    ra[i] = qa; rb[i] = qb;
                    qb = av[i] * (qb + cc[i]); qa = av[i] * qa;
                }
                float sa = qa, sb = qb;
                bwd_wave_scan_rev(sa, sb, lane);
                float xa = __shfl_down(sa, 1, 64), xb = __shfl_down(sb, 1, 64);
                if (lane == 63) { xa = 1.f; xb = 0.f; }
                const float R = gcar[wave][n];
                const float qr = xa * R + xb;
                const float Rnew = bwd_lane0(sa) * R + bwd_lane0(sb);
                float pA = 0.f, dBv[8], dCv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float hprev = i == 0 ? hin : la[i - 1] * hin + lb[i - 1];
                    const float h = la[i] * hin + lb[i];
                    const float gi = i < rem ? cc[i] + (ra[i] * qr + rb[i]) : 0.f;
                    const float gh = gi * hprev * av[i];
                    dCv[i] = i < rem ? dy[i] * h : 0.f;
                    dBv[i] = gi * dl[i] * uv[i];
                    pA += gh * dl[i];
                    ddl[i] += gh * An + gi * bv[i] * uv[i];
                    dus[i] += gi * dl[i] * bv[i];
                }
                if (lane == 0) gcar[wave][n] = Rnew;
                if (NFIX == 1) accA1 += pA;
                else {
                    const float w = bwd_wave_sum(pA);
                    if (lane == 0) accA[wave][n] += w;
                }
                // dB / dC: the channels of the workgroup, in wave order, into this workgroup's partial
#pragma unroll
                for (int i = 0; i < 8; ++i) { red[0][wave][lane * 8 + i] = valid ? dBv[i] : 0.f; red[1][wave][lane * 8 + i] = valid ? dCv[i] : 0.f; }
                __syncthreads();
                for (int v = threadIdx.x; v < 2 * kStep; v += W * 64) {
                    const int arr = v / kStep, pos = v % kStep;
                    float sum = 0.f;
#pragma unroll
                    for (int w = 0; w < W; ++w) sum += red[arr][w][pos];
                    if (l0 + pos < L) (arr ? bcC : bcB)[(int64_t)n * L + l0 + pos] = sum;
                }
                __syncthreads();
            }
            float duv[8], ddv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool ok = i < rem;
                duv[i] = Dval * dy[i] + dus[i];
                ddv[i] = ok ? (softplus ? ddl[i] / (1.f + xp_exp_fast(-tr[i])) : ddl[i]) : 0.f;
                accD += ok ? dy[i] * uv[i] : 0.f;
                accDB += ddv[i];
            }
            if (valid) {
                st8(static_cast<T*>(p.du) + row * L, off, rem, vec, duv);
                if (rep == 1) st8(static_cast<T*>(p.ddelta) + row * L, off, rem, vec, ddv);
                else st8(p.ddelta_part + row * L, off, rem, vec, ddv);
            }
        }
    }
    const float sD = bwd_wave_sum(accD), sDB = bwd_wave_sum(accDB);
    if (NFIX == 1) {
        const float sA = bwd_wave_sum(accA1);
        if (valid && lane == 0) p.pA[row] = sA;
    } else if (valid) {
        for (int n = lane; n < N; n += 64) p.pA[row * N + n] = accA[wave][n];
    }
    if (valid && lane == 0) { p.pD[row] = sD; p.pdb[row] = sDB; }
}

// dB / dC: sum of the per-workgroup partials in tile order, cast to B's dtype; grouped ddelta: sum over the repeat in channel order
template <class T>
__global__ __launch_bounds__(256) void selective_scan_bwd_reduce_kernel(const float* __restrict__ bc_part, const float* __restrict__ ddelta_part,
                                                                       T* __restrict__ dB, T* __restrict__ dC, T* __restrict__ ddelta,
                                                                       int64_t nbc, int tiles, int64_t NL, int64_t ndd, int rep, int L) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * nbc) {
        const int arr = i >= nbc;
        const int64_t j = i - arr * nbc, bg = j / NL, r = j % NL;
        const float* src = bc_part + arr * nbc * tiles + bg * tiles * NL + r;
        float s = 0.f;
        for (int t = 0; t < tiles; ++t) s += src[t * NL];
        BwdIO<T>::put((arr ? dC : dB) + j, s);
    } else if (i < 2 * nbc + ndd) {
        const int64_t j = i - 2 * nbc, bdd = j / L, l = j % L;          // (b, dd) row of the grouped ddelta
        const float* src = ddelta_part + bdd * rep * (int64_t)L + l;
        float s = 0.f;
        for (int r = 0; r < rep; ++r) s += src[(int64_t)r * L];
        BwdIO<T>::put(ddelta + j, s);
    }
}

// dA (dim, N), dD (dim), ddelta_bias (delta_dim): the per-row partials summed over the batch (and the delta repeat) in order
__global__ __launch_bounds__(256) void selective_scan_bwd_params_kernel(const float* __restrict__ pA, const float* __restrict__ pD, const float* __restrict__ pdb,
                                                                       float* __restrict__ dA, float* __restrict__ dD, float* __restrict__ ddb,
                                                                       int batch, int dim, int N, int delta_dim) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int rep = dim / delta_dim;
    if (i < dim * N) {
        float s = 0.f;
        for (int b = 0; b < batch; ++b) s += pA[(int64_t)b * dim * N + i];
        dA[i] = s;
    } else if (i < dim * N + dim) {
        const int d = i - dim * N;
        if (!dD) return;
        float s = 0.f;
        for (int b = 0; b < batch; ++b) s += pD[(int64_t)b * dim + d];
        dD[d] = s;
    } else if (i < dim * N + dim + delta_dim) {
        const int dd = i - dim * N - dim;
        if (!ddb) return;
        float s = 0.f;
        for (int r = 0; r < rep; ++r)
            for (int b = 0; b < batch; ++b) s += pdb[(int64_t)b * dim + dd * rep + r];
        ddb[dd] = s;
    }
}

constexpr int kWavesN1 = 8, kWavesGen = 4;

struct BwdLayout { size_t bc, ddp, pA, pD, pdb, total; int tiles; };
BwdLayout bwd_layout(int batch, int dim, int delta_dim, int L, int N, int G) {
    BwdLayout w;
    const int W = N == 1 ? kWavesN1 : kWavesGen;
    w.tiles = (dim / G + W - 1) / W;
    auto al = [](size_t n) { return (n * sizeof(float) + 255) & ~(size_t)255; };
    w.bc = 0;
    w.ddp = w.bc + al((size_t)2 * batch * G * w.tiles * N * L);
    w.pA = w.ddp + (delta_dim < dim ? al((size_t)batch * dim * L) : 0);
    w.pD = w.pA + al((size_t)batch * dim * N);
    w.pdb = w.pD + al((size_t)batch * dim);
    w.total = w.pdb + al((size_t)batch * dim);
    return w;
}

template <class T, class OT>
void launch_bwd(const BwdParams& p, int N, int nblocks, hipStream_t s) {
    if (N == 1) hipLaunchKernelGGL((selective_scan_bwd_kernel<T, OT, 1, kWavesN1>), dim3(nblocks), dim3(kWavesN1 * 64), 0, s, p);
    else hipLaunchKernelGGL((selective_scan_bwd_kernel<T, OT, 0, kWavesGen>), dim3(nblocks), dim3(kWavesGen * 64), 0, s, p);
}

}  // namespace

extern "C" size_t xp_selective_scan_bwd_workspace_bytes(int batch, int dim, int delta_dim, int seqlen, int dstate, int ngroups) {
    if (batch <= 0 || dim <= 0 || delta_dim <= 0 || seqlen <= 0 || dstate <= 0 || ngroups <= 0 || dim % ngroups || dim % delta_dim) return 0;
    return bwd_layout(batch, dim, delta_dim, seqlen, dstate, ngroups).total;
}

extern "C" int xp_selective_scan_bwd_typed(const void* u, const void* delta, const float* A, const void* Bm, const void* Cm, const float* Dv,
                                           const float* delta_bias, const void* dout, const float* x_chunks, void* du, void* ddelta, float* dA,
                                           void* dB, void* dC, float* dD, float* ddelta_bias, void* workspace, size_t workspace_bytes, int itype,
                                           int dout_float, int batch, int dim, int delta_dim, int seqlen, int dstate, int ngroups,
                                           int delta_softplus, void* stream) {
    XP_CHECK_ARG(u && delta && A && Bm && Cm && dout && du && ddelta && dA && dB && dC, "xp_selective_scan_bwd_typed: null tensor pointer");
    XP_CHECK_ARG(itype >= 0 && itype <= 2, "xp_selective_scan_bwd_typed: itype 0 (f32), 1 (f16) or 2 (bf16)");
    XP_CHECK_ARG(batch > 0 && dim > 0 && seqlen > 0, "xp_selective_scan_bwd_typed: batch/dim/seqlen must be positive");
    XP_CHECK_ARG(dstate > 0 && dstate <= 256, "xp_selective_scan_bwd_typed: dstate must be in [1,256] (got %d)", dstate);
    XP_CHECK_ARG(ngroups > 0 && dim % ngroups == 0, "xp_selective_scan_bwd_typed: dim %% ngroups != 0");
    XP_CHECK_ARG(delta_dim > 0 && dim % delta_dim == 0, "xp_selective_scan_bwd_typed: dim %% delta_dim != 0");
    XP_CHECK_ARG(!(dD && !Dv) && !(ddelta_bias && !delta_bias), "xp_selective_scan_bwd_typed: dD / ddelta_bias need D / delta_bias");
    XP_CHECK_ARG(x_chunks || seqlen <= kXChunk, "xp_selective_scan_bwd_typed: x (the forward's chunk states) is required when seqlen > %d", kXChunk);
    const BwdLayout w = bwd_layout(batch, dim, delta_dim, seqlen, dstate, ngroups);
    XP_CHECK_ARG(workspace && workspace_bytes >= w.total, "xp_selective_scan_bwd_typed: workspace of %zu bytes needed (got %zu)", w.total, workspace_bytes);
    XP_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "xp_selective_scan_bwd_typed: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    BwdParams p;
    p.u = u; p.delta = delta; p.A = A; p.Bm = Bm; p.Cm = Cm; p.Dv = Dv; p.delta_bias = delta_bias; p.dout = dout; p.x = x_chunks;
    p.du = du; p.ddelta = ddelta;
    p.ddelta_part = reinterpret_cast<float*>(ws + w.ddp); p.bc_part = reinterpret_cast<float*>(ws + w.bc);
    p.pA = reinterpret_cast<float*>(ws + w.pA); p.pD = reinterpret_cast<float*>(ws + w.pD); p.pdb = reinterpret_cast<float*>(ws + w.pdb);
    p.batch = batch; p.dim = dim; p.delta_dim = delta_dim; p.L = seqlen; p.N = dstate; p.G = ngroups; p.softplus = delta_softplus;
    p.tiles = w.tiles;
    const size_t isz = itype == 0 ? 4 : 2, osz = (dout_float || itype == 0) ? 4 : 2;
    const uintptr_t ia = 8 * isz - 1, oa = 8 * osz - 1;
    p.vec = (seqlen % 8 == 0) && ((((uintptr_t)u | (uintptr_t)delta | (uintptr_t)Bm | (uintptr_t)Cm | (uintptr_t)du | (uintptr_t)ddelta) & ia) == 0) &&
            (((uintptr_t)dout & oa) == 0);
    const int nblocks = batch * ngroups * w.tiles;
    const double bdl = (double)batch * dim * seqlen, bgnl = (double)batch * ngroups * dstate * seqlen;
    XpProfScope prof(dstate == 1 ? "selective_scan_bwd_n1" : "selective_scan_bwd_gen", s, 40.0 * dstate * bdl,
                     (3.0 * isz + osz) * bdl + 2.0 * isz * bdl + 4.0 * isz * bgnl + 2.0 * 4.0 * 2.0 * w.tiles * bgnl);
    if (itype == 0) launch_bwd<float, float>(p, dstate, nblocks, s);
    else if (itype == 1) { if (dout_float) launch_bwd<_Float16, float>(p, dstate, nblocks, s); else launch_bwd<_Float16, _Float16>(p, dstate, nblocks, s); }
    else { if (dout_float) launch_bwd<__bf16, float>(p, dstate, nblocks, s); else launch_bwd<__bf16, __bf16>(p, dstate, nblocks, s); }
    XP_LAUNCH_CHECK();
    const int64_t nbc = (int64_t)batch * ngroups * dstate * seqlen, ndd = delta_dim < dim ? (int64_t)batch * delta_dim * seqlen : 0;
    const int64_t nred = 2 * nbc + ndd;
    const int rep = dim / delta_dim;
#define XP_RED(T) hipLaunchKernelGGL(selective_scan_bwd_reduce_kernel<T>, dim3((unsigned)((nred + 255) / 256)), dim3(256), 0, s, p.bc_part, p.ddelta_part, \
                                     (T*)dB, (T*)dC, (T*)ddelta, nbc, w.tiles, (int64_t)dstate * seqlen, ndd, rep, seqlen)
    if (itype == 0) XP_RED(float); else if (itype == 1) XP_RED(_Float16); else XP_RED(__bf16);
#undef XP_RED
    XP_LAUNCH_CHECK();
    const int nparam = dim * dstate + dim + delta_dim;
    hipLaunchKernelGGL(selective_scan_bwd_params_kernel, dim3((nparam + 255) / 256), dim3(256), 0, s, p.pA, p.pD, p.pdb, dA, dD, ddelta_bias,
                       batch, dim, dstate, delta_dim);
    XP_LAUNCH_CHECK();
    return XP_OK;
}
