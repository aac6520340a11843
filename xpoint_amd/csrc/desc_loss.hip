// Dense descriptor loss of XPoint training (reference xpoint/utils/losses.py:688-755), forward and backward, without ever
// writing an (HW x HW) tensor.  Per sample b, with t a cell of one image and r a cell of the other:
//     dot = <d_t, d_r>,  s = [ |w_t - w_r| <= threshold ],  v = v_t v_r
//     pos = lambda_d s max(0, mp - dot) v,   neg = (1 - s) max(0, dot - mn) v,   sums over all pairs, norm_b = sum v2 * sum v1.
//
// CDNA4 mapping.  A pre-pass (dl_convert_kernel) turns each NCHW f32 descriptor image into split-fp16 planes (hi = fp16(S x),
// lo = fp16(S x - hi); S = one power of two PER SAMPLE that puts the sample's largest |x| into [1024, 2048), so no lo part of a
// significant element is an fp16 subnormal and a sample's planes do not depend on its batch neighbours), stored per block of
// 32 cells in the exact register image of the v_mfma_f32_32x32x16_f16 operands, twice:
//     CM (cell-major):  lane (c, h), element e of k-step ks  = x[cell c][k = 16 ks + 8 h + e]             Gram operand (A or B)
//     KM (k-major):     lane (kr, h), element e of step s     = x[cell 16 s + 8 (e >> 2) + 4 h + (e & 3)][k = 32 kb + kr]
// so a fragment is ONE coalesced 16-byte load per lane, no transposing read and no lane masks; dead cells past HW and dead k past
// D are zeros with cell mask 0.  The KM order is the row order of a 32x32 accumulator tile's registers 8s..8s+7: the Gram tile's
// accumulator, turned into the gradient factor g in place, is the B operand of the second product with no lane movement.
//
// One kernel, dl_sweep_kernel, does forward and both gradient sweeps.  A workgroup of 4 waves owns 128 "resident" cells r (each
// wave 32: split planes in registers for the whole kernel) and walks every 32-cell block t of the other image, staged through LDS
// (global -> registers one block ahead -> LDS).  X[t][r] = dot on the matrix pipe as hi.hi + (hi.lo + lo.hi) (gemm_h2_core.h's
// three products, f32 accumulate), epilogue from 4 floats per row / column (warped centre y, x, cell mask).
//   forward : three sums per lane in f64, one partial per wave, reduced in a fixed order by dl_finish_kernel.
//   backward: g[t][r] = (alpha [!s][dot > mn] + beta [s][dot < mp]) v_t in fp16 (exact: alpha = 1, beta = -lambda_d when lambda_d
//             is an fp16 number, else two sweeps with (1, 0) and (0, 1) whose f32 results are combined), then
//             Y[k][r] += sum_t x_t[k] g[t][r] with x_t split hi + lo (two MFMAs per 32 k), Y (D x 32 per wave) in registers until
//             the sweep ends; dD[b][k][r] = c_b v_r Y / S.  Sweep 1: r = image 1, t = image 2 (dD1); sweep 2 the other way (dD2).
// No atomics, no partial gradient buffers: every output element has exactly one writer and a fixed summation order, and a sample's
// work does not depend on the batch size, so results are bit-reproducible and per-sample batch invariant.
#include "xp_common.h"
#include "xpoint_hip.h"

typedef _Float16 dl_h8 __attribute__((ext_vector_type(8)));
typedef float dl_f16 __attribute__((ext_vector_type(16)));
typedef unsigned dl_u4 __attribute__((ext_vector_type(4)));      // native vectors: arrays of HIP's uint4 / float4 structs stay in scratch
typedef float dl_f4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int DL_PARTS = 64;        // partial maxima per sample
constexpr int DL_WAVES = 4;         // waves per sweep workgroup, 32 resident cells each

static inline size_t dl_up(size_t n) { return (n + 255) / 256 * 256; }
static inline int dl_ks(int D) { return (D + 63) / 64 * 4; }           // 16-wide k steps of the staged planes (D padded to 64)

struct DlWs {
    float* amax;       // (B, DL_PARTS)
    float2* scale;     // (B): S, 1 / S
    float4* cell1;     // (B, NP): y, x, v, 0
    float4* cell2;
    uint4* img1;       // (B, nblk, KS * 256) 16-byte units: CM then KM
    uint4* img2;
    double* part;      // (B, nstrips * DL_WAVES, 2): sum pos / lambda_d, sum neg
    int NP, nblk, nstrips, KS;
    size_t bytes;
};

static DlWs dl_carve(void* ws, int B, int D, int HW) {
    DlWs w;
    w.KS = dl_ks(D);
    w.NP = (HW + 127) / 128 * 128;
    w.nblk = w.NP / 32;
    w.nstrips = w.NP / 128;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* q = p + off; off += dl_up(n); return q; };
    w.amax = (float*)take((size_t)B * DL_PARTS * sizeof(float));
    w.scale = (float2*)take((size_t)B * sizeof(float2));
    w.cell1 = (float4*)take((size_t)B * w.NP * sizeof(float4));
    w.cell2 = (float4*)take((size_t)B * w.NP * sizeof(float4));
    const size_t img = (size_t)B * w.nblk * w.KS * 256 * sizeof(uint4);
    w.img1 = (uint4*)take(img);
    w.img2 = (uint4*)take(img);
    w.part = (double*)take((size_t)B * w.nstrips * DL_WAVES * 2 * sizeof(double));
    w.bytes = off;
    return w;
}

// ---- pass 0a: largest |x| of each sample over both descriptor images (maxima: order-free, hence deterministic) ----
__global__ __launch_bounds__(256) void dl_amax_kernel(const float* __restrict__ d1, const float* __restrict__ d2, int64_t n, float* __restrict__ part) {
    const int b = blockIdx.y;
    const float* p1 = d1 + (size_t)b * n;
    const float* p2 = d2 + (size_t)b * n;
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)DL_PARTS * 256) m = fmaxf(m, fmaxf(fabsf(p1[i]), fabsf(p2[i])));
    m = xp_block_max256(m);
    if (threadIdx.x == 0) part[b * DL_PARTS + blockIdx.x] = m;
}

// ---- pass 0b: the sample's power of two ----
__global__ __launch_bounds__(64) void dl_scale_kernel(const float* __restrict__ part, float2* __restrict__ scale) {
    const int b = blockIdx.x;
    const float m = xp_wave_max(part[b * DL_PARTS + threadIdx.x]);
    if (threadIdx.x == 0) {
        int e = 11;                                    // m == 0 or not finite: S = 1
        if (m > 0.f && m <= 3.0e38f) (void)frexpf(m, &e);           // m = f 2^e, f in [0.5, 1)  ->  m 2^(11 - e) in [1024, 2048)
        int se = 11 - e;
        se = se < -100 ? -100 : (se > 100 ? 100 : se);
        scale[b] = make_float2(ldexpf(1.f, se), ldexpf(1.f, -se));
    }
}

// ---- pass 0c: split-fp16 operand images of one block of 32 cells + the cells' (y, x, v) ----
template <int KS>
__global__ __launch_bounds__(256) void dl_convert_kernel(const float* __restrict__ d1, const float* __restrict__ d2, const float* __restrict__ w1,
                                                         const float* __restrict__ w2, const float* __restrict__ v1, const float* __restrict__ v2,
                                                         const float2* __restrict__ scale, uint4* __restrict__ img1, uint4* __restrict__ img2,
                                                         float4* __restrict__ cell1, float4* __restrict__ cell2, int D, int HW, int Wc, int NP, int nblk) {
    constexpr int KD = KS * 16;
    __shared__ float tile[KD][33];
    const int blk = blockIdx.x, which = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const float* src = (which ? d2 : d1) + (size_t)b * D * HW;
    const float* w = which ? w2 : w1;
    const float* v = which ? v2 : v1;
    uint4* img = (which ? img2 : img1) + ((size_t)b * nblk + blk) * (KS * 256);
    float4* cell = (which ? cell2 : cell1) + (size_t)b * NP + blk * 32;
    const float S = scale[b].x;
    for (int idx = tid; idx < KD * 32; idx += 256) {
        const int k = idx >> 5, c = idx & 31, n = blk * 32 + c;
        tile[k][c] = (k < D && n < HW) ? src[(size_t)k * HW + n] * S : 0.f;
    }
    if (tid < 32) {
        const int n = blk * 32 + tid;
        float4 ci = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n < HW) {
            if (w) { ci.x = w[((size_t)b * HW + n) * 2]; ci.y = w[((size_t)b * HW + n) * 2 + 1]; }
            else { ci.x = (float)(n / Wc) * 8.f + 4.f; ci.y = (float)(n % Wc) * 8.f + 4.f; }
            ci.z = v ? v[(size_t)b * HW + n] : 1.f;
        }
        cell[tid] = ci;
    }
    __syncthreads();
    for (int u = tid; u < KS * 256; u += 256) {
        const int lane = u & 63, plane = (u >> 6) & 1, r = lane & 31, h = lane >> 5;
        dl_h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float x;
            if (u < KS * 128) {
                x = tile[16 * (u >> 7) + 8 * h + e][r];                                            // CM: ks = u >> 7
            } else {
                const int q = u - KS * 128, s = (q >> 7) & 1, kb = q >> 8;
                x = tile[kb * 32 + r][16 * s + 8 * (e >> 2) + 4 * h + (e & 3)];                    // KM
            }
            const _Float16 hi = (_Float16)x;
            o[e] = plane ? (_Float16)(x - (float)hi) : hi;
        }
        img[u] = __builtin_bit_cast(uint4, o);
    }
}

struct DlSweep {
    const dl_u4* imgR;
    const dl_u4* imgT;
    const dl_f4* cellR;
    const dl_f4* cellT;
    const float2* scale;
    const float* coef;        // backward: c_b (device, (B))
    float* out;               // backward: (B, D, HW)
    double* part;             // forward
    int nblk, NP, HW, D, accumulate;
    float thr, mp, mn, alpha, beta, outscale;
};

__device__ __forceinline__ double dl_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int KS, bool BWD>
__global__ __launch_bounds__(256) void dl_sweep_kernel(DlSweep p) {
    constexpr int BLK = KS * 256;                       // 16-byte units of a staged block in memory
    constexpr int TU = BWD ? KS * 256 : KS * 128;       // units of it that this kernel stages (the forward needs the CM half only)
    constexpr int PER = TU / 256;
    constexpr int KB = KS / 2;
    extern __shared__ dl_u4 dl_lds[];
    dl_f4* ldsc = (dl_f4*)(dl_lds + TU);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, rr = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, rblk = blockIdx.x * DL_WAVES + wv;
    const float invS = p.scale[b].y;

    dl_h8 rf[KS][2];
    {
        const dl_u4* R = p.imgR + ((size_t)b * p.nblk + rblk) * BLK;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            rf[ks][0] = __builtin_bit_cast(dl_h8, R[(ks * 2 + 0) * 64 + lane]);
            rf[ks][1] = __builtin_bit_cast(dl_h8, R[(ks * 2 + 1) * 64 + lane]);
        }
    }
    const dl_f4 cr = p.cellR[(size_t)b * p.NP + rblk * 32 + rr];

    dl_f16 Y[BWD ? KB : 1];
#pragma unroll
    for (int i = 0; i < (BWD ? KB : 1); ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) Y[i][e] = 0.f;
    double sp = 0.0, sn = 0.0;

    dl_u4 pf[PER];
    dl_f4 pfc;
    const dl_u4* T = p.imgT + (size_t)b * p.nblk * BLK + tid;
    const dl_f4* CT = p.cellT + (size_t)b * p.NP + (tid & 31);
#pragma unroll
    for (int q = 0; q < PER; ++q) pf[q] = T[q * 256];
    pfc = CT[0];
    for (int tb = 0; tb < p.nblk; ++tb) {
        __syncthreads();                                // the previous block's readers are done
#pragma unroll
        for (int q = 0; q < PER; ++q) dl_lds[q * 256 + tid] = pf[q];
        if (tid < 32) ldsc[tid] = pfc;
        __syncthreads();
        if (tb + 1 < p.nblk) {
#pragma unroll
            for (int q = 0; q < PER; ++q) pf[q] = T[(size_t)(tb + 1) * BLK + q * 256];
            pfc = CT[(tb + 1) * 32];
        }

        dl_f16 ahh, ax;
#pragma unroll
        for (int e = 0; e < 16; ++e) { ahh[e] = 0.f; ax[e] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const dl_h8 th = __builtin_bit_cast(dl_h8, dl_lds[(ks * 2 + 0) * 64 + lane]);
            const dl_h8 tl = __builtin_bit_cast(dl_h8, dl_lds[(ks * 2 + 1) * 64 + lane]);
            ahh = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, rf[ks][0], ahh, 0, 0, 0);
            ax = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, rf[ks][1], ax, 0, 0, 0);
            ax = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, rf[ks][0], ax, 0, 0, 0);
        }
        // epilogue: accumulator register e of lane (rr, h) is X[t = (e & 3) + 8 (e >> 2) + 4 h][r = rr]
        float tp = 0.f, tn = 0.f;
        _Float16 gh[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const dl_f4 ct = ldsc[(e & 3) + 8 * (e >> 2) + 4 * h];
            const float dot = (ahh[e] + ax[e]) * invS * invS;
            const float dy = cr.x - ct.x, dx = cr.y - ct.y;
            const bool s = sqrtf(dy * dy + dx * dx) <= p.thr;
            if (BWD) {
                const float g = (s ? (dot < p.mp ? p.beta : 0.f) : (dot > p.mn ? p.alpha : 0.f)) * ct.z;
                gh[e] = (_Float16)g;
            } else {
                const float v = ct.z * cr.z;
                tp += s ? fmaxf(0.f, p.mp - dot) * v : 0.f;
                tn += s ? 0.f : fmaxf(0.f, dot - p.mn) * v;
            }
        }
        if (BWD) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                dl_h8 gf;
#pragma unroll
                for (int e = 0; e < 8; ++e) gf[e] = gh[8 * s2 + e];
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) {
                    const dl_h8 th = __builtin_bit_cast(dl_h8, dl_lds[KS * 128 + ((kb * 2 + s2) * 2 + 0) * 64 + lane]);
                    const dl_h8 tl = __builtin_bit_cast(dl_h8, dl_lds[KS * 128 + ((kb * 2 + s2) * 2 + 1) * 64 + lane]);
                    Y[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, gf, Y[kb], 0, 0, 0);
                    Y[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, gf, Y[kb], 0, 0, 0);
                }
            }
        } else {
            sp += (double)tp;
            sn += (double)tn;
        }
    }
    if (BWD) {
        const int n = rblk * 32 + rr;
        const float c = p.coef[b] * p.outscale * cr.z;
        if (n < p.HW) {
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int k = kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (k < p.D) {
                        float* o = p.out + ((size_t)b * p.D + k) * p.HW + n;
                        const float val = Y[kb][e] * invS * c;
                        *o = p.accumulate ? *o + val : val;
                    }
                }
        }
    } else {
        sp = dl_wave_sum(sp);
        sn = dl_wave_sum(sn);
        if (lane == 0) {
            double* o = p.part + ((size_t)b * gridDim.x * DL_WAVES + rblk) * 2;
            o[0] = sp;
            o[1] = sn;
        }
    }
}

// ---- forward finish: fixed-order sum of the wave partials, the two mask sums and norm_b ----
__global__ __launch_bounds__(256) void dl_finish_kernel(const double* __restrict__ part, const float4* __restrict__ cell1, const float4* __restrict__ cell2,
                                                        int nparts, int NP, float lambda_d, float* __restrict__ sums, float* __restrict__ norm) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ double s1[256], s2[256];
    double a1 = 0.0, a2 = 0.0;
    for (int n = tid; n < NP; n += 256) { a1 += (double)cell1[(size_t)b * NP + n].z; a2 += (double)cell2[(size_t)b * NP + n].z; }
    s1[tid] = a1; s2[tid] = a2;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (tid < m) { s1[tid] += s1[tid + m]; s2[tid] += s2[tid + m]; }
        __syncthreads();
    }
    if (tid == 0) {
        double P = 0.0, N = 0.0;
        for (int i = 0; i < nparts; ++i) { P += part[((size_t)b * nparts + i) * 2]; N += part[((size_t)b * nparts + i) * 2 + 1]; }
        P *= (double)lambda_d;
        sums[b * 3 + 0] = (float)(P + N);
        sums[b * 3 + 1] = (float)P;
        sums[b * 3 + 2] = (float)N;
        norm[b] = (float)(s2[0] * s1[0]);
    }
}

template <int KS, bool BWD>
static int dl_launch_sweep(const DlSweep& p, int nstrips, int B, hipStream_t s) {
    constexpr size_t lds = (size_t)(BWD ? KS * 256 : KS * 128) * sizeof(uint4) + 32 * sizeof(float4);
    static XpPerDeviceOnce once;
    if (once.need()) XP_HIP(hipFuncSetAttribute((const void*)dl_sweep_kernel<KS, BWD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((dl_sweep_kernel<KS, BWD>), dim3(nstrips, B), dim3(256), lds, s, p);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

template <bool BWD>
static int dl_sweep(int KS, const DlSweep& p, int nstrips, int B, hipStream_t s) {
    switch (KS) {
        case 4: return dl_launch_sweep<4, BWD>(p, nstrips, B, s);
        case 8: return dl_launch_sweep<8, BWD>(p, nstrips, B, s);
        case 12: return dl_launch_sweep<12, BWD>(p, nstrips, B, s);
        default: return dl_launch_sweep<16, BWD>(p, nstrips, B, s);
    }
}

static int dl_check(const char* who, int B, int D, int Hc, int Wc) {
    XP_CHECK_ARG(B > 0 && Hc > 0 && Wc > 0 && (int64_t)Hc * Wc <= (1 << 24), "%s: bad shape B=%d Hc=%d Wc=%d", who, B, Hc, Wc);
    XP_CHECK_ARG(D >= 16 && D <= 256 && D % 16 == 0, "%s: D must be a multiple of 16 in [16, 256] (got %d)", who, D);
    return XP_OK;
}

// lambda_d (hence -lambda_d) is an fp16 number: at most 11 significant bits, normal fp16 range
static bool dl_is_f16(float x) {
    if (x == 0.f) return true;
    int e;
    const float m = frexpf(fabsf(x), &e);
    const float q = m * 2048.f;
    return q == floorf(q) && e >= -13 && e <= 16;
}

}  // namespace

extern "C" size_t xp_descriptor_loss_workspace_bytes(int B, int D, int Hc, int Wc) {
    if (B <= 0 || D <= 0 || Hc <= 0 || Wc <= 0 || D > 256) return 0;
    return dl_carve(nullptr, B, D, Hc * Wc).bytes;
}

extern "C" int xp_descriptor_loss_fwd(const float* d1, const float* d2, const float* w1, const float* w2, const float* v1, const float* v2, int B, int D,
                                      int Hc, int Wc, float threshold, float positive_margin, float negative_margin, float lambda_d, void* workspace,
                                      size_t workspace_bytes, float* sums, float* norm, void* stream) {
    if (int rc = dl_check("xp_descriptor_loss_fwd", B, D, Hc, Wc)) return rc;
    XP_CHECK_ARG(d1 && d2 && workspace && sums && norm, "xp_descriptor_loss_fwd: null pointer");
    const int HW = Hc * Wc;
    const DlWs w = dl_carve(workspace, B, D, HW);
    XP_CHECK_ARG(workspace_bytes >= w.bytes, "xp_descriptor_loss_fwd: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    XP_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "xp_descriptor_loss_fwd: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const double gram = 2.0 * 3.0 * B * (double)w.NP * w.NP * (w.KS * 16);
    XpProfScope prof("descriptor_loss_fwd", s, gram, 2.0 * B * (double)D * HW * 4);
    hipLaunchKernelGGL(dl_amax_kernel, dim3(DL_PARTS, B), dim3(256), 0, s, d1, d2, (int64_t)D * HW, w.amax);
    XP_LAUNCH_CHECK();
    hipLaunchKernelGGL(dl_scale_kernel, dim3(B), dim3(64), 0, s, w.amax, w.scale);
    XP_LAUNCH_CHECK();
#define DL_CONVERT(KS_)                                                                                                                                   \
    hipLaunchKernelGGL((dl_convert_kernel<KS_>), dim3(w.nblk, 2, B), dim3(256), 0, s, d1, d2, w1, w2, v1, v2, w.scale, w.img1, w.img2, w.cell1, w.cell2, \
                       D, HW, Wc, w.NP, w.nblk)
    switch (w.KS) {
        case 4: DL_CONVERT(4); break;
        case 8: DL_CONVERT(8); break;
        case 12: DL_CONVERT(12); break;
        default: DL_CONVERT(16); break;
    }
#undef DL_CONVERT
    XP_LAUNCH_CHECK();
    DlSweep p = {};
    p.imgR = (const dl_u4*)w.img1; p.imgT = (const dl_u4*)w.img2; p.cellR = (const dl_f4*)w.cell1; p.cellT = (const dl_f4*)w.cell2; p.scale = w.scale; p.part = w.part;
    p.nblk = w.nblk; p.NP = w.NP; p.HW = HW; p.D = D;
    p.thr = threshold; p.mp = positive_margin; p.mn = negative_margin;
    if (int rc = dl_sweep<false>(w.KS, p, w.nstrips, B, s)) return rc;
    hipLaunchKernelGGL(dl_finish_kernel, dim3(B), dim3(256), 0, s, w.part, w.cell1, w.cell2, w.nstrips * DL_WAVES, w.NP, lambda_d, sums, norm);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_descriptor_loss_bwd(const float* coef, int B, int D, int Hc, int Wc, float threshold, float positive_margin, float negative_margin,
                                      float lambda_d, const void* workspace, size_t workspace_bytes, float* dD1, float* dD2, void* stream) {
    if (int rc = dl_check("xp_descriptor_loss_bwd", B, D, Hc, Wc)) return rc;
    XP_CHECK_ARG(coef && workspace, "xp_descriptor_loss_bwd: null pointer");
    const int HW = Hc * Wc;
    const DlWs w = dl_carve((void*)workspace, B, D, HW);
    XP_CHECK_ARG(workspace_bytes >= w.bytes, "xp_descriptor_loss_bwd: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    const bool exact = dl_is_f16(lambda_d);
    const int sweeps = (dD1 ? 1 : 0) + (dD2 ? 1 : 0);
    XpProfScope prof("descriptor_loss_bwd", s, sweeps * (exact ? 1 : 2) * 2.0 * 5.0 * B * (double)w.NP * w.NP * (w.KS * 16), sweeps * (double)B * D * HW * 8);
    for (int which = 0; which < 2; ++which) {
        float* out = which ? dD2 : dD1;
        if (!out) continue;
        DlSweep p = {};
        p.imgR = (const dl_u4*)(which ? w.img2 : w.img1); p.imgT = (const dl_u4*)(which ? w.img1 : w.img2);
        p.cellR = (const dl_f4*)(which ? w.cell2 : w.cell1); p.cellT = (const dl_f4*)(which ? w.cell1 : w.cell2);
        p.scale = w.scale; p.coef = coef; p.out = out;
        p.nblk = w.nblk; p.NP = w.NP; p.HW = HW; p.D = D;
        p.thr = threshold; p.mp = positive_margin; p.mn = negative_margin;
        if (exact) {
            p.alpha = 1.f; p.beta = -lambda_d; p.outscale = 1.f; p.accumulate = 0;
            if (int rc = dl_sweep<true>(w.KS, p, w.nstrips, B, s)) return rc;
        } else {                            // negative part, then the positive part scaled by -lambda_d in f32
            p.alpha = 1.f; p.beta = 0.f; p.outscale = 1.f; p.accumulate = 0;
            if (int rc = dl_sweep<true>(w.KS, p, w.nstrips, B, s)) return rc;
            p.alpha = 0.f; p.beta = 1.f; p.outscale = -lambda_d; p.accumulate = 1;
            if (int rc = dl_sweep<true>(w.KS, p, w.nstrips, B, s)) return rc;
        }
    }
    return XP_OK;
}
