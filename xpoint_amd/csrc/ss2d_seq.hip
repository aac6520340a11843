// The sequential form of the fused SS2D core (deep stages): one wave, or a pipeline of NW waves, per route of 64 channels; a second kernel merges the four
// routes and applies out_norm.  ss2d.hip has the operator's description and the choice between the forms.
#include <stdlib.h>

#include <string>

#include "ss2d_core.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Sequential form for the deepest stage (short sequences, many channels: L = 300 x C = 768 at 480 x 640; measured slower than the
// chunked form at L = 1200 x C = 384, where 1200 dependent steps of one wave per SIMD outlast the three passes).  With 3072-float LDS tiles the chunks above shrink to 8 pixels there, every step is evaluated twice (summary
// pass + re-run) and the three passes cost as much as at stage 1 for a half / a quarter of the steps.  Here one wave
// walks ONE route of 64 channels of one image from end to end — every step evaluated once, no carry pass — and writes the
// route's y; a second kernel adds the four routes in the reference's order (y0 + y2) + (y1 + y3) (csm_triton.py:60-62) and applies
// out_norm.  batch * 4 * C / 64 independent waves (768 at both deep stages of a 16-image batch); u and the route's xdbl rows
// are fetched a 32-pixel tile ahead.
// ---------------------------------------------------------------------------------------------------------------
constexpr int SEQ_TP = 32;
// The dt_rank >= 16 kernels below are held to TWO waves per SIMD: vector + accumulator registers <= 256 of the SIMD's 512 per lane.  A lone wave issues a
// vector instruction every ~5.4 cycles, two resident waves one every ~2.7 (tools/pkfma_probe.hip), and these kernels are issue-bound.  The attribute makes the
// register allocator keep the bound; it must be met without scratch (profiles/ss2d_seq_occupancy.txt has the compiler's report).
constexpr int SEQ_RESIDENT = 2;
#define XP_SEQ_TWO_WAVES __attribute__((amdgpu_waves_per_eu(2)))
typedef volatile __attribute__((address_space(3))) int* SeqLdsInt;      // the wave-to-wave turn protocol's LDS words, accessed with DS instructions
typedef volatile __attribute__((address_space(3))) float* SeqLdsFloat;
template <int R>
__global__ __launch_bounds__(64) void ss2d_seq_scan(SS2DParams p, float* __restrict__ ys) {
    constexpr int RW = R + 2, HW2 = RW / 2;                             // floats / float2 pieces per xdbl row of one route
    static_assert(HW2 <= 32, "two rows per staging instruction");
    __shared__ __align__(16) float s_x[2][SEQ_TP * RW];
    const int lane = threadIdx.x, d = blockIdx.y, b = blockIdx.z;
    const int pair = d >> 1, back = d & 1;                              // directions in the stored order (0, 2, 1, 3)
    const int c = blockIdx.x * 64 + lane;                               // C % 64 == 0 (host)
    const int L = p.H * p.W, XD = 4 * RW;
    float w[R];
#pragma unroll
    for (int r = 0; r < R; ++r) w[r] = XP_L2E * p.wdt[((int64_t)d * R + r) * p.C + c];
    const float bias = XP_L2E * p.dtb[d * p.C + c], Av = XP_L2E * p.A[d * p.C + c], Dv = p.Dp[d * p.C + c];
    const float* ub = p.u + (int64_t)b * L * p.C + c;
    const float* xb = p.xdbl + (int64_t)b * L * XD + pair * 2 * RW + back * RW + 2 * (lane & 31);
    float* yb = ys + ((int64_t)d * p.Bn + b) * L * p.C + c;
    // sequence index i -> pixel: forward routes walk l = i, backward routes l = L - 1 - i (the flipped sequence, csm_triton.py:33-36);
    // column-major routes need (w, h) = (l / H, l % H): one division per tile, then stepping (a division per step and use —
    // three per step — was a third of this kernel).  Indices past the end repeat the last pixel (loaded, never stored).
    auto tile_pixels = [&](int t, int (&px)[SEQ_TP]) {
        const int i0 = t * SEQ_TP;
        if (pair == 0) {
#pragma unroll
            for (int j = 0; j < SEQ_TP; ++j) { const int i = min(i0 + j, L - 1); px[j] = back ? L - 1 - i : i; }
        } else {
            const int l0 = back ? L - 1 - i0 : i0;
            int ww = l0 / p.H, hh = l0 - ww * p.H;
#pragma unroll
            for (int j = 0; j < SEQ_TP; ++j) {
                px[j] = hh * p.W + ww;
                if (i0 + j < L - 1) {
                    if (back) { if (--hh < 0) { hh = p.H - 1; --ww; } }
                    else { if (++hh == p.H) { hh = 0; ++ww; } }
                }
            }
        }
    };
    const int ntile = (L + SEQ_TP - 1) / SEQ_TP;
    float ucur[SEQ_TP], unext[SEQ_TP];
    int pxc[SEQ_TP], pxn[SEQ_TP];          // wave-uniform
    float2 xreg[SEQ_TP / 2];
    auto load_u = [&](const int (&px)[SEQ_TP], float (&uv)[SEQ_TP]) {
#pragma unroll
        for (int j = 0; j < SEQ_TP; ++j) uv[j] = ub[px[j] * p.C];      // 32-bit offsets (host checks H*W*C < 2^31)
    };
    // two xdbl rows per instruction: lanes 0..31 row 2q, lanes 32..63 row 2q+1, float2 piece lane & 31 (lanes past the row
    // length load a valid neighbour and are not stored)
    const bool xok = (lane & 31) < HW2;
    auto load_x = [&](const int (&px)[SEQ_TP]) {
#pragma unroll
        for (int q = 0; q < SEQ_TP / 2; ++q) {
            const int pj = (lane >> 5) ? px[2 * q + 1] : px[2 * q];
            xreg[q] = *reinterpret_cast<const float2*>(xb + (xok ? (int64_t)pj * XD : 0));
        }
    };
    const int xdst = (lane >> 5) * RW + 2 * (lane & 31);
    auto store_x = [&](int buf) {
        if (xok) {
#pragma unroll
            for (int q = 0; q < SEQ_TP / 2; ++q) *reinterpret_cast<float2*>(&s_x[buf][2 * q * RW + xdst]) = xreg[q];
        }
    };
    tile_pixels(0, pxc);
    load_u(pxc, ucur); load_x(pxc); store_x(0);
    float h = 0.f;
    // four steps at a time: their operand evaluation (projection, softplus, exp) is independent and interleaves; only the
    // h update is a chain.  Full tiles carry no bounds tests; the last, partial tile evaluates on valid LDS rows and masks its stores.
    auto run_tile = [&](const float* sx, int nj, auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
        for (int j0 = 0; j0 < SEQ_TP; j0 += 4) {
            if (FULL || j0 < nj) {                                      // uniform
                float a[4], bb[4], cv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) step_vals<R>(sx + (j0 + k) * RW, w, bias, Av, ucur[j0 + k], a[k], bb[k], cv[k]);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    h = a[k] * h + bb[k];
                    if (FULL || j0 + k < nj) yb[pxc[j0 + k] * p.C] = cv[k] * h + Dv * ucur[j0 + k];   // y = C*h + D*u (csms6s.py:61,67)
                }
            }
        }
    };
    for (int t = 0; t < ntile; ++t) {
        if (t + 1 < ntile) { tile_pixels(t + 1, pxn); load_u(pxn, unext); load_x(pxn); }
        const int nj = L - t * SEQ_TP;
        if (nj >= SEQ_TP) run_tile(s_x[t & 1], SEQ_TP, std::true_type{});
        else run_tile(s_x[t & 1], nj, std::false_type{});
        if (t + 1 < ntile) {
            store_x((t + 1) & 1);
#pragma unroll
            for (int j = 0; j < SEQ_TP; ++j) { ucur[j] = unext[j]; pxc[j] = pxn[j]; }
        }
    }
}

// Which route a workgroup of the dt_rank >= 16 kernels takes.  Workgroup ids go round-robin to the 8 XCDs, one L2 each, and the four routes of one (image,
// 64-channel group) read the same u columns and the same xdbl rows: in grid order (channel group fastest, then route) they land on four different XCDs and u
// is fetched past L2 four times per launch (profiles/ss2d_seq_occupancy.txt).  Here ids 8 q + x, q = 4 s .. 4 s + 3, are the four routes of group x (G / 8) + s: one
// XCD, adjacent slots, and every XCD takes one contiguous run of groups — the channel groups of the same few images, whose xdbl rows then pass through one
// L2 instead of eight.  Groups past the last whole eight keep a plain order.  A bijection of the grid: placement only, never results.
__device__ __forceinline__ void seq_block_route(int& cg, int& d, int& b) {
    const int gx = gridDim.x, G = gx * gridDim.z;
    const int lin = blockIdx.x + gx * (blockIdx.y + 4 * blockIdx.z);
    const int whole = (G >> 3) * 32;
    int g;
    if (lin < whole) { const int q = lin >> 3; d = q & 3; g = (lin & 7) * (G >> 3) + (q >> 2); }
    else { const int rem = lin - whole; d = rem & 3; g = (G & ~7) + (rem >> 2); }
    b = g / gx; cg = g - b * gx;
}

// Sequential form for dt_rank >= 16 (the deep stages), written for INSTRUCTION COUNT: with one wave per SIMD every instruction of any
// kind — scalar address arithmetic, branches, LDS reads — is issue time, and the first kernel above spends ~3 500 of them per 32-pixel
// tile (64-bit scalar address chains per access, a branchy scalar walk of the pixel order, R FMAs per step).  Here
//  * the dt projection of a tile runs on the matrix pipe:  dt[pixel][channel] = bias[channel] + sum_r x[pixel][r] Wdt[channel][r]  as two
//    32x32 MFMA tiles (64 channels) x ceil(R / 16) slabs, both operands split into two fp16 planes, three products per slab
//    (gemm_h2_core.h: operand error <= 2^-23 — f32-grade); the weight fragments stay in registers (as many as the R scalar weights they
//    replace), the pixel rows are split from the LDS tile.  The accumulator layout (lane = column = channel, 16 registers = rows
//    {0-3, 8-11, 16-19, 24-27} + 4 (lane >> 5)) becomes "lane = channel, 32 registers = the tile's 32 pixels" with one
//    v_permlane32_swap per register pair of the two tiles — the scan's own layout;
//  * a tile's pixel offsets are computed once by 32 lanes (vector arithmetic, one reciprocal multiply for the column-major routes) and
//    reach the memory instructions as the SCALAR offset of a buffer access (v_readlane + buffer_load / buffer_store: two instructions
//    per access); pixels past the end get an out-of-range offset, which the buffer hardware turns into a dropped store / a zero load,
//    so there is one code path for full and partial tiles;
//  * the tile's xdbl rows are fetched one row per lane pair with immediate offsets (no address arithmetic).
template <int R, bool AMP = false>
__global__ __launch_bounds__(64) XP_SEQ_TWO_WAVES void ss2d_seq_scan2(SS2DParams p, float* __restrict__ ys) {
    constexpr int RW = R + 2, NP = RW / 2, NPL = (NP + 1) / 2;          // float2 pieces per xdbl row of one route; pieces fetched by one lane
    __shared__ __align__(16) float s_x[2][SEQ_TP * RW];
    const int lane = threadIdx.x;
    int cg, d, b;
    seq_block_route(cg, d, b);
    const int pair = d >> 1, back = d & 1;                              // directions in the stored order (0, 2, 1, 3)
    const int fr = lane & 31, fh = lane >> 5;
    const int L = p.H * p.W, XD = 4 * RW;
    const int c = cg * 64 + lane;                                       // C % 64 == 0 (host)
    DtWeights<R> dw;
    dt_load_weights<R, AMP>(dw, p.wdt + (int64_t)d * R * p.C, p.dtb + d * p.C, p.C, cg * 64);
    const float Av = XP_L2E * p.A[d * p.C + c], Dv = p.Dp[d * p.C + c];
#define XP_SEQ_ROUTE_SX(buf) s_x[buf]
#include "ss2d_seq_route.h"                                             // ru, ry, cbyte, ucur, unext, tile_offsets, load_tile, store_x
#undef XP_SEQ_ROUTE_SX
    int offc, offn, offx;
    const int ntile = (L + SEQ_TP - 1) / SEQ_TP;
    tile_offsets(0, offc, offx);
    load_tile(offc, offx, ucur);
    store_x(0);
    float h = 0.f;
    for (int t = 0; t < ntile; ++t) {
        if (t + 1 < ntile) { tile_offsets(t + 1, offn, offx); load_tile(offn, offx, unext); }
        const float* sx = s_x[t & 1];
        float dtv[2][16];
        dt_tile<R, AMP>(dw, sx, RW, dtv);                               // dt of the tile on the matrix pipe
        // four steps at a time: their operand evaluation (softplus, exp) is independent and interleaves; only the h update is a chain
#pragma unroll
        for (int j0 = 0; j0 < SEQ_TP; j0 += 4) {
            float a[4], bb[4], cv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float2 bc = *reinterpret_cast<const float2*>(sx + (j0 + k) * RW + R);
                float delta;
                xp_softplus_decay_l2_nb(XP_DTV(dtv, j0 + k), Av, delta, a[k]);
                bb[k] = delta * bc.x * ucur[j0 + k];
                cv[k] = bc.y;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                h = a[k] * h + bb[k];
                const float y = cv[k] * h + Dv * ucur[j0 + k];          // y = C*h + D*u (csms6s.py:61,67)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y), ry, cbyte, __builtin_amdgcn_readlane(offc, j0 + k), 0);
            }
        }
        if (t + 1 < ntile) {
            store_x((t + 1) & 1);
#pragma unroll
            for (int j = 0; j < SEQ_TP; ++j) ucur[j] = unext[j];
            offc = offn;
        }
    }
}

// The same sequential recurrence PIPELINED OVER THE WAVES OF A WORKGROUP (round 4).  ss2d_seq_scan2 is one wave per (image, route, 64 channels): its time is the
// route's length — ~100 instructions per step of issue latency, 117 us for L = 1 200 whatever the batch — although only two of those instructions (h = a h + b,
// y = C h + D u) form the chain; the projection, softplus and exp of a step depend on nothing before it.  Here NW waves share the route: wave w takes the tiles
// w, w + NW, ... — loads, matrix-pipe dt projection and the (a, b, C, D u) of all 32 steps of its tile into registers, in parallel with the other waves' tiles —
// then waits for its turn (an LDS counter), takes the running state from LDS, runs the 32 chain steps + stores, and passes the state on.  The chain itself is the
// same instruction sequence in the same order (h = a * h + b; y = C * h + D u with the same operands), so the results are bit-identical to ss2d_seq_scan2;
// what changes is that the chain's length, not the evaluation's, sets the time.  All NW waves of a workgroup are resident together, so the turn wait cannot
// deadlock; a waiting wave sleeps (s_sleep) on a SIMD nobody else of the workgroup uses (a wave of another workgroup may: two are resident per SIMD).
template <int R, bool AMP, int NW>
__global__ __launch_bounds__(64 * NW) XP_SEQ_TWO_WAVES void ss2d_seq_scan3(SS2DParams p, float* __restrict__ ys) {
    constexpr int RW = R + 2, NP = RW / 2, NPL = (NP + 1) / 2;
    __shared__ __align__(16) float s_x[NW][2][SEQ_TP * RW];
    __shared__ float s_h[64];
    __shared__ int s_turn;
    const int lane = threadIdx.x & 63;
    int cg, d, b;
    seq_block_route(cg, d, b);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pair = d >> 1, back = d & 1;
    const int fr = lane & 31, fh = lane >> 5;
    const int L = p.H * p.W, XD = 4 * RW;
    const int c = cg * 64 + lane;
    if (threadIdx.x < 64) s_h[lane] = 0.f;
    if (threadIdx.x == 0) s_turn = 0;
    __syncthreads();
    DtWeights<R> dw;
    dt_load_weights<R, AMP>(dw, p.wdt + (int64_t)d * R * p.C, p.dtb + d * p.C, p.C, cg * 64);
    const float Av = XP_L2E * p.A[d * p.C + c], Dv = p.Dp[d * p.C + c];
#define XP_SEQ_ROUTE_SX(buf) s_x[wave][buf]
#include "ss2d_seq_route.h"
#undef XP_SEQ_ROUTE_SX
    int offc = 0, offn = 0, offx = 0;
    const int ntile = (L + SEQ_TP - 1) / SEQ_TP;
    if (wave < ntile) {
        tile_offsets(wave, offc, offx);
        load_tile(offc, offx, ucur);
        store_x(0);
    }
    int it = 0;
    for (int t = wave; t < ntile; t += NW, ++it) {
        if (t + NW < ntile) { tile_offsets(t + NW, offn, offx); load_tile(offn, offx, unext); }
        const float* sx = s_x[wave][it & 1];                            // (written and read by this wave only: LDS operations of a wave execute in order)
        // Only what the chain needs is held across the turn: a[], bb[] and the tile's u (C stays in the wave's LDS tile, D u is formed after the turn).
        float a[SEQ_TP], bb[SEQ_TP];
        {
            float dtv[2][16];
            dt_tile<R, AMP>(dw, sx, RW, dtv);
#pragma unroll
            for (int j = 0; j < SEQ_TP; ++j) {
                float delta;
                xp_softplus_decay_l2_nb(XP_DTV(dtv, j), Av, delta, a[j]);
                bb[j] = delta * sx[j * RW + R] * ucur[j];
            }
        }
        // (pin the tile's operand evaluation BEFORE the turn wait: they are pure arithmetic, which the compiler may otherwise sink past the wait, into the chain)
#pragma unroll
        for (int j = 0; j < SEQ_TP; ++j) asm volatile("" :: "v"(a[j]), "v"(bb[j]));
        // the next tile's xdbl rows go to the tile's other LDS buffer now (they were requested before the evaluation above, and that buffer was last read
        // before this iteration began), so that their registers are not held across the turn
        if (t + NW < ntile) store_x((it + 1) & 1);
        // my turn: every tile before t has passed its state on
        // (LDS only, and LDS operations of a wave execute in order: plain volatile accesses + compiler barriers.  An acquire / release pair at workgroup
        //  scope would also drain the wave's outstanding GLOBAL stores and prefetch loads — s_waitcnt vmcnt(0) — into the chain: measured 1.5x instead of 3x.
        //  The pointers carry the LDS address space: through a generic volatile pointer each of these accesses is a FLAT instruction followed by that
        //  same s_waitcnt vmcnt(0).)
        SeqLdsInt turn = (SeqLdsInt)&s_turn;
        SeqLdsFloat hst = (SeqLdsFloat)&s_h[lane];
        while (*turn != t) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
        float h = *hst;
        // the turn is the chain and nothing else: 32 dependent updates, h_j written over a[j]
#pragma unroll
        for (int j = 0; j < SEQ_TP; ++j) {
            h = a[j] * h + bb[j];
            a[j] = h;
        }
        *hst = h;
        asm volatile("" ::: "memory");
        *turn = t + 1;
        asm volatile("" ::: "memory");
        // off the turn, while the next wave runs its chain: y = C*h + D*u (csms6s.py:61,67) — C from this wave's own LDS tile (store_x above wrote the
        // tile's OTHER buffer) into the registers bb[] has left, D u the same rounded product as before, in place — and the 32 stores with their
        // v_readlane.  (The empty asm statements keep the products and the lane reads from being scheduled up into the turn: volatile asm statements stay
        // in program order.  D u has a loop of its own so that the compiler's packed multiplies pair neighbouring steps, not C h with D u of one step,
        // which needs h_j and u_j copied into a register pair.)
        float cv[SEQ_TP];
#pragma unroll
        for (int j = 0; j < SEQ_TP; ++j) cv[j] = sx[j * RW + R + 1];
        int offs = offc;
        asm volatile("" : "+v"(offs));
#pragma unroll
        for (int j = 0; j < SEQ_TP; ++j) asm volatile("" : "+v"(ucur[j]));
#pragma unroll
        for (int j = 0; j < SEQ_TP; ++j) ucur[j] = Dv * ucur[j];
#pragma unroll
        for (int j = 0; j < SEQ_TP; ++j) {
            const float y = cv[j] * a[j] + ucur[j];
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y), ry, cbyte, __builtin_amdgcn_readlane(offs, j), 0);
        }
        if (t + NW < ntile) {
#pragma unroll
            for (int j = 0; j < SEQ_TP; ++j) ucur[j] = unext[j];
            offc = offn;
        }
    }
}

// out[b][px][:] = LayerNorm_C((y0 + y2) + (y1 + y3)); one wave per pixel, the row held in registers (C <= 768)
template <typename OT = float>
__global__ __launch_bounds__(256) void ss2d_seq_merge_ln(SS2DParams p, const float* __restrict__ ys) {
    const int lane = threadIdx.x & 63;
    const int64_t M = (int64_t)p.Bn * p.H * p.W;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int64_t plane = M * p.C;
    float v[12];
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const int cc = q * 64 + lane;
        v[q] = 0.f;
        if (cc < p.C) {
            const float* y = ys + row * p.C + cc;
            v[q] = (y[0] + y[plane]) + (y[2 * plane] + y[3 * plane]);
            s += v[q];
        }
    }
    const float mean = xp_wave_sum(s) / (float)p.C;
    float q2 = 0.f;
#pragma unroll
    for (int q = 0; q < 12; ++q) if (q * 64 + lane < p.C) { const float dd = v[q] - mean; q2 = fmaf(dd, dd, q2); }
    const float rstd = 1.f / sqrtf(xp_wave_sum(q2) / (float)p.C + p.eps);
    if (std::is_same<OT, float>::value && p.out_p32) {
        // the two-plane image the ring GEMM (out_proj) loads by DMA: lane pairs own adjacent channels, so a wave stores whole 64-byte plane segments
        _Float16* prow = reinterpret_cast<_Float16*>(p.out) + row * p.C * 2;
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            const int cc = q * 64 + lane;
            if (cc < p.C) {
                const float o = (v[q] - mean) * rstd * p.ln_w[cc] + p.ln_b[cc];
                const _Float16 hi = (_Float16)o, lo = (_Float16)(o - (float)hi);
                _Float16* d = prow + (cc >> 5) * 64 + (cc & 31);
                d[0] = hi; d[32] = lo;
            }
        }
        return;
    }
    OT* orow = reinterpret_cast<OT*>(p.out) + row * p.C;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const int cc = q * 64 + lane;
        if (cc < p.C) orow[cc] = (OT)((v[q] - mean) * rstd * p.ln_w[cc] + p.ln_b[cc]);
    }
}

}  // namespace

// ss2d_seq_scan2 serves dt_rank >= 16 (whole 8-value fragment halves) while a plane's byte offsets fit the 32-bit buffer offsets
bool ss2d_seq_scan2_applies(int R, int H, int W, int C) {
    static const bool old_seq = getenv("XP_SS2D_SEQ_V1") && atoi(getenv("XP_SS2D_SEQ_V1")) != 0;      // A/B: first kernel (dt projection on the vector ALU)
    return !old_seq && R >= 16 && R % 8 == 0 && (int64_t)H * W * C < (1ll << 29) && (int64_t)H * W * 4 * (R + 2) < (1ll << 29);
}

namespace {

// THE table of the dt_rank >= 16 instances, [half_out][log2(NW)]: the occupancy query and the launch both read it
struct SeqInstance {
    void (*kernel)(SS2DParams, float*);
    int threads;
};
template <int R>
const SeqInstance& seq_instance(bool half_out, int k) {
    static const SeqInstance table[2][3] = {
        {{ss2d_seq_scan2<R, false>, 64}, {ss2d_seq_scan3<R, false, 2>, 128}, {ss2d_seq_scan3<R, false, 4>, 256}},
        {{ss2d_seq_scan2<R, true>, 64}, {ss2d_seq_scan3<R, true, 2>, 128}, {ss2d_seq_scan3<R, true, 4>, 256}}};
    return table[half_out ? 1 : 0][k];
}

// half_out: the fast mixed-precision class — u / xdbl are f32 COPIES of the half tensors (written beside them by their producers: the deep stages are
// small), the dt projection rounds like step_vals<R, AMP>, out is stored as fp16
template <int R>
int launch_ss2d_seq(const SS2DParams& p, float* ys, hipStream_t s, bool half_out) {
    const double MC = (double)p.Bn * p.H * p.W * p.C, MX = (double)p.Bn * p.H * p.W * 4 * (R + 2);
    const std::string sfx = xp_prof_by_shape() ? "_C" + std::to_string(p.C) : std::string();
    {   // every route reads u and its quarter of xdbl, writes its y
        XpProfScope prof(("ss2d_seq_scan" + sfx).c_str(), s, 4.0 * MC * (2.0 * R + 14.0), 4.0 * (8.0 * MC + MX));
        const bool v2 = ss2d_seq_scan2_applies(R, p.H, p.W, p.C);
        if constexpr (R >= 16 && R % 8 == 0) {
            // waves per route (ss2d_seq_scan3): XP_SS2D_SEQ_NW = 1 selects the one-wave kernel (bit-identical results)
            // As many waves per route as can all be RESIDENT: the largest NW of 4 / 2 / 1 with routes x NW <= (resident waves per SIMD of that instance) x
            // SIMDs.  Every dt_rank >= 16 instance fits two waves per SIMD (XP_SEQ_TWO_WAVES), so that is 2 x 1024 waves on an MI355X: NW = 4 up to 21 images
            // at C = 384 and 10 at C = 768, NW = 2 up to 42 / 21.  Waves that are not resident run as a second round of workgroups and only add turn waits.
            // Whole core (scan + merge), tools/ss2d_bench.py, us with NW = 1 / 2 / 4 — 16 images: C = 384 141 / 119 / 81, C = 768 54 / 49 / 50 (3072 waves: not
            // resident); 2 images: C = 384 114 / 71 / 45, C = 768 42 / 32 / 25 (profiles/ss2d_seq_occupancy.txt; forced NW = 2 at C = 384, 16 images, was 99 when the
            // register file kept its 768 waves one to a SIMD — where two may share one they now do; the rule never picks it there).
            // Bit-identical for every NW (tools/ss2d_bench.py prints the CRC, tests/test_gpu_ss2d_seq_bits.py holds the digests), so the choice may depend on the batch.
            static const int force_nw = getenv("XP_SS2D_SEQ_NW") ? atoi(getenv("XP_SS2D_SEQ_NW")) : 0;
            static int n_simd = 0;
            if (n_simd == 0) {
                int dev = 0, v = 0;
                if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
                n_simd = 4 * v;
            }
            // waves per SIMD that the runtime really keeps resident of each instance (NW = 1, 2, 4), asked once: registers and LDS as compiled, so a
            // build that misses the two-wave bound sizes NW for one wave instead of queueing a second round of workgroups
            static int resident[2][3] = {{0, 0, 0}, {0, 0, 0}};
            auto waves_per_simd = [&](int k) {                          // k = log2(NW)
                int& r = resident[half_out ? 1 : 0][k];
                if (r == 0) {
                    int nb = 0;
                    const SeqInstance& si = seq_instance<R>(half_out, k);
                    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, si.kernel, si.threads, 0);
                    const int w = e == hipSuccess ? (nb << k) / 4 : 1;  // workgroups per CU x NW waves over the CU's 4 SIMDs
                    r = w < 1 ? 1 : (w > SEQ_RESIDENT ? SEQ_RESIDENT : w);      // (more than two add nothing: two already fill the issue slots)
                }
                return r;
            };
            const dim3 grid(xp_cdiv(p.C, 64), 4, p.Bn);
            const int64_t routes = (int64_t)grid.x * grid.y * grid.z;
            const int nw = force_nw ? force_nw : (routes * 4 <= (int64_t)waves_per_simd(2) * n_simd ? 4 : (routes * 2 <= (int64_t)waves_per_simd(1) * n_simd ? 2 : 1));
            if (v2) {
                const SeqInstance& si = seq_instance<R>(half_out, nw == 4 ? 2 : (nw == 2 ? 1 : 0));     // (any other forced value: the one-wave kernel)
                hipLaunchKernelGGL(si.kernel, grid, dim3(si.threads), 0, s, p, ys);
            }
        }
        if (!v2) {
            if (half_out) { xp_set_error("xp_ss2d_core_fwd_f16: the sequential form needs dt_rank >= 16 (got %d)", R); return XP_ERR_ARG; }
            hipLaunchKernelGGL(ss2d_seq_scan<R>, dim3(xp_cdiv(p.C, 64), 4, p.Bn), dim3(64), 0, s, p, ys);
        }
    }
    {
        XpProfScope prof(("ss2d_seq_merge_ln" + sfx).c_str(), s, 12.0 * MC, 4.0 * 5.0 * MC);
        if (half_out) hipLaunchKernelGGL(ss2d_seq_merge_ln<_Float16>, dim3(xp_cdiv((int64_t)p.Bn * p.H * p.W, 4)), dim3(256), 0, s, p, ys);
        else hipLaunchKernelGGL(ss2d_seq_merge_ln<float>, dim3(xp_cdiv((int64_t)p.Bn * p.H * p.W, 4)), dim3(256), 0, s, p, ys);
    }
    XP_LAUNCH_CHECK();
    return XP_OK;
}

}  // namespace

int ss2d_launch_seq(const SS2DParams& p, float* ys, int R, bool half_out, hipStream_t s) {
    int rc = XP_ERR_ARG;
    SS2DRanks::dispatch(R, [&](auto r) { rc = launch_ss2d_seq<decltype(r)::value>(p, ys, s, half_out); });
    return rc;
}
