// The chunked three-pass form of the fused SS2D core (stages 0-1): pass 1 / pass 2 / pass 3 as described at the top of ss2d.hip, and their launch.
#include <string>

#include "ss2d_core.h"

namespace {

// Shared staging of one block's chunk(s): pixel indices and the xdbl rows of this route pair.
// UT: element type of u / xdbl / out in HBM — float, or _Float16 in the fast mixed-precision class (fp16 storage; every value is converted on load, and the
// conversion on the out_norm store IS the recipe's `y.to(x.dtype)`, VMamba.py:646)
// T: the chunk length (p.T; a power of two).  Pass 3 hands it in as a compile-time constant, so i / T is a shift there; XW and XD are template
// constants, so i / XW is a multiply by a reciprocal and the row offset a shift-and-add.  The image's row base and the pair's column offset are
// taken out of the per-element index.
template <int R, typename UT = float>
__device__ __forceinline__ void stage_chunk(const SS2DParams& p, int T, int b, int pair, int chunk0, int* s_pix, int* s_off, float* s_x) {
    const int L = p.H * p.W;
    const int npx = p.cpb * T;
    const int tsh = 31 - __builtin_clz(T);
    for (int i = threadIdx.x; i < npx; i += blockDim.x) {
        int cl = i >> tsh, ii = i - (cl << tsh);
        int chunk = chunk0 + cl;
        const int px = (chunk < p.nc) ? pixel_of((chunk << tsh) + ii, L, p.H, p.W, pair == 1) : -1;
        s_pix[i] = px;
        s_off[i] = px >= 0 ? px * p.C : -1;      // element offset of the pixel's row: the step loops address u / ya / out with it (no v_mul_lo_u32 per step)
    }
    __syncthreads();
    constexpr int XW = 2 * (R + 2);
    constexpr int XD = 2 * XW;
    const UT* xsrc = reinterpret_cast<const UT*>(p.xdbl) + (int64_t)b * L * XD + pair * XW;
    for (int i = threadIdx.x; i < npx * XW; i += blockDim.x) {
        int pi = i / XW, e = i - pi * XW;
        int px = s_pix[pi];
        s_x[i] = (px >= 0) ? (float)xsrc[(int64_t)px * XD + e] : 0.f;
    }
    __syncthreads();
}

// Pass 1's u of the four steps i0 .. i0 + 3 of chunk slot cl, for both of its branches: px = element offset of the pixel row, -1 past the end (loaded from the
// row start and zeroed); 32-bit offsets (host checks B*L*C < 2^31).  A macro: as a function the bounds-tested instances compiled to two instructions more.
#define XP_PASS1_LOAD_U4(uv)                                                                                            \
    int px[4];                                                                                                          \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                                     \
        px[k] = s_off[cl * p.T + i0 + k];                                                                               \
        const float t = (XP_SS2D_DBG & 8) ? 1.f : (float)ub[(FULL || px[k] >= 0) ? px[k] : 0];                          \
        uv[k] = (FULL || px[k] >= 0) ? t : 0.f;                                                                         \
    }

// FULL: every chunk of every block is complete (L % T == 0 and nc % cpb == 0 — all shapes of the 480 x 640 model): the per-step
// validity selects (compare + two cndmask per step) are compiled out
template <int R, bool FULL, bool AMP = false, typename UT = float>
__global__ __launch_bounds__(768) void ss2d_pass1(SS2DParams p) {
    constexpr float WL2E = AMP ? 1.f : XP_L2E;        // factor folded into the dt weights and bias where they are loaded (see step_vals)
    extern __shared__ __align__(16) char smem[];
    const int npx = p.cpb * p.T;
    int* s_pix = reinterpret_cast<int*>(smem);
    int* s_off = s_pix + npx;
    float* s_x = reinterpret_cast<float*>(smem + sizeof(int) * 2 * npx);
    constexpr int XW = 2 * (R + 2);
    const int b = blockIdx.y, pair = blockIdx.z, chunk0 = blockIdx.x * p.cpb;
    stage_chunk<R, UT>(p, p.T, b, pair, chunk0, s_pix, s_off, s_x);
    const int cl = threadIdx.x / p.C, c = threadIdx.x - cl * p.C;
    const int chunk = chunk0 + cl;
    if (chunk >= p.nc) return;
    const int L = p.H * p.W;
    const UT* ub = reinterpret_cast<const UT*>(p.u) + (int64_t)b * L * p.C + c;
    float P0 = 1.f, S0 = 0.f, Q1 = 1.f, S1 = 0.f;
    if constexpr (R < 16) {
        // small dt_rank (the wide, HBM-bound stages): both routes in one sweep over u
        float w0[R], w1[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            w0[r] = WL2E * p.wdt[((int64_t)(pair * 2 + 0) * R + r) * p.C + c];
            w1[r] = WL2E * p.wdt[((int64_t)(pair * 2 + 1) * R + r) * p.C + c];
        }
        const float b0 = WL2E * p.dtb[(pair * 2 + 0) * p.C + c], b1 = WL2E * p.dtb[(pair * 2 + 1) * p.C + c];
        const float A0 = XP_L2E * p.A[(pair * 2 + 0) * p.C + c], A1 = XP_L2E * p.A[(pair * 2 + 1) * p.C + c];
        for (int i0 = 0; i0 < p.T; i0 += 4) {
            float uv[4];
            XP_PASS1_LOAD_U4(uv)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // Pixels past the end of the last chunk run as u = 0 steps (their xdbl row is zero-filled): b = 0, and their
                // decay factor only reaches states that nobody reads (forward: after the last pixel; backward: multiplied
                // into the zero initial state), so no branch is needed.
                const float* xr = s_x + (cl * p.T + i0 + k) * XW;
                float a, bb, cv;
                step_vals<R, AMP>(xr, w0, b0, A0, uv[k], a, bb, cv);
                S0 = a * S0 + bb; P0 *= a;
                step_vals<R, AMP>(xr + (R + 2), w1, b1, A1, uv[k], a, bb, cv);
                S1 = fmaf(Q1, bb, S1); Q1 *= a;     // backward route accumulated in forward order
            }
        }
    } else {
    // large dt_rank: the two routes run one after the other so that only one route's R projection weights are live at a time: with
    // both (2R = 96 registers at C = 768) a 768-thread workgroup fills the CU's register file by itself and every
    // load latency is exposed.  u is re-read for the second route (L1 / L2 hits; these stages are small).
#pragma unroll 1
    for (int route = 0; route < 2; ++route) {
        float w[R];
#pragma unroll
        for (int r = 0; r < R; ++r) w[r] = WL2E * p.wdt[((int64_t)(pair * 2 + route) * R + r) * p.C + c];
        const float bias = WL2E * p.dtb[(pair * 2 + route) * p.C + c], Av = XP_L2E * p.A[(pair * 2 + route) * p.C + c];
        float Pr = 1.f, Sr = 0.f;
        for (int i0 = 0; i0 < p.T; i0 += 4) {
            float uv[4];
            XP_PASS1_LOAD_U4(uv)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // Pixels past the end of the last chunk run as u = 0 steps (their xdbl row is zero-filled): b = 0, and their
                // decay factor only reaches states that nobody reads (forward: after the last pixel; backward: multiplied
                // into the zero initial state), so no branch is needed.
                const float* xr = s_x + (cl * p.T + i0 + k) * XW + route * (R + 2);
                float a, bb, cv;
                step_vals<R, AMP>(xr, w, bias, Av, uv[k], a, bb, cv);
                if (route == 0) Sr = a * Sr + bb;
                else Sr = fmaf(Pr, bb, Sr);                 // backward route accumulated in forward order
                Pr *= a;
            }
        }
        if (route == 0) { P0 = Pr; S0 = Sr; } else { Q1 = Pr; S1 = Sr; }
    }
    }
    const int64_t o = ((((int64_t)b * 2 + pair) * p.nc + chunk) * 2) * p.C + c;
    p.wsP[o] = P0; p.wsS[o] = S0;
    p.wsP[o + p.C] = Q1; p.wsS[o + p.C] = S1;
}

// pass 2: carry over chunks, per (image, pair, direction, channel).  Two-level so that the sequential depth is
// ~2*nc/G + G instead of nc: G groups of consecutive chunks are composed in parallel, a short serial pass gives the
// state entering each group, then every group re-walks its chunks storing the state entering each chunk (over S).
#ifndef XP_SS2D_P2G
#define XP_SS2D_P2G 16
#endif
constexpr int P2_G = XP_SS2D_P2G;      // (-D override: tools/instep_ab.sh)
__global__ __launch_bounds__(64 * P2_G) void ss2d_pass2(SS2DParams p) {
    __shared__ float s_P[P2_G][64], s_S[P2_G][64];
    const int lane = threadIdx.x, g = threadIdx.y;
    const int c = blockIdx.x * 64 + lane;
    const int bp = blockIdx.y >> 1, dir = blockIdx.y & 1;    // bp = b*2 + pair
    const bool ok = c < p.C;
    const int per = (p.nc + P2_G - 1) / P2_G;
    const int j0 = g * per, j1 = min(p.nc, j0 + per);
    auto off = [&](int jj) -> int64_t {
        const int j = dir ? (p.nc - 1 - jj) : jj;
        return (((int64_t)bp * p.nc + j) * 2 + dir) * p.C + c;
    };
    float P = 1.f, S = 0.f;
    if (ok) {
        int jj = j0;
        for (; jj + 4 <= j1; jj += 4) {
            float Pv[4], Sv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int64_t o = off(jj + k); Pv[k] = p.wsP[o]; Sv[k] = p.wsS[o]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) { S = fmaf(Pv[k], S, Sv[k]); P *= Pv[k]; }
        }
        for (; jj < j1; ++jj) { const int64_t o = off(jj); const float Pj = p.wsP[o], Sj = p.wsS[o]; S = fmaf(Pj, S, Sj); P *= Pj; }
    }
    s_P[g][lane] = P; s_S[g][lane] = S;
    __syncthreads();
    float h = 0.f;
    for (int gg = 0; gg < g; ++gg) h = fmaf(s_P[gg][lane], h, s_S[gg][lane]);
    if (!ok) return;
    int jj = j0;
    for (; jj + 4 <= j1; jj += 4) {
        float Pv[4], Sv[4];
        int64_t ov[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { ov[k] = off(jj + k); Pv[k] = p.wsP[ov[k]]; Sv[k] = p.wsS[ov[k]]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { p.wsS[ov[k]] = h; h = fmaf(Pv[k], h, Sv[k]); }
    }
    for (; jj < j1; ++jj) { const int64_t o = off(jj); const float Pj = p.wsP[o], Sj = p.wsS[o]; p.wsS[o] = h; h = fmaf(Pj, h, Sj); }
}

// T: the chunk length (= p.T) as a compile-time constant.  A thread loads its chunk's T values of u ONCE, before the forward route, with all loads in
// flight together, and keeps them in registers: the backward route walks the same pixels and reuses them (it used to load them again, four
// 4-byte loads and a wait per four steps; in the column traversal consecutive steps are W * C * 4 bytes apart, so each was a fresh line).  The
// column pair fetches the row pair's partial sums in the same batch, so their latency hides behind the forward route; the row pair keeps its T
// sums in the registers u leaves and stores them after its last step, outside the dependent chain.  Values, addresses and the order of every
// floating-point operation are those of the step-by-step form.
// (COLPAIR stays the second template argument: bench.py tells the row and the column launch apart by the kernel name's first two arguments)
template <int R, bool COLPAIR, bool FULL, int T, bool AMP = false, typename UT = float>
__global__ __launch_bounds__(768) void ss2d_pass3(SS2DParams p) {
    constexpr float WL2E = AMP ? 1.f : XP_L2E;
    extern __shared__ __align__(16) char smem[];
    const int npx = p.cpb * T;
    int* s_pix = reinterpret_cast<int*>(smem);
    int* s_off = s_pix + npx;
    float* s_x = reinterpret_cast<float*>(smem + sizeof(int) * 2 * npx);
    constexpr int XW = 2 * (R + 2);
    float* s_y = s_x + npx * XW;   // [npx][C + 8]: the pad keeps the 16-lanes-per-pixel LayerNorm reads of 4 rows off the same banks
    const int SY = p.C + 8;
    const int pair = COLPAIR ? 1 : 0;
    const int b = blockIdx.y, chunk0 = blockIdx.x * p.cpb;
    stage_chunk<R, UT>(p, T, b, pair, chunk0, s_pix, s_off, s_x);
    const int cl = threadIdx.x / p.C, c = threadIdx.x - cl * p.C;
    const int chunk = chunk0 + cl;
    const int L = p.H * p.W;
    if (chunk < p.nc) {
        const int* so = s_off + cl * T;             // the chunk's pixel row offsets, -1 past the end
        const float* sx = s_x + cl * T * XW;
        float* sy = s_y + cl * T * SY + c;
        const UT* ub = reinterpret_cast<const UT*>(p.u) + (int64_t)b * L * p.C + c;
        const float* prev = COLPAIR ? (p.ya + (int64_t)b * L * p.C + c) : nullptr;
        float* dst = COLPAIR ? nullptr : (p.ya + (int64_t)b * L * p.C + c);
        // one route's projection weights live at a time (see pass 1)
        float w0[R];
#pragma unroll
        for (int r = 0; r < R; ++r) w0[r] = WL2E * p.wdt[((int64_t)(pair * 2 + 0) * R + r) * p.C + c];
        const float b0 = WL2E * p.dtb[(pair * 2 + 0) * p.C + c];
        const float A0 = XP_L2E * p.A[(pair * 2 + 0) * p.C + c];
        const float D0 = p.Dp[(pair * 2 + 0) * p.C + c];
        const int64_t o = ((((int64_t)b * 2 + pair) * p.nc + chunk) * 2) * p.C + c;
        float h = p.wsS[o];
        // the chunk's operands, once for both routes: T (column pair: 2 T) independent loads issued back to back, after the first route's
        // weights and in the order of their use (the memory counter retires in order: step i waits for u[i] only)
        float uv[T], pv[COLPAIR ? T : 1];
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const int off = so[i];
            const float t = (XP_SS2D_DBG & 8) ? 1.f : (float)ub[(FULL || off >= 0) ? off : 0];
            uv[i] = (FULL || off >= 0) ? t : 0.f;
            if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);      // eight 64-bit addresses at a time, not all T of them before the first load
        }
        if (COLPAIR) {
#pragma unroll
            for (int i = T - 1; i >= 0; --i) {
                const int off = so[i];
                pv[i] = (XP_SS2D_DBG & 2) ? 0.f : prev[(FULL || off >= 0) ? off : 0];
                if ((i & 7) == 0) __builtin_amdgcn_sched_barrier(0);
            }
        }
        // forward route.  Four steps at a time, as before: their operand evaluation (projection, softplus, exp) is independent and interleaves, only
        // the h update is a chain.  The loops are unrolled because the operands sit in registers; the scheduling barrier after each group keeps
        // the compiler from interleaving more steps than four (a few registers: 130 -> 126 in the fp16-storage column instance of stage 0, the
        // difference between three and four waves per SIMD).
        // A step works on a copy of its u (the empty asm): the compiler evaluates (delta B u, a h) and (D u, C h) as packed pairs with u and h in
        // an aligned register pair, and without the copy it gives every one of the T held values a pair of its own.
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i0 = 0; i0 < T; i0 += 4) {
#pragma unroll
            for (int i = i0; i < i0 + 4; ++i) {
                float a, bb, cv;
                float ui = uv[i];
                asm("" : "+v"(ui));
                step_vals<R, AMP>(sx + i * XW, w0, b0, A0, ui, a, bb, cv);
                h = a * h + bb;
                sy[i * SY] = cv * h + D0 * ui;      // y = C*h + D*u (csms6s.py:61,67); rows past the end are never read
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // backward route over the same pixels
        asm volatile("" ::: "memory");      // keep the second route's weight loads below the forward loop
        float w1[R];
#pragma unroll
        for (int r = 0; r < R; ++r) w1[r] = WL2E * p.wdt[((int64_t)(pair * 2 + 1) * R + r) * p.C + c];
        const float b1 = WL2E * p.dtb[(pair * 2 + 1) * p.C + c];
        const float A1 = XP_L2E * p.A[(pair * 2 + 1) * p.C + c];
        const float D1 = p.Dp[(pair * 2 + 1) * p.C + c];
        h = p.wsS[o + p.C];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i0 = T - 4; i0 >= 0; i0 -= 4) {
#pragma unroll
            for (int i = i0 + 3; i >= i0; --i) {
                float a, bb, cv;
                float ui = uv[i];
                asm("" : "+v"(ui));
                step_vals<R, AMP>(sx + i * XW + (R + 2), w1, b1, A1, ui, a, bb, cv);
                h = a * h + bb;                                      // u = 0 steps before the image's last pixel keep h = 0
                const float y2 = cv * h + D1 * ui;
                float tot = sy[i * SY] + y2;                       // y_fwd + flip(y_bwd)
                if (COLPAIR) sy[i * SY] = pv[i] + tot;            // (y0+y2) + (y1+y3)
                else {
                    // u of this step is done with: its register holds the sum until the stores below.  The asm pins the sum to its step: with no
                    // store in the loop the compiler otherwise sinks the whole h chain below it and carries every step's a, b, C and y_fwd there.
                    asm volatile("" : "+v"(tot));
                    uv[i] = tot;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!COLPAIR) {
            asm volatile("" ::: "memory");      // read the offsets again here: their T 64-bit store addresses are not carried through both routes
#pragma unroll
            for (int i = 0; i < T; ++i) {
                const int off = so[i];
                if (FULL || off >= 0) dst[off] = uv[i];
                if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (!COLPAIR) return;
    __syncthreads();
    if (XP_SS2D_DBG & 1) { if (threadIdx.x < 4) p.out[(int64_t)b * L * p.C + blockIdx.x * 4 + threadIdx.x] = s_y[threadIdx.x]; return; }
    // out_norm: LayerNorm over C per pixel (two-pass mean / variance).  Narrow stages (C <= 192): 16 lanes per pixel, four
    // pixels per wave — with a whole wave per pixel two thirds of the lanes idle at C = 96 and the two 6-step shuffle
    // reductions dominate (this part was a third of the column pass at stage 0).  Wide stages: one wave per pixel.
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    if (p.C <= 192) {
        // 8 lanes per pixel, eight pixels per wave; a lane owns the float4 chunks sub + 8 j (C / 32 <= 6 of them): the row is read from LDS
        // once (ds_read_b128), both reductions run on registers, every store instruction writes full 128-byte lines, and the out_norm
        // weights are loaded once per lane.  (The first form — 16 lanes per pixel, scalar elements, three LDS reads of the row and the
        // weights fetched per pixel — was 38 % of the column pass at stage 0.)
        const int sub = lane & 7, grp = lane >> 3;
        const int nj = p.C >> 5;
        const float invC = 1.f / (float)p.C;
        float4 gw[6], gb[6];
#pragma unroll
        for (int j = 0; j < 6; ++j)
            if (j < nj) {
                gw[j] = *reinterpret_cast<const float4*>(p.ln_w + 4 * (sub + 8 * j));
                gb[j] = *reinterpret_cast<const float4*>(p.ln_b + 4 * (sub + 8 * j));
            }
        for (int pi = wave * 8 + grp; pi < npx; pi += nw * 8) {      // an 8-lane group skips as a whole: the shuffles stay inside the group
            const int px = s_pix[pi];
            if (px < 0) continue;
            const float* row = s_y + pi * SY;
            float4 r[6];
            float sm = 0.f;
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if (j < nj) { r[j] = *reinterpret_cast<const float4*>(row + 4 * (sub + 8 * j)); sm += (r[j].x + r[j].y) + (r[j].z + r[j].w); }
            sm = xp_row8_sum(sm);
            const float mean = sm * invC;
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if (j < nj) {
                    const float dx = r[j].x - mean, dy = r[j].y - mean, dz = r[j].z - mean, dw = r[j].w - mean;
                    v = fmaf(dx, dx, v); v = fmaf(dy, dy, v); v = fmaf(dz, dz, v); v = fmaf(dw, dw, v);
                }
            v = xp_row8_sum(v);
            const float rstd = 1.f / sqrtf(v * invC + p.eps);
            UT* orow = reinterpret_cast<UT*>(p.out) + ((int64_t)b * L + px) * p.C;
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if (j < nj) {
                    float4 o;
                    o.x = (r[j].x - mean) * rstd * gw[j].x + gb[j].x; o.y = (r[j].y - mean) * rstd * gw[j].y + gb[j].y;
                    o.z = (r[j].z - mean) * rstd * gw[j].z + gb[j].z; o.w = (r[j].w - mean) * rstd * gw[j].w + gb[j].w;
                    if constexpr (std::is_same<UT, float>::value) *reinterpret_cast<float4*>(orow + 4 * (sub + 8 * j)) = o;
                    else {
                        union { _Float16 h[4]; uint2 u; } hh;
                        hh.h[0] = (_Float16)o.x; hh.h[1] = (_Float16)o.y; hh.h[2] = (_Float16)o.z; hh.h[3] = (_Float16)o.w;
                        *reinterpret_cast<uint2*>(orow + 4 * (sub + 8 * j)) = hh.u;
                    }
                }
        }
        return;
    }
    for (int pi = wave; pi < npx; pi += nw) {
        const int px = s_pix[pi];
        if (px < 0) continue;
        const float* row = s_y + pi * SY;
        float s = 0.f;
        for (int cc = lane; cc < p.C; cc += 64) s += row[cc];
        const float mean = xp_wave_sum(s) / (float)p.C;
        float v = 0.f;
        for (int cc = lane; cc < p.C; cc += 64) { float d = row[cc] - mean; v = fmaf(d, d, v); }
        const float rstd = 1.f / sqrtf(xp_wave_sum(v) / (float)p.C + p.eps);
        UT* orow = reinterpret_cast<UT*>(p.out) + ((int64_t)b * L + px) * p.C;
        for (int cc = lane; cc < p.C; cc += 64) orow[cc] = (UT)((row[cc] - mean) * rstd * p.ln_w[cc] + p.ln_b[cc]);
    }
}

// The kernels of one precision class: pass 1, and pass 3 by chunk length (a template constant there: the chunk's operands live in registers) and route pair
typedef void (*ChunkKernel)(SS2DParams);
struct ChunkKernels {
    ChunkKernel pass1;
    ChunkKernel pass3[3][2];                                            // [log2(T / 8)][COLPAIR]
};
template <int R, bool FULL, bool AMP, typename UT>
constexpr ChunkKernels chunk_kernels = {ss2d_pass1<R, FULL, AMP, UT>,
                                        {{ss2d_pass3<R, false, FULL, 8, AMP, UT>, ss2d_pass3<R, true, FULL, 8, AMP, UT>},
                                         {ss2d_pass3<R, false, FULL, 16, AMP, UT>, ss2d_pass3<R, true, FULL, 16, AMP, UT>},
                                         {ss2d_pass3<R, false, FULL, 32, AMP, UT>, ss2d_pass3<R, true, FULL, 32, AMP, UT>}}};
// THE choice of the precision class, once per call, from the table of the five classes.  full: the instances without bounds tests — which the
// f32-container mixed-precision class (amp) does not have: it runs the general (bounds-tested) instances with the dt rounding of step_vals
template <int R>
const ChunkKernels& chunk_class(bool half_io, bool amp, bool full) {
    static const ChunkKernels table[5] = {chunk_kernels<R, true, true, _Float16>, chunk_kernels<R, false, true, _Float16>, chunk_kernels<R, false, true, float>,
                                          chunk_kernels<R, true, false, float>, chunk_kernels<R, false, false, float>};
    return table[half_io ? (full ? 0 : 1) : (amp ? 2 : (full ? 3 : 4))];
}

template <int R>
int launch_ss2d(const SS2DParams& p, hipStream_t s, bool half_io) {
    constexpr int XW = 2 * (R + 2);
    const int npx = p.cpb * p.T;
    const int threads = p.cpb * p.C;
    const bool full = (p.H * p.W) % p.T == 0 && p.nc % p.cpb == 0;
    const ChunkKernels& k = chunk_class<R>(half_io, xp_amp_value() != 0, full);
    const int ti = p.T == 8 ? 0 : (p.T == 16 ? 1 : 2);
    const size_t sm1 = sizeof(int) * 2 * npx + sizeof(float) * npx * XW;
    const size_t sm3 = sm1 + sizeof(float) * (size_t)npx * (p.C + 8);
    dim3 grid1(xp_cdiv(p.nc, p.cpb), p.Bn, 2), grid3(xp_cdiv(p.nc, p.cpb), p.Bn, 1);
    const double MC = (double)p.Bn * p.H * p.W * p.C, MX = (double)p.Bn * p.H * p.W * XW;
    const std::string sfx = xp_prof_by_shape() ? "_C" + std::to_string(p.C) : std::string();
    const double el = 4.0 * MC;   // (pixel, channel, direction) scan elements of the whole core
    {   // reads u + its half of xdbl for each of the two route pairs
        XpProfScope prof(("ss2d_pass1" + sfx).c_str(), s, el * (2.0 * R + 12.0) / 2.0, 4.0 * 2.0 * (MC + MX));
        hipLaunchKernelGGL(k.pass1, grid1, dim3(threads), sm1, s, p);
    }
    {
        XpProfScope prof(("ss2d_pass2" + sfx).c_str(), s, 0.0, 4.0 * 3.0 * (double)p.Bn * 4 * p.nc * p.C);
        hipLaunchKernelGGL(ss2d_pass2, dim3(xp_cdiv(p.C, 64), p.Bn * 4), dim3(64, P2_G), 0, s, p);
    }
    {   // read u, xdbl half; write ya
        XpProfScope prof(("ss2d_pass3_row" + sfx).c_str(), s, el * (2.0 * R + 14.0) / 4.0, 4.0 * (2.0 * MC + MX));
        hipLaunchKernelGGL(k.pass3[ti][0], grid3, dim3(threads), sm3, s, p);
    }
    {   // read u, ya, xdbl half; write out (after out_norm)
        XpProfScope prof(("ss2d_pass3_col_ln" + sfx).c_str(), s, el * (2.0 * R + 14.0) / 4.0, 4.0 * (3.0 * MC + MX));
        hipLaunchKernelGGL(k.pass3[ti][1], grid3, dim3(threads), sm3, s, p);
    }
    XP_LAUNCH_CHECK();
    return XP_OK;
}

}  // namespace

int ss2d_launch_chunked(const SS2DParams& p, int R, bool half_io, hipStream_t s) {
    int rc = XP_ERR_ARG;
    SS2DRanks::dispatch(R, [&](auto r) { rc = launch_ss2d<decltype(r)::value>(p, s, half_io); });
    return rc;
}
