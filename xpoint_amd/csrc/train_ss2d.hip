// The SS2D core of VSS-block training in PIXEL layout (xpoint_amd/training/ops.py ss2d_core): the four-route selective scan
// (d_state 1) and its backward without a (B, 4, C, L) route tensor anywhere.  Inputs and outputs are rows of the (B, H, W) pixel grid, M = B H W:
// u (M, C), dtp (M, 4, C) the dt projection's output, B / C read out of the x_proj row through a pointer and two strides, A / Ds / dt_bias (4, C).
// Route k in the reference's order: 0 row-major, 1 column-major, 2 and 3 their reverses (pixel_of in ss2d_core.h is the walk).  Per sample, route k,
// channel c and step l along the route, m_l the pixel:
//     dl_l = softplus(dtp[m_l, k, c] + dt_bias[k, c])        a_l = exp(dl_l A[k, c])
//     h_l  = a_l h_{l-1} + dl_l Bv[m_l, k] u[m_l, c]         y_k[m_l, c] = Cv[m_l, k] h_l + D[k, c] u[m_l, c]
//     ym[m, c] = (y_0 + y_2) + (y_1 + y_3)                   (xp_cross_merge's order of additions)
// Backward, g_l = dym[m_l, c] Cv[m_l, k] + a_{l+1} g_{l+1} carried from right to left along the route as q_l = a_l g_l (the recurrence at the top of
// selective_scan_bwd.hip):
//     du[m, c]      = sum_k (g dl Bv + D dym)                ddl = g (h_{l-1} a_l A + Bv u)
//     ddtp[m, k, c] = ddl sigmoid(dtp + dt_bias)             ddt_bias[k, c] = sum_{b, l} ddtp
//     dBv[m, k]     = sum_c g dl u                           dCv[m, k] = sum_c dym h
//     dA[k, c]      = sum_{b, l} g h_{l-1} a_l dl            dD[k, c] = sum_{b, l} dym u
// softplus and exp(dl A) are xp_softplus_decay (xp_common.h), the definition selective_scan.hip's d_state-1 forward uses (linear above 20); the
// sigmoid is 1 / (1 + xp_exp_fast(-x)) as in selective_scan_bwd.hip.
//
// CDNA4 mapping.  lane = channel: every step of every route, the column-major ones included, reads and writes whole pixel rows (coalesced), and the
// step's B / C are wave-uniform.  A workgroup owns one chunk of T consecutive route steps of one sample and one route PAIR (k, k + 2: the same pixels
// walked both ways), all C channels.  Forward: pass 1 leaves the chunk's decay product P and its local end state per route, the carry kernel turns
// the local states into the state ENTERING each chunk, pass 3 re-walks the chunk from it; the row pair's launch writes y_0 + y_2 to ym and the column
// pair's launch, after it on the stream, adds y_1 + y_3 to what it reads there.  P and the entering states stay in the workspace: they are all the
// backward needs of the forward.  Backward: pass 1 leaves each chunk's local q (the same P carries it), the carry kernel walks the chunks the other
// way, pass 3 rebuilds h over the chunk into LDS (T x C floats per route), walks back with q, and adds the pair's du in registers; row pair, then
// column pair through du itself, as in the forward.  dBv / dCv: a wave sum per step (fixed lane order), the waves' sums added in wave order through
// LDS.  dA, dD and ddt_bias: per-thread sums over the chunk, one partial per (sample, chunk), added in (sample, chunk) order in f64 by two last
// kernels.  No atomics: two calls are bit-identical, and ym / du / ddtp / dbc of a sample do not depend on the other samples of the call.
// 32-bit element offsets into u / dtp (the host refuses batch L 4 C >= 2^31).
#include <string>

#include "ss2d_core.h"
#include "../../include/xpoint_hip.h"

namespace {

constexpr int kMaxChunk = 64;
constexpr int kMaxTC = 6144;        // chunk x C that pass 3 of the backward holds in LDS: two planes of T x C floats = 48 KiB (+ the wave sums: <= 2.5 KiB)

struct TsParams {
    const float* u; const float* dtp; const float* bc; const float* A; const float* Dv; const float* dtb; const float* dym;
    float* ym; float* du; float* ddtp; float* dbc;
    float* P; float* Hin; float* Q; float* part;      // workspace: (B, 4, nc, C) x 3, (B nc, 3, 4, C)
    double* tmp;                                      // workspace: (kRedSplit, 3, 4, C)
    int64_t bc_ld, bc_ks;                             // floats between the B / C pairs of two pixels, of two routes
    int Bn, H, W, C, L, T, nc;
};

__device__ __forceinline__ int ts_pixel(const TsParams& p, int b, int l, bool col) { return b * p.L + pixel_of(l, p.L, p.H, p.W, col); }
__device__ __forceinline__ int64_t ts_state(const TsParams& p, int b, int k, int chunk, int c) { return (((int64_t)b * 4 + k) * p.nc + chunk) * p.C + c; }

// ---- forward -------------------------------------------------------------------------------------------------------------------------------
// pass 1: per (chunk, sample, pair) and channel, both routes in one ascending sweep: the forward route's (P, S) by its recurrence, the reverse
// route's S = sum_i b_i prod_{j < i} a_j accumulated in ascending order
__global__ __launch_bounds__(1024) void ts_fwd_pass1(TsParams p) {
    const int c = threadIdx.x;
    if (c >= p.C) return;
    const int chunk = blockIdx.x, b = blockIdx.y, pair = blockIdx.z, k0 = pair, k1 = pair + 2, C = p.C;
    const int l0 = chunk * p.T, n = min(p.T, p.L - l0);
    const float* __restrict__ u = p.u; const float* __restrict__ dtp = p.dtp; const float* __restrict__ bc = p.bc;
    const float A0 = p.A[k0 * C + c], A1 = p.A[k1 * C + c], b0 = p.dtb[k0 * C + c], b1 = p.dtb[k1 * C + c];
    float P0 = 1.f, S0 = 0.f, P1 = 1.f, S1 = 0.f;
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
        const int m = ts_pixel(p, b, l0 + i, pair == 1);
        const float uv = u[m * C + c], t0 = dtp[(m * 4 + k0) * C + c] + b0, t1 = dtp[(m * 4 + k1) * C + c] + b1;
        const float B0 = bc[m * p.bc_ld + k0 * p.bc_ks], B1 = bc[m * p.bc_ld + k1 * p.bc_ks];
        float dl, a;
        xp_softplus_decay(t0, A0, dl, a);
        S0 = a * S0 + dl * B0 * uv; P0 *= a;
        xp_softplus_decay(t1, A1, dl, a);
        S1 = fmaf(P1, dl * B1 * uv, S1); P1 *= a;
    }
    const int64_t o0 = ts_state(p, b, k0, chunk, c), o1 = ts_state(p, b, k1, chunk, c);
    p.P[o0] = P0; p.Hin[o0] = S0; p.P[o1] = P1; p.Hin[o1] = S1;
}

// The carry over chunks, per (sample, route, channel): S (the chunk's local result) becomes the state entering the chunk, in the route's chunk
// order (routes 2 and 3 walk the chunks downwards); flip: the other way (the backward's q runs against the route).  Two levels, as ss2d_pass2 of the
// inference core: kCarryG groups of consecutive chunks compose in parallel, a short serial pass gives the state entering each group, then every group
// walks its chunks again and stores the entering states.  A workgroup owns 64 channels of one (sample, route).
constexpr int kCarryG = 16;
__global__ __launch_bounds__(64 * kCarryG) void ts_carry(const float* __restrict__ P, float* __restrict__ S, int nc, int C, int flip) {
    __shared__ float s_P[kCarryG][64], s_S[kCarryG][64];
    const int lane = threadIdx.x, g = threadIdx.y, ct = (C + 63) / 64;
    const int bk = blockIdx.x / ct, c = (blockIdx.x - bk * ct) * 64 + lane;
    const bool ok = c < C;
    const bool down = ((bk & 3) >= 2) != (flip != 0);
    const int per = (nc + kCarryG - 1) / kCarryG, j0 = min(nc, g * per), j1 = min(nc, j0 + per);
    auto off = [&](int jj) -> int64_t { return ((int64_t)bk * nc + (down ? nc - 1 - jj : jj)) * C + c; };
    float Pg = 1.f, Sg = 0.f;
    if (ok)
        for (int jj = j0; jj < j1; ++jj) { const int64_t o = off(jj); const float Pj = P[o], Sj = S[o]; Sg = fmaf(Pj, Sg, Sj); Pg *= Pj; }
    s_P[g][lane] = Pg; s_S[g][lane] = Sg;
    __syncthreads();
    float h = 0.f;
    for (int gg = 0; gg < g; ++gg) h = fmaf(s_P[gg][lane], h, s_S[gg][lane]);
    if (!ok) return;
    for (int jj = j0; jj < j1; ++jj) { const int64_t o = off(jj); const float Pj = P[o], Sj = S[o]; S[o] = h; h = fmaf(Pj, h, Sj); }
}

// pass 3: the chunk again from its entering states.  LDS: the forward route's y per step, T x C floats (a thread reads back only what it wrote)
template <bool COL>
__global__ __launch_bounds__(1024) void ts_fwd_pass3(TsParams p) {
    extern __shared__ __align__(16) float ts_smem[];
    const int c = threadIdx.x;
    if (c >= p.C) return;
    const int chunk = blockIdx.x, b = blockIdx.y, k0 = COL ? 1 : 0, k1 = k0 + 2, C = p.C;
    const int l0 = chunk * p.T, n = min(p.T, p.L - l0);
    const float* __restrict__ u = p.u; const float* __restrict__ dtp = p.dtp; const float* __restrict__ bc = p.bc;
    float* sy = ts_smem + c;
    {
        const float Ak = p.A[k0 * C + c], bk = p.dtb[k0 * C + c], Dk = p.Dv[k0 * C + c];
        float h = p.Hin[ts_state(p, b, k0, chunk, c)];
#pragma unroll 4
        for (int i = 0; i < n; ++i) {
            const int m = ts_pixel(p, b, l0 + i, COL);
            const float uv = u[m * C + c], t = dtp[(m * 4 + k0) * C + c] + bk;
            const float Bv = bc[m * p.bc_ld + k0 * p.bc_ks], Cv = bc[m * p.bc_ld + k0 * p.bc_ks + 1];
            float dl, a;
            xp_softplus_decay(t, Ak, dl, a);
            h = a * h + dl * Bv * uv;
            sy[i * C] = Cv * h + Dk * uv;
        }
    }
    const float Ak = p.A[k1 * C + c], bk = p.dtb[k1 * C + c], Dk = p.Dv[k1 * C + c];
    float h = p.Hin[ts_state(p, b, k1, chunk, c)];
#pragma unroll 4
    for (int i = n - 1; i >= 0; --i) {
        const int m = ts_pixel(p, b, l0 + i, COL);
        const float uv = u[m * C + c], t = dtp[(m * 4 + k1) * C + c] + bk;
        const float Bv = bc[m * p.bc_ld + k1 * p.bc_ks], Cv = bc[m * p.bc_ld + k1 * p.bc_ks + 1];
        float dl, a;
        xp_softplus_decay(t, Ak, dl, a);
        h = a * h + dl * Bv * uv;
        const float tot = sy[i * C] + (Cv * h + Dk * uv);           // y_k + y_{k + 2}
        p.ym[m * C + c] = COL ? p.ym[m * C + c] + tot : tot;        // (y_0 + y_2) + (y_1 + y_3)
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------------
// pass 1: each chunk's local q = a (q' + dym Cv) with nothing entering, per route: the forward route's q runs downwards and is accumulated in
// ascending order (q_0 = sum_i dym_i Cv_i prod_{j <= i} a_j), the reverse route's runs upwards
__global__ __launch_bounds__(1024) void ts_bwd_pass1(TsParams p) {
    const int c = threadIdx.x;
    if (c >= p.C) return;
    const int chunk = blockIdx.x, b = blockIdx.y, pair = blockIdx.z, k0 = pair, k1 = pair + 2, C = p.C;
    const int l0 = chunk * p.T, n = min(p.T, p.L - l0);
    const float* __restrict__ dtp = p.dtp; const float* __restrict__ bc = p.bc; const float* __restrict__ dym = p.dym;
    const float A0 = p.A[k0 * C + c], A1 = p.A[k1 * C + c], b0 = p.dtb[k0 * C + c], b1 = p.dtb[k1 * C + c];
    float P0 = 1.f, Q0 = 0.f, Q1 = 0.f;
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
        const int m = ts_pixel(p, b, l0 + i, pair == 1);
        const float dy = dym[m * C + c], t0 = dtp[(m * 4 + k0) * C + c] + b0, t1 = dtp[(m * 4 + k1) * C + c] + b1;
        const float C0 = bc[m * p.bc_ld + k0 * p.bc_ks + 1], C1 = bc[m * p.bc_ld + k1 * p.bc_ks + 1];
        float dl, a;
        xp_softplus_decay(t0, A0, dl, a);
        P0 *= a; Q0 = fmaf(P0, dy * C0, Q0);
        xp_softplus_decay(t1, A1, dl, a);
        Q1 = a * (Q1 + dy * C1);
    }
    p.Q[ts_state(p, b, k0, chunk, c)] = Q0;
    p.Q[ts_state(p, b, k1, chunk, c)] = Q1;
}

struct TsSums { float A, D, B; };
// One step of the walk back: q = a_{l+1} g_{l+1} on entry, a_l g_l on exit; hp = h_{l-1}, h = h_l.  Returns the route's share of du.
__device__ __forceinline__ float ts_bwd_step(float u, float t, float dy, float Bv, float Cv, float Ak, float Dk, float hp, float h, float& q, TsSums& s,
                                             float& ddt, float& pB, float& pC) {
    float dl, a;
    xp_softplus_decay(t, Ak, dl, a);
    const float g = dy * Cv + q;
    const float gh = g * hp * a;
    const float ddl = gh * Ak + g * Bv * u;
    ddt = ddl / (1.f + xp_exp_fast(-t));
    s.A += gh * dl; s.D += dy * u; s.B += ddt;
    pB = g * dl * u; pC = dy * h;
    q = a * g;
    return g * dl * Bv + Dk * dy;
}

// pass 3.  LDS: s_h (T x C) the route's h per step, s_du (T x C) the first route's share of du, s_red (waves x T x 4) the waves' dBv / dCv sums.
// A thread reads back only its own column of s_h / s_du; lanes past C (the last wave's) take part in the wave sums with zeros and touch no memory.
template <bool COL>
__global__ __launch_bounds__(1024) void ts_bwd_pass3(TsParams p) {
    extern __shared__ __align__(16) float ts_smem[];
    const int C = p.C, T = p.T;
    const int c = threadIdx.x, wave = c >> 6, lane = c & 63, nw = blockDim.x >> 6;
    const bool valid = c < C;
    float* s_h = ts_smem + c; float* s_du = ts_smem + T * C + c; float* s_red = ts_smem + 2 * T * C;
    const int chunk = blockIdx.x, b = blockIdx.y, k0 = COL ? 1 : 0, k1 = k0 + 2;
    const int l0 = chunk * T, n = min(T, p.L - l0);
    const float* __restrict__ u = p.u; const float* __restrict__ dtp = p.dtp; const float* __restrict__ bc = p.bc; const float* __restrict__ dym = p.dym;
    float* __restrict__ ddtp = p.ddtp;
    TsSums s0 = {0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f};
    float Ak = 0.f, bk = 0.f, Dk = 0.f, hin = 0.f, q = 0.f;
    // ---- route k0: h upwards into LDS, then the walk back downwards
    if (valid) {
        Ak = p.A[k0 * C + c]; bk = p.dtb[k0 * C + c]; Dk = p.Dv[k0 * C + c];
        const int64_t o = ts_state(p, b, k0, chunk, c);
        hin = p.Hin[o]; q = p.Q[o];
        float h = hin;
#pragma unroll 4
        for (int i = 0; i < n; ++i) {
            const int m = ts_pixel(p, b, l0 + i, COL);
            const float uv = u[m * C + c], t = dtp[(m * 4 + k0) * C + c] + bk, Bv = bc[m * p.bc_ld + k0 * p.bc_ks];
            float dl, a;
            xp_softplus_decay(t, Ak, dl, a);
            h = a * h + dl * Bv * uv;
            s_h[i * C] = h;
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        float pB = 0.f, pC = 0.f;
        if (valid) {
            const int m = ts_pixel(p, b, l0 + i, COL);
            const float uv = u[m * C + c], t = dtp[(m * 4 + k0) * C + c] + bk, dy = dym[m * C + c];
            const float Bv = bc[m * p.bc_ld + k0 * p.bc_ks], Cv = bc[m * p.bc_ld + k0 * p.bc_ks + 1];
            const float h = s_h[i * C], hp = i > 0 ? s_h[(i - 1) * C] : hin;
            float ddt;
            s_du[i * C] = ts_bwd_step(uv, t, dy, Bv, Cv, Ak, Dk, hp, h, q, s0, ddt, pB, pC);
            ddtp[(m * 4 + k0) * C + c] = ddt;
        }
        pB = xp_wave_sum(pB); pC = xp_wave_sum(pC);
        if (lane == 0) { s_red[(wave * T + i) * 4 + 0] = pB; s_red[(wave * T + i) * 4 + 1] = pC; }
    }
    // ---- route k1: h downwards into LDS, then the walk back upwards; the pair's du leaves here
    if (valid) {
        Ak = p.A[k1 * C + c]; bk = p.dtb[k1 * C + c]; Dk = p.Dv[k1 * C + c];
        const int64_t o = ts_state(p, b, k1, chunk, c);
        hin = p.Hin[o]; q = p.Q[o];
        float h = hin;
#pragma unroll 4
        for (int i = n - 1; i >= 0; --i) {
            const int m = ts_pixel(p, b, l0 + i, COL);
            const float uv = u[m * C + c], t = dtp[(m * 4 + k1) * C + c] + bk, Bv = bc[m * p.bc_ld + k1 * p.bc_ks];
            float dl, a;
            xp_softplus_decay(t, Ak, dl, a);
            h = a * h + dl * Bv * uv;
            s_h[i * C] = h;
        }
    }
    for (int i = 0; i < n; ++i) {
        float pB = 0.f, pC = 0.f;
        if (valid) {
            const int m = ts_pixel(p, b, l0 + i, COL);
            const float uv = u[m * C + c], t = dtp[(m * 4 + k1) * C + c] + bk, dy = dym[m * C + c];
            const float Bv = bc[m * p.bc_ld + k1 * p.bc_ks], Cv = bc[m * p.bc_ld + k1 * p.bc_ks + 1];
            const float h = s_h[i * C], hp = i + 1 < n ? s_h[(i + 1) * C] : hin;
            float ddt;
            const float tot = s_du[i * C] + ts_bwd_step(uv, t, dy, Bv, Cv, Ak, Dk, hp, h, q, s1, ddt, pB, pC);
            ddtp[(m * 4 + k1) * C + c] = ddt;
            p.du[m * C + c] = COL ? p.du[m * C + c] + tot : tot;       // (k = 0, 2) + (k = 1, 3), the order of ym's additions
        }
        pB = xp_wave_sum(pB); pC = xp_wave_sum(pC);
        if (lane == 0) { s_red[(wave * T + i) * 4 + 2] = pB; s_red[(wave * T + i) * 4 + 3] = pC; }
    }
    if (valid) {
        float* part = p.part + ((int64_t)b * p.nc + chunk) * 12 * C + c;
        part[(0 * 4 + k0) * C] = s0.A; part[(1 * 4 + k0) * C] = s0.D; part[(2 * 4 + k0) * C] = s0.B;
        part[(0 * 4 + k1) * C] = s1.A; part[(1 * 4 + k1) * C] = s1.D; part[(2 * 4 + k1) * C] = s1.B;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n * 4; idx += blockDim.x) {
        const int i = idx >> 2, j = idx & 3;
        float s = 0.f;
        for (int w = 0; w < nw; ++w) s += s_red[(w * T + i) * 4 + j];
        const int m = ts_pixel(p, b, l0 + i, COL);
        p.dbc[((int64_t)m * 4 + (j < 2 ? k0 : k1)) * 2 + (j & 1)] = s;
    }
}

// dA, dD, ddt_bias (4, C) each: the (sample, chunk) partials in order, f64, in two steps: kRedSplit consecutive groups of rows each to one f64 sum,
// then the groups in order
constexpr int kRedSplit = 32;
__global__ __launch_bounds__(256) void ts_reduce_rows(const float* __restrict__ part, double* __restrict__ tmp, int rows, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x, sp = blockIdx.y;
    if (j >= n) return;
    const int per = (rows + kRedSplit - 1) / kRedSplit, r0 = min(rows, sp * per), r1 = min(rows, r0 + per);
    double acc = 0.0;
    for (int r = r0; r < r1; ++r) acc += (double)part[(int64_t)r * n + j];
    tmp[(int64_t)sp * n + j] = acc;
}
__global__ __launch_bounds__(256) void ts_reduce_params(const double* __restrict__ tmp, float* __restrict__ dA, float* __restrict__ dD,
                                                        float* __restrict__ ddb, int C) {
    const int j = blockIdx.x * 256 + threadIdx.x, n = 12 * C;
    if (j >= n) return;
    double t = 0.0;
    for (int sp = 0; sp < kRedSplit; ++sp) t += tmp[(int64_t)sp * n + j];
    const int which = j / (4 * C), e = j - which * 4 * C;
    (which == 0 ? dA : (which == 1 ? dD : ddb))[e] = (float)t;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
bool ts_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
// THE chunk length of a call: the caller's (a power of two in [2, 64] with chunk x C <= 6144), or for 0 the library's (16, 8 or 4: at most 12 KiB of
// LDS planes per workgroup up to C = 192, 24 KiB above); -1: not accepted
int ts_chunk(int C, int chunk) {
    if (chunk == 0) return C <= 128 ? 16 : (C <= 512 ? 8 : 4);      // by width, from the measurement at the four training widths
    return (ts_pow2(chunk) && chunk >= 2 && chunk <= kMaxChunk && (int64_t)chunk * C <= kMaxTC) ? chunk : -1;
}
bool ts_shape_ok(int batch, int H, int W, int C) { return batch > 0 && batch <= 65535 && H > 0 && W > 0 && C > 0 && C <= 1024; }

struct TsLayout { size_t P, Hin, Q, part, tmp, total; int T, nc; };
TsLayout ts_layout(int batch, int H, int W, int C, int T) {
    TsLayout w;
    w.T = T; w.nc = xp_cdiv((int64_t)H * W, T);
    const size_t st = xp_up256(sizeof(float) * (size_t)batch * 4 * w.nc * C);
    w.P = 0; w.Hin = st; w.Q = 2 * st; w.part = 3 * st;
    w.tmp = w.part + xp_up256(sizeof(float) * (size_t)batch * w.nc * 12 * C);
    w.total = w.tmp + xp_up256(sizeof(double) * (size_t)kRedSplit * 12 * C);
    return w;
}

void ts_fill(TsParams& p, const TsLayout& w, void* workspace, int batch, int H, int W, int C) {
    char* ws = static_cast<char*>(workspace);
    p.P = reinterpret_cast<float*>(ws + w.P); p.Hin = reinterpret_cast<float*>(ws + w.Hin); p.Q = reinterpret_cast<float*>(ws + w.Q);
    p.part = reinterpret_cast<float*>(ws + w.part); p.tmp = reinterpret_cast<double*>(ws + w.tmp);
    p.Bn = batch; p.H = H; p.W = W; p.C = C; p.L = H * W; p.T = w.T; p.nc = w.nc;
}

}  // namespace

extern "C" size_t xp_ss2d_train_workspace_bytes(int batch, int H, int W, int C, int chunk) {
    if (!ts_shape_ok(batch, H, W, C) || (int64_t)batch * H * W * 4 * C >= ((int64_t)1 << 31)) return 0;
    const int T = ts_chunk(C, chunk);
    return T < 0 ? 0 : ts_layout(batch, H, W, C, T).total;
}

#define XP_TS_COMMON_CHECKS(who)                                                                                                                    \
    XP_CHECK_ARG(dstate == 1, who ": d_state 1 only (got %d)", dstate);                                                                             \
    XP_CHECK_ARG(ts_shape_ok(batch, H, W, C), who ": batch in [1, 65535], H, W >= 1 and C in [1, 1024] (got %d, %d, %d, %d)", batch, H, W, C);      \
    XP_CHECK_ARG((int64_t)batch * H * W * 4 * C < ((int64_t)1 << 31), who ": batch H W 4 C must stay below 2^31 (32-bit element offsets)");         \
    const int T = ts_chunk(C, chunk);                                                                                                               \
    XP_CHECK_ARG(T > 0, who ": chunk must be 0 or a power of two in [2, %d] with chunk x C <= %d (got %d at C = %d)", kMaxChunk, kMaxTC, chunk, C); \
    XP_CHECK_ARG(bc_ld >= 2 && bc_kstride >= 2, who ": the B / C strides must be at least 2 floats (got %lld, %lld)", (long long)bc_ld,             \
                 (long long)bc_kstride);                                                                                                            \
    const TsLayout w = ts_layout(batch, H, W, C, T);                                                                                                \
    XP_CHECK_ARG(workspace && workspace_bytes >= w.total, who ": workspace of %zu bytes needed (got %zu)", w.total, workspace_bytes);               \
    XP_CHECK_ARG(((uintptr_t)workspace & 255) == 0, who ": workspace must be 256-byte aligned")

extern "C" int xp_ss2d_train_fwd(const float* u, const float* dtp, const float* bc, int64_t bc_ld, int64_t bc_kstride, const float* A, const float* Ds,
                                 const float* dt_bias, float* ym, void* workspace, size_t workspace_bytes, int batch, int H, int W, int C, int dstate,
                                 int chunk, void* stream) {
    XP_CHECK_ARG(u && dtp && bc && A && Ds && dt_bias && ym, "xp_ss2d_train_fwd: null tensor pointer");
    XP_TS_COMMON_CHECKS("xp_ss2d_train_fwd");
    hipStream_t s = (hipStream_t)stream;
    TsParams p = {};
    p.u = u; p.dtp = dtp; p.bc = bc; p.bc_ld = bc_ld; p.bc_ks = bc_kstride; p.A = A; p.Dv = Ds; p.dtb = dt_bias; p.ym = ym;
    ts_fill(p, w, workspace, batch, H, W, C);
    const int threads = xp_cdiv(C, 64) * 64;
    const double MC = (double)batch * H * W * C, MK = (double)batch * H * W * 4, ST = (double)batch * 4 * w.nc * C;
    const std::string sfx = xp_prof_by_shape() ? "_C" + std::to_string(C) : std::string();
    {   // reads u, dtp, B; writes P, S
        XpProfScope prof(("ss2d_train_fwd_pass1" + sfx).c_str(), s, 4.0 * MC * 16.0, 4.0 * (5.0 * MC + MK + 2.0 * ST));
        hipLaunchKernelGGL(ts_fwd_pass1, dim3(w.nc, batch, 2), dim3(threads), 0, s, p);
    }
    {
        XpProfScope prof(("ss2d_train_carry" + sfx).c_str(), s, 2.0 * ST, 4.0 * 3.0 * ST);
        hipLaunchKernelGGL(ts_carry, dim3(batch * 4 * xp_cdiv(C, 64)), dim3(64, kCarryG), 0, s, p.P, p.Hin, w.nc, C, 0);
    }
    const size_t sm = sizeof(float) * (size_t)T * C;
    {   // reads u, half of dtp and of B / C, the entering states; writes ym
        XpProfScope prof(("ss2d_train_fwd_pass3_row" + sfx).c_str(), s, 2.0 * MC * 20.0, 4.0 * (4.0 * MC + MK + 0.5 * ST));
        hipLaunchKernelGGL(ts_fwd_pass3<false>, dim3(w.nc, batch), dim3(threads), sm, s, p);
    }
    {   // the same, and ym once more
        XpProfScope prof(("ss2d_train_fwd_pass3_col" + sfx).c_str(), s, 2.0 * MC * 20.0, 4.0 * (5.0 * MC + MK + 0.5 * ST));
        hipLaunchKernelGGL(ts_fwd_pass3<true>, dim3(w.nc, batch), dim3(threads), sm, s, p);
    }
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_ss2d_train_bwd(const float* u, const float* dtp, const float* bc, int64_t bc_ld, int64_t bc_kstride, const float* A, const float* Ds,
                                 const float* dt_bias, const float* dym, float* du, float* ddtp, float* dbc, float* dA, float* dD, float* ddt_bias,
                                 void* workspace, size_t workspace_bytes, int batch, int H, int W, int C, int dstate, int chunk, void* stream) {
    XP_CHECK_ARG(u && dtp && bc && A && Ds && dt_bias && dym && du && ddtp && dbc && dA && dD && ddt_bias, "xp_ss2d_train_bwd: null tensor pointer");
    XP_TS_COMMON_CHECKS("xp_ss2d_train_bwd");
    hipStream_t s = (hipStream_t)stream;
    TsParams p = {};
    p.u = u; p.dtp = dtp; p.bc = bc; p.bc_ld = bc_ld; p.bc_ks = bc_kstride; p.A = A; p.Dv = Ds; p.dtb = dt_bias; p.dym = dym;
    p.du = du; p.ddtp = ddtp; p.dbc = dbc;
    ts_fill(p, w, workspace, batch, H, W, C);
    const int threads = xp_cdiv(C, 64) * 64;
    const double MC = (double)batch * H * W * C, MK = (double)batch * H * W * 4, ST = (double)batch * 4 * w.nc * C;
    const std::string sfx = xp_prof_by_shape() ? "_C" + std::to_string(C) : std::string();
    {   // reads dym, dtp, C; writes the local q
        XpProfScope prof(("ss2d_train_bwd_pass1" + sfx).c_str(), s, 4.0 * MC * 14.0, 4.0 * (5.0 * MC + MK + ST));
        hipLaunchKernelGGL(ts_bwd_pass1, dim3(w.nc, batch, 2), dim3(threads), 0, s, p);
    }
    {
        XpProfScope prof(("ss2d_train_carry" + sfx).c_str(), s, 2.0 * ST, 4.0 * 3.0 * ST);
        hipLaunchKernelGGL(ts_carry, dim3(batch * 4 * xp_cdiv(C, 64)), dim3(64, kCarryG), 0, s, p.P, p.Q, w.nc, C, 1);
    }
    const size_t sm = sizeof(float) * ((size_t)2 * T * C + (size_t)(threads / 64) * T * 4);
    {   // reads u, dym, half of dtp and of B / C, the states; writes half of ddtp and of dbc, du
        XpProfScope prof(("ss2d_train_bwd_pass3_row" + sfx).c_str(), s, 2.0 * MC * 60.0, 4.0 * (7.0 * MC + 2.0 * MK + ST));
        hipLaunchKernelGGL(ts_bwd_pass3<false>, dim3(w.nc, batch), dim3(threads), sm, s, p);
    }
    {   // the same, and du once more
        XpProfScope prof(("ss2d_train_bwd_pass3_col" + sfx).c_str(), s, 2.0 * MC * 60.0, 4.0 * (8.0 * MC + 2.0 * MK + ST));
        hipLaunchKernelGGL(ts_bwd_pass3<true>, dim3(w.nc, batch), dim3(threads), sm, s, p);
    }
    {
        XpProfScope prof(("ss2d_train_reduce" + sfx).c_str(), s, 0.0, 4.0 * 12.0 * C * ((double)batch * w.nc + 1.0));
        hipLaunchKernelGGL(ts_reduce_rows, dim3(xp_cdiv(12 * C, 256), kRedSplit), dim3(256), 0, s, p.part, p.tmp, batch * w.nc, 12 * C);
        hipLaunchKernelGGL(ts_reduce_params, dim3(xp_cdiv(12 * C, 256)), dim3(256), 0, s, p.tmp, dA, dD, ddt_bias, C);
    }
    XP_LAUNCH_CHECK();
    return XP_OK;
}
