// Box NMS on the heat map, exact, in two forms (which shape takes which: xp_box_nms_plan), and keep_top_k.
//   box_nms            reference xpoint/utils/utils.py:148-192  (torchvision.ops.nms / batched_nms)
// The fixed-point formulation, the priority rule and everything else the two forms share are in nms_core.h.
// Tiles of 32x32 pixels with a halo iterate locally in LDS; launches repeat until no pixel in the batch is undecided (device counter).
#include <stdlib.h>

#include <array>

#include "nms_core.h"

namespace {

enum : int { ST_NONE = 0, ST_UNDECIDED = 1, ST_KEPT = 2 };

// One sweep over every active 32x32 tile.  Tile state lives in LDS as per-row 64-bit masks (undecided / kept)
// plus the scores; the owned undecided candidates are compacted into a list so that lanes work on candidates,
// not pixels.  A candidate's test is 2R+1 mask tests for a kept neighbour and a walk over the set bits of the
// undecided neighbours (few) for the priority test.
//   first != 0: states are derived from prob (> min_prob) instead of being read; every tile is active.
//   sweep k > 0 exits at once when sweep k-1 left nothing undecided, and skips tiles with no undecided pixel.
// Each active tile writes its owned part of `out` (kept ? score : 0) and of `state`.
__global__ __launch_bounds__(256) void nms_sweep_kernel(const float* __restrict__ prob, uint8_t* __restrict__ state,
                                                        float* __restrict__ out, uint8_t* __restrict__ tile_active, int H, int W,
                                                        NmsTable tab, float min_prob, int* __restrict__ counters, int sweep,
                                                        int first, int local_iters) {
    if (sweep > 0 && counters[sweep - 1] == 0) return;   // converged in an earlier sweep (uniform early exit)
    const int tile_id = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (!first && !tile_active[tile_id]) return;
    constexpr int TWMAX = NMS_TILE + 2 * NMS_MAXR, THMAX = NMS_TH + 2 * NMS_MAXR;
    __shared__ float s_sc[TWMAX * THMAX];
    __shared__ unsigned long long m_und[THMAX], m_kept[THMAX];
    __shared__ unsigned short s_list[NMS_TILE * NMS_TH];
    __shared__ int s_n, s_changed;
    const int R = tab.reach;
    const int TW = NMS_TILE + 2 * R, TH = NMS_TH + 2 * R;
    const int b = blockIdx.z;
    const int y0 = blockIdx.y * NMS_TH - R, x0 = blockIdx.x * NMS_TILE - R;
    const float* pb = prob + (int64_t)b * H * W;
    uint8_t* sb = state + (int64_t)b * H * W;
    float* ob = out + (int64_t)b * H * W;
    for (int i = threadIdx.x; i < TH; i += 256) { m_und[i] = 0ull; m_kept[i] = 0ull; }
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < TW * TH; i += 256) {
        const int ty = i / TW, tx = i - ty * TW;
        const int y = y0 + ty, x = x0 + tx;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const float sc = in ? pb[(int64_t)y * W + x] : 0.f;
        int st = ST_NONE;
        if (in) st = first ? (sc > min_prob ? ST_UNDECIDED : ST_NONE) : sb[(int64_t)y * W + x];
        s_sc[i] = sc;
        if (st == ST_UNDECIDED) {
            atomicOr(&m_und[ty], 1ull << tx);
            const bool own = ty >= R && ty < R + NMS_TH && tx >= R && tx < R + NMS_TILE;
            if (own) { const int pos = atomicAdd(&s_n, 1); s_list[pos] = (unsigned short)(ty * 64 + tx); }
        } else if (st == ST_KEPT) {
            atomicOr(&m_kept[ty], 1ull << tx);
        }
    }
    __syncthreads();
    const int n = s_n;
    if (n > 0) {
        for (int it = 0; it < local_iters; ++it) {
            if (threadIdx.x == 0) s_changed = 0;
            __syncthreads();
            for (int li = threadIdx.x; li < n; li += 256) {
                const int ty = s_list[li] >> 6, tx = s_list[li] & 63;
                const unsigned long long mybit = 1ull << tx;
                if (!(m_und[ty] & mybit)) continue;
                const float sc = s_sc[ty * TW + tx];
                // Concurrent lanes flip bits while we look.  A lane that keeps q sets q's KEPT bit BEFORE clearing its
                // UNDECIDED bit, so reading UNDECIDED first and KEPT afterwards can never miss q in both.  Order:
                // (1) cheap filter on KEPT, (2) priority walk over UNDECIDED, (3) KEPT again (the authoritative read).
                const volatile unsigned long long* vk = m_kept;
                const volatile unsigned long long* vu = m_und;
                auto kept_in_window = [&] {
                    for (int dy = -R; dy <= R; ++dy)
                        if (vk[ty + dy] & (tab.win[dy < 0 ? -dy : dy] << (tx - R))) return true;
                    return false;
                };
                if (kept_in_window()) { atomicAnd(&m_und[ty], ~mybit); s_changed = 1; continue; }
                if (nms_tile_any_ahead(vu, s_sc, TW, ty, tx, sc, R, tab)) continue;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                if (kept_in_window()) { atomicAnd(&m_und[ty], ~mybit); s_changed = 1; continue; }
                atomicOr(&m_kept[ty], mybit);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                atomicAnd(&m_und[ty], ~mybit);
                s_changed = 1;
            }
            __syncthreads();
            if (!s_changed) break;
            __syncthreads();
        }
    }
    int left = 0;
    for (int o = threadIdx.x; o < NMS_TILE * NMS_TH; o += 256) {
        const int ty = R + o / NMS_TILE, tx = R + o % NMS_TILE;
        const int y = y0 + ty, x = x0 + tx;
        if (y < H && x < W) {
            const bool kept = (m_kept[ty] >> tx) & 1ull, und = (m_und[ty] >> tx) & 1ull;
            sb[(int64_t)y * W + x] = (uint8_t)(kept ? ST_KEPT : (und ? ST_UNDECIDED : ST_NONE));
            ob[(int64_t)y * W + x] = kept ? s_sc[ty * TW + tx] : 0.f;
            left |= und;
        }
    }
    left = __syncthreads_or(left);
    if (threadIdx.x == 0) {
        tile_active[tile_id] = left ? 1 : 0;
        if (left) atomicAdd(&counters[sweep], 1);
    }
}


// ---------------------------------------------------------------------------------------------
// Box NMS, round-3 form: exact, convergence guaranteed inside the last launch.
// Measured on a 480 x 640 heat map of this model (tools/nms_rounds.py): 31 k of 307 k pixels are candidates; the candidates that are
// maxima of their own overlap window (2.5 k) decide 22.5 k more in one step, and the remaining 6.4 k settle in three more keep rounds.
//   A  nms_localmax_kernel: one pass over the image in 32 x 64 tiles + halo — candidate mask, "kept in round 1" mask (a candidate with no
//      higher-priority candidate in its window; needs only the raw scores, so no tile ever waits for another) and the provisional output
//      (score where kept, 0 elsewhere).  Bit masks go to global memory as one uint32 per (row, 32 columns): a tile owns its words.
//   A2 nms_round_kernel: candidates that a round-1 keeper suppresses leave the undecided set.
//   B  nms_finish_kernel: ONE workgroup per image holds the image's two bit masks in LDS (480 x 640: 87 KB), lists what is left undecided
//      with its scores in LDS and runs the keep / suppress fixed point inside the workgroup until nothing is undecided — no other workgroup, no
//      host round trip, no sweep count.  Later keepers patch the output sparsely.
// Images whose masks do not fit LDS as one band (1024 x 1024: 3 bands, 2048 x 640: 4) are finished band by band, the finisher launch repeated.
// The sweep form above is left with images narrower than 32 columns, wider than 64 mask words or taller than 32 bands (nms_two_launch_applies;
// xp_box_nms_plan tells).
// ---------------------------------------------------------------------------------------------
#ifndef XP_NMS_DBG
#define XP_NMS_DBG 0   /* timing experiments only (wrong results), nms_localmax_kernel: 1 no candidate tests, 2 no out store, 4 no list building, 8 no loads, 16 no window walk */
#endif

// Wave compaction into an LDS list: the flagged lanes of a wave take consecutive slots from ONE atomicAdd of the ballot's popcount on the list's
// LDS counter (slot = base + flagged lanes below this one).  Returns the slot; it means something in flagged lanes only.
__device__ __forceinline__ int nms_wave_slot(bool flag, int* counter) {
    const unsigned long long sv = __ballot(flag);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (sv) {
        if (lane == 0) base = atomicAdd(counter, __popcll(sv));
        base = __shfl(base, 0, 64);
    }
    return base + __popcll(sv & ((1ull << lane) - 1ull));
}

template <int RT>
__global__ __launch_bounds__(256) void nms_localmax_kernel(const float* __restrict__ prob, float* __restrict__ out, unsigned* __restrict__ cand32,
                                                           unsigned* __restrict__ kept32, int H, int W, int wpr, NmsTable tab, float min_prob) {
    constexpr int RMAX = RT > 0 ? RT : NMS_MAXR;                     // compile-time reach: the tile image is sized for it (13.4 instead of 15.4 KB at reach 6: 7 instead of 4 workgroups per CU with the lists)
    constexpr int TWMAX = NMS_TILE + 2 * RMAX, THMAX = NMS_TH + 2 * RMAX;
    __shared__ float s_sc[TWMAX * THMAX];
    __shared__ unsigned long long m_cand[THMAX], m_kept[THMAX];
    __shared__ unsigned short s_list[NMS_TILE * NMS_TH], s_surv[NMS_TILE * NMS_TH];
    __shared__ int s_n, s_m;
    const int R = RT > 0 ? RT : tab.reach;          // RT > 0: compile-time reach (the window reads below unroll into straight-line code)
    const int TW = NMS_TILE + 2 * R, TH = NMS_TH + 2 * R;
    const int b = blockIdx.z;
    const int y0 = blockIdx.y * NMS_TH - R, x0 = blockIdx.x * NMS_TILE - R;
    const float* pb = prob + (int64_t)b * H * W;
    float* ob = out + (int64_t)b * H * W;
    for (int i = threadIdx.x; i < TH; i += 256) { m_cand[i] = 0ull; m_kept[i] = 0ull; }
    if (threadIdx.x == 0) { s_n = 0; s_m = 0; }
    __syncthreads();
    // tile + halo, a wave per tile row (lane = column, TW <= 62): the row's candidate mask is one ballot — no LDS atomics on the masks — and the
    // owned candidates of the row take their list slots from ONE atomicAdd per wave and row (nms_wave_slot).  Batches of 8 rows per
    // wave: the loads of a batch are issued before the first is used.
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int x = x0 + lane;
        const bool xin = lane < TW && x >= 0 && x < W;
        const unsigned long long own_cols = ((1ull << NMS_TILE) - 1ull) << R;
        for (int r0 = wave; r0 < TH; r0 += 4 * 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int ty = r0 + 4 * k, y = y0 + ty;
                v[k] = (ty < TH && xin && y >= 0 && y < H && !((XP_NMS_DBG & 8) && ty > 2)) ? pb[(int64_t)y * W + x] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int ty = r0 + 4 * k;
                if (ty >= TH) continue;                              // wave-uniform
                if (lane < TW) s_sc[ty * TW + lane] = v[k];
                const unsigned long long m = __ballot(v[k] > min_prob);      // (elements outside the image were loaded as 0 <= min_prob)
                if (lane == 0) m_cand[ty] = m;
                const unsigned long long own = (ty >= R && ty < R + NMS_TH) ? (m & own_cols) : 0ull;
                if (own && !(XP_NMS_DBG & 4)) {
                    const bool mine = (own >> lane) & 1ull;
                    const int slot = nms_wave_slot(mine, &s_n);
                    if (mine) s_list[slot] = (unsigned short)(ty * 64 + lane);
                }
            }
        }
    }
    __syncthreads();
    const int n = (XP_NMS_DBG & 1) ? 0 : s_n;
    // Phase 1, every candidate: quick reject — the 8 immediate neighbours are inside every overlap window (non-candidates score <= min_prob < sc:
    // harmless); eight independent LDS reads settle ~8 of 9 candidates.  The survivors are COMPACTED into a second list (one LDS atomic per wave and
    // batch) before the window walk: walking inside this loop, nearly every wave had a surviving lane and ran the whole data-dependent walk with
    // one lane in nine active (16 walk batches per tile on the bench's dense maps; now 2).
    for (int l0 = 0; l0 < n; l0 += 256) {
        const int li = l0 + threadIdx.x;
        bool top = li < n;
        unsigned short item = 0;
        if (top) {
            item = s_list[li];
            if (R >= 1) {
                const int ty = item >> 6, tx = item & 63;
                const float sc = s_sc[ty * TW + tx];
                const float* c = s_sc + ty * TW + tx;
                const float n0 = c[-TW - 1], n1 = c[-TW], n2 = c[-TW + 1], n3 = c[-1], n4 = c[1], n5 = c[TW - 1], n6 = c[TW], n7 = c[TW + 1];
                // nms_ahead with the position known: n0 .. n3 come before this pixel in row-major order (a tie loses to them), n4 .. n7 after it
                top = !(n0 >= sc || n1 >= sc || n2 >= sc || n3 >= sc || n4 > sc || n5 > sc || n6 > sc || n7 > sc);
            }
        }
        const int slot = nms_wave_slot(top, &s_m);
        if (top) s_surv[slot] = item;
    }
    __syncthreads();
    const int m = (XP_NMS_DBG & 16) ? 0 : s_m;
    // Phases 2 and 3, survivors only: is any pixel of the overlap window AHEAD of this one (nms_ahead)?
    if constexpr (RT > 0) {
        // Compile-time reach: every position of the (2 RT + 1)^2 square is read as a plain score at an immediate offset — straight-line code, all LDS
        // reads independent and in flight together; whether a position belongs to the overlap window is a uniform bit that masks the comparison, and a
        // non-candidate can never be ahead (its score <= min_prob < sc).  Phase 2 looks at the 7 x 7 neighbourhood (minus the 3 x 3 already seen) and
        // compacts again; phase 3 reads the rest of the square for what is left (the true maxima and a few more: about one wave per tile).  The
        // bit walk (nms_tile_any_ahead, runtime reach) is a chain of ffs -> dependent LDS read -> compare -> branch, ~130 links for a true maximum, and
        // every wave holds one: 40 of the kernel's 65 us on the bench's dense maps.
        auto ahead_in = [&](int ty, int tx, float sc, auto rin_tag, auto rout_tag) {          // positions with RIN < max(|dy|, |dx|) <= ROUT
            constexpr int RIN = decltype(rin_tag)::value, ROUT = decltype(rout_tag)::value;
            const float* c = s_sc + ty * (NMS_TILE + 2 * RT) + tx;
            bool ahead = false;
#pragma unroll
            for (int dy = -ROUT; dy <= ROUT; ++dy) {
                const unsigned long long w = tab.win[dy < 0 ? -dy : dy] >> (RT - ROUT);
#pragma unroll
                for (int dx = -ROUT; dx <= ROUT; ++dx) {
                    if ((dy < 0 ? -dy : dy) <= RIN && (dx < 0 ? -dx : dx) <= RIN) continue;          // compile time
                    const float sq = c[dy * (NMS_TILE + 2 * RT) + dx];
                    const bool in = (w >> (dx + ROUT)) & 1ull;                                      // uniform
                    ahead |= in && ((dy < 0 || (dy == 0 && dx < 0)) ? sq >= sc : sq > sc);          // nms_ahead, its position test folded at compile time
                }
            }
            return ahead;
        };
        constexpr int R2 = RT < 3 ? RT : 3;
        if (threadIdx.x == 0) s_n = 0;                  // reused as the length of the second survivor list (s_list is free again)
        __syncthreads();
        for (int l0 = 0; l0 < m; l0 += 256) {
            const int li = l0 + threadIdx.x;
            bool top = li < m;
            unsigned short item = 0;
            if (top) {
                item = s_surv[li];
                const int ty = item >> 6, tx = item & 63;
                top = !ahead_in(ty, tx, s_sc[ty * TW + tx], std::integral_constant<int, 1>{}, std::integral_constant<int, R2>{});
            }
            const int slot = nms_wave_slot(top, &s_n);
            if (top) s_list[slot] = item;
        }
        __syncthreads();
        const int m2 = s_n;
        for (int li = threadIdx.x; li < m2; li += 256) {
            const int ty = s_list[li] >> 6, tx = s_list[li] & 63;
            if (!ahead_in(ty, tx, s_sc[ty * TW + tx], std::integral_constant<int, R2>{}, std::integral_constant<int, RT>{})) atomicOr(&m_kept[ty], 1ull << tx);
        }
    } else {
        // runtime reach: walk over the candidate bits of the overlap window, early exit
        for (int li = threadIdx.x; li < m; li += 256) {
            const int ty = s_surv[li] >> 6, tx = s_surv[li] & 63;
            if (!nms_tile_any_ahead(m_cand, s_sc, TW, ty, tx, s_sc[ty * TW + tx], R, tab)) atomicOr(&m_kept[ty], 1ull << tx);
        }
    }
    __syncthreads();
    for (int o = threadIdx.x; o < NMS_TILE * NMS_TH; o += 256) {      // NMS_TILE = 32: a wave instruction writes two full 128-byte row segments
        const int ty = R + o / NMS_TILE, tx = R + o % NMS_TILE;
        const int y = y0 + ty, x = x0 + tx;
        if (y < H && x < W && !((XP_NMS_DBG & 2) && o > 3)) ob[(int64_t)y * W + x] = ((m_kept[ty] >> tx) & 1ull) ? s_sc[ty * TW + tx] : 0.f;
    }
    for (int r = threadIdx.x; r < NMS_TH; r += 256) {
        const int y = y0 + R + r;
        if (y < H) {
            const int64_t wo = ((int64_t)b * H + y) * wpr + blockIdx.x;
            cand32[wo] = (unsigned)((m_cand[R + r] & ~m_kept[R + r]) >> R);     // the undecided set after round 1
            kept32[wo] = (unsigned)(m_kept[R + r] >> R);
        }
    }
}

// ---- pass A2, one suppression round over the whole batch (all CUs): every undecided candidate with a kept box in its window leaves the undecided
// set.  Bit-mask work only; a workgroup owns a band of NMS_S1_ROWS rows and keeps the band's rows + reach of both masks in LDS.
// Only suppression runs wide.  After the local-maximum pass no candidate can become a keeper yet (its higher-priority neighbours are still undecided
// until this very round suppresses them): 22.5 k of 28.9 k candidates of a 480 x 640 map leave here.  A wide KEEP round distributes candidates by
// mask word, which serialises dense blobs (32 undecided pixels in one word = 32 dependent chains in one lane): it measured 95 us for round 2 on the
// model's maps against 11 us for this kernel, and the finisher's compacted list balances them — so the keep rounds are the finisher's.
template <int RT>
__global__ __launch_bounds__(256) void nms_round_kernel(const unsigned* __restrict__ und_in, const unsigned* __restrict__ kept_in,
                                                        unsigned* __restrict__ und_out, unsigned* __restrict__ kept_out, int H, int wpr, NmsTable tab) {
    __shared__ unsigned s_k[(NMS_S1_ROWS + 2 * NMS_MAXR) * (2 + 64)];      // kept rows of the band + reach, padded (wpr <= 64: host)
    __shared__ unsigned s_u[(NMS_S1_ROWS + 2 * NMS_MAXR) * (2 + 64)];      // undecided rows
    const int R = RT > 0 ? RT : tab.reach;
    const int rw = wpr + 2, b = blockIdx.y, y0 = blockIdx.x * NMS_S1_ROWS;
    const int nrows = NMS_S1_ROWS + 2 * R;
    for (int i = threadIdx.x; i < nrows * rw; i += 256) {
        const int r = i / rw, wi = i - r * rw - 1, y = y0 - R + r;
        const bool in = y >= 0 && y < H && wi >= 0 && wi < wpr;
        s_k[i] = in ? kept_in[((int64_t)b * H + y) * wpr + wi] : 0u;
        s_u[i] = in ? und_in[((int64_t)b * H + y) * wpr + wi] : 0u;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NMS_S1_ROWS * wpr; i += 256) {
        const int r = i / wpr, wi = i - r * wpr, y = y0 + r;
        if (y >= H) continue;
        const int64_t wo = ((int64_t)b * H + y) * wpr + wi;
        unsigned stay = s_u[(r + R) * rw + wi + 1];
        for (unsigned u = stay; u; u &= u - 1) {
            const int bit = __ffs((int)u) - 1;
            if (nms_any_in_window<RT>(s_k, rw, r + R, wi * 32 + bit, R, tab)) stay &= ~(1u << bit);          // suppressed
        }
        und_out[wo] = stay;
        kept_out[wo] = s_k[(r + R) * rw + wi + 1];
    }
}

// ---- pass B: the finisher (plan and LDS layout: nms_finish_plan).  With more than one band a workgroup sees the rows of its neighbours (reach R above
// and below) as they were when the launch started and cannot decide a candidate that waits on one of them: such launches are repeated (ping-pong
// masks) until a launch leaves nothing undecided — rare chains across a band border.
template <int RT>
__global__ __launch_bounds__(NMS_FIN_THREADS) void nms_finish_kernel(const float* __restrict__ prob, float* __restrict__ out,
                                                                       const unsigned* __restrict__ und32, const unsigned* __restrict__ kept32,
                                                                       unsigned* __restrict__ und_out, unsigned* __restrict__ kept_out,
                                                                       int* __restrict__ glist, int H, int W, NmsTable tab, int* __restrict__ counters,
                                                                       int sweep, int* __restrict__ info) {
    extern __shared__ __align__(16) unsigned char fin_lds[];
    __shared__ int s_n;
    const int R = RT > 0 ? RT : tab.reach;
    constexpr int NW = RT > 0 ? 2 * RT + 1 : 2 * NMS_MAXR + 1;
    const NmsFinishPlan pl = nms_finish_plan(H, W, R, NMS_FIN_LDS);
    unsigned* mU = reinterpret_cast<unsigned*>(fin_lds);                          // undecided (bits cleared as decisions fall)
    unsigned* mK = reinterpret_cast<unsigned*>(fin_lds + pl.mask_bytes);          // kept
    if (sweep > 0 && counters[sweep - 1] == 0) return;                            // banded form: an earlier launch already left nothing undecided
    const int b = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    const float* pb = prob + (int64_t)b * H * W;
    float* ob = out + (int64_t)b * H * W;
    const int wpr = pl.wpr, rw = pl.rw;
    const int yb0 = band * pl.brows, yb1 = min(H, yb0 + pl.brows);                // owned rows; LDS row r <-> image row yb0 - R + r
    const int nwords = (yb1 - yb0) * wpr;
    const int64_t img_words = (int64_t)b * H * wpr;
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    auto stamp = [&](int slot) { if (tid == 0 && info && band == 0) info[8 * b + slot] = (int)(__builtin_amdgcn_s_memrealtime() - t_start); };     // 100 MHz ticks (diagnostics)
    for (int i = tid; i < pl.rows * rw; i += NMS_FIN_THREADS) { mU[i] = 0u; mK[i] = 0u; }
    if (tid == 0) s_n = 0;
    __syncthreads();
    // halo rows (reach R above and below the band, as the launch found them): read-only neighbours
    if (pl.bands > 1) {
        for (int i = tid; i < 2 * R * wpr; i += NMS_FIN_THREADS) {
            const int h = i / wpr, wi = i - h * wpr;
            const int r = h < R ? h : (pl.rows - 2 * R + h);                      // LDS rows 0..R-1 and rows-R..rows-1
            const int y = yb0 - R + r;
            if (y >= 0 && y < H && !(y >= yb0 && y < yb1)) {
                mU[r * rw + wi + 1] = und32[img_words + (int64_t)y * wpr + wi];
                mK[r * rw + wi + 1] = kept32[img_words + (int64_t)y * wpr + wi];
            }
        }
    }
    // masks in; undecided positions into the list (LDS when it fits, else the caller's workspace — same code through a flat pointer)
    int my_count = 0;
    for (int i = tid; i < nwords; i += NMS_FIN_THREADS) {
        const int yl = i / wpr, wi = i - yl * wpr;
        const unsigned u = und32[img_words + (int64_t)(yb0 + yl) * wpr + wi];
        mU[(yl + R) * rw + wi + 1] = u;
        mK[(yl + R) * rw + wi + 1] = kept32[img_words + (int64_t)(yb0 + yl) * wpr + wi];
        my_count += __popc(u);
    }
    int my_base = my_count ? atomicAdd(&s_n, my_count) : 0;
    __syncthreads();
    const int total = s_n;
    // (workspace: positions then scores, sized by the rows this band OWNS — with pl.brows a short last band's scores would run past the image's slice)
    const int cap = total <= pl.list_cap ? pl.list_cap : (yb1 - yb0) * W;
    int* list = total <= pl.list_cap ? reinterpret_cast<int*>(fin_lds + pl.list_off) : glist + ((int64_t)b * H + yb0) * W * 2;
    float* lscore = reinterpret_cast<float*>(list + cap);
    for (int i = tid; i < nwords; i += NMS_FIN_THREADS) {
        const int yl = i / wpr, wi = i - yl * wpr;
        unsigned u = mU[(yl + R) * rw + wi + 1];
        while (u) {
            const int bit = __ffs((int)u) - 1;
            u &= u - 1;
            lscore[my_base] = pb[(int64_t)(yb0 + yl) * W + wi * 32 + bit];
            list[my_base++] = (yl << 16) | (wi * 32 + bit);                     // band-local row
        }
    }
    __syncthreads();
    if (tid == 0 && info) { info[8 * b] = total; info[8 * b + 1] = total <= pl.list_cap ? 0 : 1; }
    stamp(3);
    // Fixed point, asynchronous inside the workgroup.  Races between lanes are harmless by ordering: a lane that keeps q sets q's KEPT bit BEFORE
    // clearing its UNDECIDED bit, and a reader looks at UNDECIDED first and at KEPT afterwards, so it can never miss q in both.
    // The whole image runs on ONE CU, so instructions — not latency — are the budget (16 waves share 4 SIMDs): after every round the list is
    // compacted to the still-undecided entries (a wave is then busy with 64 live candidates, not with one), and a candidate's work is a loop over
    // the few undecided neighbours it really has, not an unrolled worst case.
    volatile unsigned* vU = mU;
    __shared__ int s_cnt[NMS_FIN_THREADS / 64];
    int n_live = total;
    for (int round = 0; round < 1000000; ++round) {
        // entries [0, n_live) are live; this thread's slice is contiguous within the round: e = tid + k * 1024
        int nkeep = 0, progress = 0;
        int kpos[8]; float ksc[8];                                   // survivors of this thread (at most 8 per round: slices beyond that stay in place, see below)
        const bool small = n_live <= 8 * NMS_FIN_THREADS;
        for (int e = tid; e < n_live; e += NMS_FIN_THREADS) {
            const int pos = list[e];
            const float sc = lscore[e];
            const int y = pos >> 16, x = pos & 0xffff;
            const int wofs = (y + R) * rw + (x >> 5) + 1;
            const unsigned mybit = 1u << (x & 31);
            bool live = (vU[wofs] & mybit) != 0u;
            if (live && nms_any_in_window<RT>(mK, rw, y + R, x, R, tab)) { atomicAnd(&mU[wofs], ~mybit); live = false; progress = 1; }
            if (live) {
                // the walk over the undecided neighbours: window words from the padded mask, scores from the heat map
                bool blocked = false;
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    const int dy = k - (NW >> 1);
                    unsigned long long v = (RT > 0 || (dy >= -R && dy <= R)) ? (nms_window(mU + (y + R + dy) * rw, x, R) & tab.win[dy < 0 ? -dy : dy]) : 0ull;
                    if (dy == 0) v &= ~(1ull << R);
                    if (blocked) v = 0ull;
                    while (v) {
                        const int j = __ffsll((long long)v) - 1;
                        v &= v - 1;
                        const int xx = x - R + j;
                        const float sq = pb[(int64_t)(yb0 + y + dy) * W + xx];      // L2-resident heat map (1.2 MB per image)
                        if (nms_ahead(sq, sc, dy, xx, x)) { blocked = true; break; }
                    }
                }
                if (!blocked) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                    if (nms_any_in_window<RT>(mK, rw, y + R, x, R, tab)) { atomicAnd(&mU[wofs], ~mybit); }      // the authoritative read
                    else {
                        atomicOr(&mK[wofs], mybit);
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                        atomicAnd(&mU[wofs], ~mybit);
                        ob[(int64_t)(yb0 + y) * W + x] = sc;
                    }
                    live = false;
                    progress = 1;
                }
            }
            if (live && small) {
                // static register slots: select chain instead of a dynamically indexed array
#pragma unroll
                for (int q = 0; q < 8; ++q) if (q == nkeep) { kpos[q] = pos; ksc[q] = sc; }
                ++nkeep;
            } else if (live) {
                nkeep = 1;                                           // large lists are not compacted (they shrink below the limit within a round or two)
            }
        }
        // banded form: a round without any decision means the rest waits on a neighbouring band — leave it to the next launch.  (One band: the
        // undecided candidate of highest priority always decides, so every round makes progress.)
        const int any_progress = __syncthreads_or(progress);
        if (!small) {
            if (!__syncthreads_or(nkeep)) { n_live = 0; break; }
            if (!any_progress) break;
            continue;
        }
        // compaction: exclusive scan of the per-thread survivor counts (wave ballots + a scan of the 16 wave totals)
        const int lane = tid & 63, wave = tid >> 6;
        int incl = nkeep;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
        if (lane == 63) s_cnt[wave] = incl;
        __syncthreads();                                             // (also: every read of list / lscore of this round is done)
        int base = 0, tot = 0;
#pragma unroll
        for (int wv = 0; wv < NMS_FIN_THREADS / 64; ++wv) { const int c = s_cnt[wv]; if (wv < wave) base += c; tot += c; }
        base += incl - nkeep;
#pragma unroll
        for (int q = 0; q < 8; ++q) if (q < nkeep) { list[base + q] = kpos[q]; lscore[base + q] = ksc[q]; }
        __syncthreads();
        n_live = tot;
        if (tid == 0 && info && band == 0) info[8 * b + 2] = round + 1;
        if (n_live == 0 || !any_progress) break;
    }
    if (pl.bands > 1) {
        // the band's rows of the next masks; a band that leaves something undecided asks for another launch
        __syncthreads();
        int left = 0;
        for (int i = tid; i < nwords; i += NMS_FIN_THREADS) {
            const int yl = i / wpr, wi = i - yl * wpr;
            const unsigned u = mU[(yl + R) * rw + wi + 1];
            und_out[img_words + (int64_t)(yb0 + yl) * wpr + wi] = u;
            kept_out[img_words + (int64_t)(yb0 + yl) * wpr + wi] = mK[(yl + R) * rw + wi + 1];
            left |= (u != 0u);
        }
        if (__syncthreads_or(left) && tid == 0) atomicAdd(&counters[sweep], 1);
    } else if (tid < NMS_MAX_SWEEPS && b == 0) {
        counters[tid] = 0;                                           // xp_box_nms_check: one band always converges inside the launch
    }

    stamp(7);
}

// Counter housekeeping as kernels, not hipMemsetAsync / hipMemcpyAsync: replayed from several hipGraphs on several streams
// (PairPipeline.capture with overlap) the API memset / copy nodes left the counters holding stale bytes on ROCm 7.2, kernel
// nodes do not.
__global__ void nms_reset_counters_kernel(int* __restrict__ counters) { if (threadIdx.x < NMS_MAX_SWEEPS) counters[threadIdx.x] = 0; }
__global__ void nms_publish_counter_kernel(int* __restrict__ counters, int from) { if (threadIdx.x == 0) counters[NMS_MAX_SWEEPS - 1] = counters[from]; }

// keep_top_k: rank of every survivor among the survivors of its image under (score desc, index asc);
// survivors with rank >= k are zeroed (utils.py:179-186: first k of the score-sorted survivors).
// Two launches: every rank is computed before any score is zeroed.
__global__ __launch_bounds__(256) void topk_rank_kernel(const float* __restrict__ out, const int* __restrict__ kp,
                                                        const int* __restrict__ counts, int* __restrict__ rank_out, int cap, int W,
                                                        int64_t HW) {
    __shared__ float s_sc[256];
    __shared__ int s_ix[256];
    const int b = blockIdx.y;
    const int n = min(counts[b], cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float* ob = out + (int64_t)b * HW;
    const int* kb = kp + (int64_t)b * cap * 2;
    float sc = 0.f; int ix = 0;
    if (i < n) { ix = kb[2 * i] * W + kb[2 * i + 1]; sc = ob[ix]; }
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + threadIdx.x;
        if (j < n) { const int jx = kb[2 * j] * W + kb[2 * j + 1]; s_ix[threadIdx.x] = jx; s_sc[threadIdx.x] = ob[jx]; }
        __syncthreads();
        const int m = min(256, n - j0);
        if (i < n)
            for (int t = 0; t < m; ++t) rank += (s_sc[t] > sc || (s_sc[t] == sc && s_ix[t] < ix));
        __syncthreads();
    }
    if (i < n) rank_out[(int64_t)b * cap + i] = rank;
}

__global__ __launch_bounds__(256) void topk_zero_kernel(float* __restrict__ out, const int* __restrict__ kp, const int* __restrict__ counts,
                                                        const int* __restrict__ rank, int cap, int W, int64_t HW, int k) {
    const int b = blockIdx.y;
    const int n = min(counts[b], cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && rank[(int64_t)b * cap + i] >= k) {
        const int* kb = kp + (int64_t)b * cap * 2;
        out[(int64_t)b * HW + kb[2 * i] * W + kb[2 * i + 1]] = 0.f;
    }
}

// the two-launch form applies when an image's padded masks and a minimal (position, score) list fit one workgroup's LDS, the mask words fit the
// round kernel's rows (64 per row) and the state bytes, and positions fit 16 bits
bool nms_two_launch_applies(int H, int W, int R) {
    static const bool force_sweeps = getenv("XP_NMS_SWEEP") != nullptr && atoi(getenv("XP_NMS_SWEEP")) != 0;     // A/B: the round-1/2 sweep form
    if (force_sweeps || W < 32) return false;
    const NmsFinishPlan pl = nms_finish_plan(H, W, R, NMS_FIN_LDS);
    return pl.wpr <= 64 && H < 65536 && W < 65536 && pl.list_cap >= 2048 && pl.bands <= 32;
}

// Local maxima, one wide suppression round (ping-pong masks), then the per-image finisher for what is left, all at kernel instance RT.
// band_sweeps: launches of the finisher when an image is split into row bands (ignored for one band)
template <int RT>
int box_nms_two_launch_at(const float* prob, float* out, void* workspace, int batch, int H, int W, int cap, const NmsTable& tab, float min_prob,
                          int band_sweeps, hipStream_t s) {
    const NmsWsLayout w = nms_ws_layout(batch, H, W, cap);
    XpProfScope prof("box_nms", s, 0.0, 8.0 * (double)batch * H * W);   // 8*H*W bytes per image
    static XpPerDeviceOnce attr_once;
    if (attr_once.need())
        XP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(nms_finish_kernel<RT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NMS_FIN_LDS));
    const int wpr = xp_cdiv(W, 32);
    unsigned* masks = nms_ws_at<unsigned>(workspace, 0);
    unsigned* um[2] = {masks, masks + 2 * w.mask_words};
    unsigned* km[2] = {masks + w.mask_words, masks + 3 * w.mask_words};
    int* counters = nms_ws_at<int>(workspace, w.counters);
    hipLaunchKernelGGL(nms_localmax_kernel<RT>, dim3(wpr, xp_cdiv(H, NMS_TH), batch), dim3(256), 0, s, prob, out, um[0], km[0], H, W, wpr, tab, min_prob);
    hipLaunchKernelGGL(nms_round_kernel<RT>, dim3(xp_cdiv(H, NMS_S1_ROWS), batch), dim3(256), 0, s, um[0], km[0], um[1], km[1], H, wpr, tab);
    int cur = 1;
    const NmsFinishPlan pl = nms_finish_plan(H, W, tab.reach, NMS_FIN_LDS);
    const int launches = pl.bands > 1 ? (band_sweeps > 0 ? band_sweeps : 1) : 1;
    if (pl.bands > 1) hipLaunchKernelGGL(nms_reset_counters_kernel, dim3(1), dim3(64), 0, s, counters);
    for (int sw = 0; sw < launches; ++sw, cur ^= 1)
        hipLaunchKernelGGL(nms_finish_kernel<RT>, dim3(pl.bands, batch), dim3(NMS_FIN_THREADS), NMS_FIN_LDS, s, prob, out, um[cur], km[cur], um[cur ^ 1], km[cur ^ 1],
                           nms_ws_at<int>(workspace, w.overflow), H, W, tab, counters, sw, nms_ws_at<int>(workspace, w.info));
    if (pl.bands > 1 && launches != NMS_MAX_SWEEPS) hipLaunchKernelGGL(nms_publish_counter_kernel, dim3(1), dim3(64), 0, s, counters, launches - 1);
    XP_LAUNCH_CHECK();
    return XP_OK;
}
// The reach of the model's boxes (size 8, iou 0.1) has compile-time instances of the three templated kernels; every other reach runs instance 0.
int box_nms_two_launch(const float* prob, float* out, void* workspace, int batch, int H, int W, int cap, const NmsTable& tab, float min_prob,
                       int band_sweeps, hipStream_t s) {
    return tab.reach == 6 ? box_nms_two_launch_at<6>(prob, out, workspace, batch, H, W, cap, tab, min_prob, band_sweeps, s)
                          : box_nms_two_launch_at<0>(prob, out, workspace, batch, H, W, cap, tab, min_prob, band_sweeps, s);
}

// Enqueue `sweeps` sweep launches (each exits at once when the previous one left nothing undecided).
int box_nms_enqueue(const float* prob, float* out, void* workspace, int batch, int H, int W, const NmsTable& tab,
                    float min_prob, int sweeps, bool first_round, hipStream_t s) {
    const NmsWsHead w = nms_ws_head(batch, H, W);
    int* counters = nms_ws_at<int>(workspace, w.counters);
    XpProfScope prof("box_nms", s, 0.0, 8.0 * (double)batch * H * W);   // 8*H*W bytes per image
    hipLaunchKernelGGL(nms_reset_counters_kernel, dim3(1), dim3(64), 0, s, counters);
    dim3 grid(xp_cdiv(W, NMS_TILE), xp_cdiv(H, NMS_TH), batch);
    // Local fixed-point iterations per sweep.  Early sweeps are dominated by decisions that wait on a neighbouring tile, so
    // iterating long inside a tile is wasted there (measured: 8 iterations in sweep 0 cost 256 us, 2 cost 128 us, and the
    // number of sweeps to convergence is the same); late sweeps touch few tiles and finish them locally.
    // XP_NMS_SCHED="a,b,c,..." overrides (tuning); read once, by whichever thread comes first.
    static const std::array<int, NMS_MAX_SWEEPS> sched = [] {
        std::array<int, NMS_MAX_SWEEPS> t;
        for (int i = 0; i < NMS_MAX_SWEEPS; ++i) t[i] = i < 3 ? 2 : 8;
        if (const char* e = getenv("XP_NMS_SCHED")) {
            int i = 0, last = 8;
            for (const char* q = e; *q && i < NMS_MAX_SWEEPS;) { last = atoi(q); t[i++] = last; while (*q && *q != ',') ++q; if (*q == ',') ++q; }
            for (; i < NMS_MAX_SWEEPS; ++i) t[i] = last;
        }
        return t;
    }();
    for (int i = 0; i < sweeps; ++i)
        hipLaunchKernelGGL(nms_sweep_kernel, grid, dim3(256), 0, s, prob, nms_ws_at<uint8_t>(workspace, 0), out, nms_ws_at<uint8_t>(workspace, w.tile_active),
                           H, W, tab, min_prob, counters, i, (first_round && i == 0) ? 1 : 0, sched[i]);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

// one counter to the host; the stream is synchronised when this returns
int nms_read_counter(const void* workspace, const NmsWsHead& w, int slot, int* host, hipStream_t s) {
    XP_HIP(hipMemcpyAsync(host, nms_ws_at<int>(const_cast<void*>(workspace), w.counters) + slot, sizeof(int), hipMemcpyDeviceToHost, s));
    XP_HIP(hipStreamSynchronize(s));
    return XP_OK;
}

}  // namespace

extern "C" size_t xp_box_nms_workspace_bytes(int batch, int H, int W, int cap) { return nms_ws_layout(batch, H, W, cap).total; }

// Which form xp_box_nms takes for a shape and box, from the launcher's own functions (host only: no launch, no device).
// plan[0..4] = form (0 sweep, 1 two-launch), reach, bands, rows per band, list_cap (undecided candidates whose list fits LDS).
extern "C" int xp_box_nms_plan(int H, int W, float size, float iou, int* plan) {
    XP_CHECK_ARG(plan, "xp_box_nms_plan: null pointer");
    XP_CHECK_ARG(H > 0 && W > 0, "xp_box_nms_plan: bad shape");
    NmsTable tab;
    XP_CHECK_ARG(make_nms_table(size, iou, &tab), "xp_box_nms: size must be a positive multiple of 0.5 and <= %d (got %f)", NMS_MAXR + 1, size);
    const NmsFinishPlan pl = nms_finish_plan(H, W, tab.reach, NMS_FIN_LDS);
    plan[0] = nms_two_launch_applies(H, W, tab.reach) ? 1 : 0;
    plan[1] = tab.reach;
    plan[2] = pl.bands;
    plan[3] = pl.brows;
    plan[4] = pl.list_cap;
    return XP_OK;
}

extern "C" int xp_box_nms(const float* prob, float* out, void* workspace, size_t workspace_bytes, int batch, int H, int W,
                          float size, float min_prob, float iou, int keep_top_k, int cap, int max_sweeps_async,
                          int* converged_host, void* stream) {
    XP_CHECK_ARG(prob && out && workspace, "xp_box_nms: null pointer");
    XP_CHECK_ARG(batch > 0 && H > 0 && W > 0, "xp_box_nms: bad shape");
    const NmsWsLayout w = nms_ws_layout(batch, H, W, cap);
    XP_CHECK_ARG(workspace_bytes >= w.total, "xp_box_nms: workspace too small");
    NmsTable tab;
    XP_CHECK_ARG(make_nms_table(size, iou, &tab), "xp_box_nms: size must be a positive multiple of 0.5 and <= %d (got %f)", NMS_MAXR + 1, size);
    hipStream_t s = (hipStream_t)stream;
    XP_CHECK_ARG(max_sweeps_async <= NMS_MAX_SWEEPS, "xp_box_nms: at most %d async sweeps", NMS_MAX_SWEEPS);
    if (nms_two_launch_applies(H, W, tab.reach)) {
        // exact, no sweep count when the image is one band (see nms_localmax_kernel): the same in the stream-ordered and in the synchronous mode.
        // Images split into row bands repeat the finisher (launches past convergence exit at once): max_sweeps_async of them stream-ordered, or —
        // synchronous mode — as many as there are counter slots, checked here.
        XP_TRY(box_nms_two_launch(prob, out, workspace, batch, H, W, cap, tab, min_prob, max_sweeps_async > 0 ? max_sweeps_async : NMS_MAX_SWEEPS, s));
        if (max_sweeps_async <= 0) {
            int left = 0;
            XP_TRY(nms_read_counter(workspace, w, NMS_MAX_SWEEPS - 1, &left, s));
            if (left != 0) { xp_set_error("xp_box_nms: %d row bands still undecided after %d finisher launches", left, NMS_MAX_SWEEPS); return XP_ERR_STATE; }
            if (converged_host) *converged_host = 1;
        }
    } else if (max_sweeps_async > 0) {
        // fire-and-forget: the caller checks the last counter later (xp_box_nms_check)
        XP_TRY(box_nms_enqueue(prob, out, workspace, batch, H, W, tab, min_prob, max_sweeps_async, true, s));
        if (max_sweeps_async != NMS_MAX_SWEEPS)
            hipLaunchKernelGGL(nms_publish_counter_kernel, dim3(1), dim3(64), 0, s, nms_ws_at<int>(workspace, w.counters), max_sweeps_async - 1);
    } else {
        bool first = true;
        const int per_round = 4;
        for (int round = 0; round < 100000; ++round) {
            XP_TRY(box_nms_enqueue(prob, out, workspace, batch, H, W, tab, min_prob, per_round, first, s));
            first = false;
            int left = 0;
            XP_TRY(nms_read_counter(workspace, w, per_round - 1, &left, s));
            if (left == 0) break;
        }
        if (converged_host) *converged_host = 1;
    }
    if (keep_top_k > 0) {
        XP_CHECK_ARG(cap > 0, "xp_box_nms: keep_top_k needs cap > 0");
        int* kp = nms_ws_at<int>(workspace, w.kp);
        int* counts = nms_ws_at<int>(workspace, w.counts);
        int* rank = nms_ws_at<int>(workspace, w.rank);
        XP_TRY(xp_extract_keypoints(out, nullptr, 0.f, kp, counts, batch, H, W, cap, nms_ws_at<void>(workspace, w.kp_ws), xp_extract_keypoints_workspace_bytes(batch, H, W), stream));
        dim3 grid(xp_cdiv(cap, 256), batch);
        hipLaunchKernelGGL(topk_rank_kernel, grid, dim3(256), 0, s, out, kp, counts, rank, cap, W, (int64_t)H * W);
        hipLaunchKernelGGL(topk_zero_kernel, grid, dim3(256), 0, s, out, kp, counts, rank, cap, W, (int64_t)H * W, keep_top_k);
        XP_LAUNCH_CHECK();
    }
    return XP_OK;
}

// After the stream has been synchronised: did the async NMS converge?  (device->host copy of one int)
extern "C" int xp_box_nms_check(const void* workspace, int batch, int H, int W, int* undecided_tiles, void* stream) {
    XP_CHECK_ARG(workspace && undecided_tiles, "xp_box_nms_check: null pointer");
    return nms_read_counter(workspace, nms_ws_head(batch, H, W), NMS_MAX_SWEEPS - 1, undecided_tiles, (hipStream_t)stream);
}
