// What both forms of box NMS and their host side (box_nms.hip) agree on: the tile constants, the overlap table, the priority rule, the padded-mask
// window reads, the finisher's band plan and the workspace layout.
//
// Greedy NMS (sort by score desc, stable; a kept box suppresses every later box with IoU > thr) is sequential by definition.  Parallel formulation
// with the IDENTICAL result for the strict total order (score desc, row-major index asc): iterate to a fixed point
//     undecided p becomes SUPPRESSED if a KEPT box overlaps it,
//     undecided p becomes KEPT if every overlapping box of higher priority is SUPPRESSED
// (all boxes overlapping a kept box are suppressed: lower priority ones by it, higher priority ones by an earlier keep, otherwise it would not have
// been kept).  Boxes are size x size squares centred on integer pixels, so "overlap with IoU > thr" is a translation-invariant predicate of
// (|dy|, |dx|): the host evaluates it with torchvision's float32 arithmetic into a bit table.
// Only box_nms.hip includes this file, so everything is in that file's anonymous namespace: internal linkage, and NmsTable keeps the name under
// which the kernels' signatures appear in every recorded profile.
#pragma once
#include <math.h>

#include "xp_common.h"

// the two entry points of keypoints.hip that keep_top_k and the workspace layout need
extern "C" size_t xp_extract_keypoints_workspace_bytes(int batch, int H, int W);
extern "C" int xp_extract_keypoints(const float* prob, const uint8_t* mask, float thr, int* kp, int* counts, int batch,
                                    int H, int W, int cap, void* workspace, size_t workspace_bytes, void* stream);

namespace {

constexpr int NMS_TILE = 32;          // tile width: the row masks are 64-bit words, NMS_TILE + 2 * NMS_MAXR <= 64
#ifndef XP_NMS_TH
#define XP_NMS_TH 64   /* measured at 480 x 640, 16 images: 0.41 ms (32), 0.37-0.39 (64), 0.44 (128), 0.58 (192) — fewer tiles pay the fixed per-tile cost, taller ones serialise */
#endif
constexpr int NMS_TH = XP_NMS_TH;     // tile height (rows are not limited by the mask width)
constexpr int NMS_MAXR = 15;
constexpr int NMS_MAX_SWEEPS = 64;        // counters[] slots (one per sweep of a round)
constexpr int NMS_S1_ROWS = 32;           // rows per workgroup of the wide suppression round
constexpr int NMS_FIN_THREADS = 1024;
constexpr size_t NMS_FIN_LDS = 158 * 1024;

struct NmsTable { unsigned long long win[NMS_MAXR + 1]; int reach; };   // win[|dy|]: bit (reach + dx) set iff overlap

inline bool make_nms_table(float size, float iou, NmsTable* t) {
    // torchvision float32 arithmetic on boxes [c - size/2, c + size/2]
    if (!(size > 0.f) || size > (float)(NMS_MAXR + 1) || (2.f * size) != floorf(2.f * size)) return false;
    const float half = size * 0.5f;
    const float area = ((0.f + half) - (0.f - half)) * ((0.f + half) - (0.f - half));
    uint32_t ovl[NMS_MAXR + 1];
    int reach = 0;
    for (int dy = 0; dy <= NMS_MAXR; ++dy) {
        uint32_t bits = 0;
        for (int dx = 0; dx <= NMS_MAXR; ++dx) {
            const float ay1 = -half, ay2 = half, ax1 = -half, ax2 = half;
            const float by1 = (float)dy - half, by2 = (float)dy + half, bx1 = (float)dx - half, bx2 = (float)dx + half;
            float w = fminf(ay2, by2) - fmaxf(ay1, by1); if (w < 0.f) w = 0.f;
            float h = fminf(ax2, bx2) - fmaxf(ax1, bx1); if (h < 0.f) h = 0.f;
            const float inter = w * h;
            const float ovr = inter / (area + area - inter);
            if (ovr > iou) { bits |= (1u << dx); if (dy > reach) reach = dy; if (dx > reach) reach = dx; }
        }
        ovl[dy] = bits;
    }
    t->reach = reach;
    for (int dy = 0; dy <= NMS_MAXR; ++dy) {
        unsigned long long m = 0;
        for (int dx = -reach; dx <= reach; ++dx)
            if ((ovl[dy] >> (dx < 0 ? -dx : dx)) & 1u) m |= 1ull << (reach + dx);
        t->win[dy] = m;
    }
    return true;
}

// THE priority rule, the one statement of the order that defines the result: box q is AHEAD of box p when its score is higher, or equal and q comes
// earlier in row-major order.  q (score sq) sits dy rows below p (above: dy < 0) at column xq, p (score sc) at column xp.
// Three places restate it in a form of their own and point here: the two straight-line tests of nms_localmax_kernel, where "earlier" is known at
// compile time (>= for earlier positions, > for later ones), and topk_rank_kernel, which ranks survivors by the same order over flat indices.
__device__ __forceinline__ bool nms_ahead(float sq, float sc, int dy, int xq, int xp) {
    return sq > sc || (sq == sc && (dy < 0 || (dy == 0 && xq < xp)));
}

// The tile forms' priority walk: is any set bit of the row masks `m` (64-bit word per tile row, bit = tile column) inside the overlap window of tile
// pixel (ty, tx) AHEAD of it?  Scores from the tile image s_sc (TW floats per row); early exit.  Mask is `const unsigned long long*`, or its volatile
// form where other lanes clear bits while this one looks (nms_sweep_kernel).
template <typename Mask>
__device__ __forceinline__ bool nms_tile_any_ahead(Mask m, const float* s_sc, int TW, int ty, int tx, float sc, int R, const NmsTable& tab) {
    const int sh = tx - R;
    bool ahead = false;
    for (int dy = -R; dy <= R && !ahead; ++dy) {
        unsigned long long u = m[ty + dy] & (tab.win[dy < 0 ? -dy : dy] << sh);
        if (dy == 0) u &= ~(1ull << tx);
        while (u) {
            const int bx = __ffsll((long long)u) - 1;
            u &= u - 1;
            if (nms_ahead(s_sc[(ty + dy) * TW + bx], sc, dy, bx, tx)) { ahead = true; break; }
        }
    }
    return ahead;
}

// ---- padded bit masks: one uint32 per (row, 32 columns), one zero word on the left and on the right of every row
__device__ __forceinline__ unsigned long long nms_window(const unsigned* __restrict__ row, int x, int R) {
    // bits [x - R, x - R + 63] of a padded mask row: bit j <-> column x - R + j
    const int xp = x - R + 32;
    const int wi = xp >> 5, sh = xp & 31;
    return (((unsigned long long)row[wi + 1] << 32) | row[wi]) >> sh;
}
// "does any bit of the padded mask M (row r of the image at M + (r + pad_rows) * rw) fall into the window of (y, x)"; RT > 0: compile-time reach,
// the 2 RT + 1 row reads are unrolled and issued together (one LDS round trip instead of 2 RT + 1 dependent ones)
template <int RT>
__device__ __forceinline__ bool nms_any_in_window(const unsigned* __restrict__ M, int rw, int yrow, int x, int R, const NmsTable& tab) {
    constexpr int NW = RT > 0 ? 2 * RT + 1 : 2 * NMS_MAXR + 1;
    unsigned long long acc = 0ull;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int dy = k - (NW >> 1);
        if (RT > 0 || (dy >= -R && dy <= R)) acc |= nms_window(M + (yrow + dy) * rw, x, R) & tab.win[dy < 0 ? -dy : dy];
    }
    return acc != 0ull;
}

// ---- the finisher's plan.  LDS: two padded bit masks ((rows + 2R) rows of wpr + 2 words) and the list of undecided positions in what is left.
// An image is handled by `bands` workgroups of `brows` rows each (1 band = the whole image: the fixed point completes inside the launch).
struct NmsFinishPlan { int wpr, rows, rw, bands, brows; size_t mask_bytes, list_off; int list_cap; };
__host__ __device__ inline NmsFinishPlan nms_finish_plan(int H, int W, int R, size_t lds_budget) {
    NmsFinishPlan p;
    p.wpr = (W + 31) / 32; p.rw = p.wpr + 2;
    const size_t per_row = (size_t)p.rw * 4 * 2;                         // both masks
    const size_t want = lds_budget * 5 / 8;                               // keep 3/8 of the budget for the (position, score) list
    int bands = 1;                                                        // as few as the LDS allows (more per image was measured: no gain, profiles/r5_nms_bands.txt)
    while (bands < 64 && (size_t)((H + bands - 1) / bands + 2 * R) * per_row > want) ++bands;
    p.bands = bands; p.brows = (H + bands - 1) / bands;
    p.rows = p.brows + 2 * R;
    p.mask_bytes = (size_t)p.rows * p.rw * 4;
    p.list_off = (2 * p.mask_bytes + 15) / 16 * 16;
    p.list_cap = lds_budget > p.list_off ? (int)((lds_budget - p.list_off) / 8) : 0;        // (position, score) per undecided candidate
    return p;
}

// ---- workspace layout: byte offsets from the workspace base, computed here and nowhere else.
// The head does not depend on `cap`: a caller that has none (the sweep form, xp_box_nms_check) gets an NmsWsHead and cannot name the tail.
struct NmsWsHead {
    size_t mask_words;      // offset 0: state bytes (sweep form) or — two-launch form, in the same bytes — four bit-mask arrays of mask_words uint32:
                            // (undecided, kept) x ping-pong; 2 * H * ceil(W / 32) words per image <= H * W bytes for W >= 32
    size_t tile_active;     // one flag per 32 x NMS_TH tile (sweep form)
    size_t counters;        // NMS_MAX_SWEEPS ints
};
struct NmsWsLayout : NmsWsHead {
    size_t kp, counts, rank, kp_ws;     // keep_top_k: (y, x) list of cap survivors per image, their counts and ranks, xp_extract_keypoints' own workspace
    size_t overflow;                    // undecided-list overflow: (position, score) per pixel (used only when an image's list outgrows LDS)
    size_t info;                        // 8 ints per image + 64: the finisher's diagnostics (tools/nms_bench.py reads them from the end of the workspace)
    size_t total;
};
inline NmsWsHead nms_ws_head(int batch, int H, int W) {
    NmsWsHead w;
    w.mask_words = (size_t)batch * H * xp_cdiv(W, 32);
    w.tile_active = xp_up256((size_t)batch * H * W);
    w.counters = w.tile_active + xp_up256((size_t)batch * xp_cdiv(H, NMS_TH) * xp_cdiv(W, NMS_TILE));
    return w;
}
inline NmsWsLayout nms_ws_layout(int batch, int H, int W, int cap) {
    NmsWsLayout w;
    static_cast<NmsWsHead&>(w) = nms_ws_head(batch, H, W);
    w.kp = w.counters + sizeof(int) * NMS_MAX_SWEEPS;
    w.counts = w.kp + sizeof(int) * (size_t)batch * cap * 2;
    w.rank = w.counts + sizeof(int) * batch;
    w.kp_ws = w.rank + sizeof(int) * (size_t)batch * cap;
    w.overflow = xp_up256(w.kp_ws + sizeof(int) * 64 + xp_extract_keypoints_workspace_bytes(batch, H, W));
    w.info = w.overflow + 2 * sizeof(float) * (size_t)batch * H * W;
    w.total = w.info + sizeof(int) * (8 * (size_t)batch + 64);
    return w;
}
template <typename T>
inline T* nms_ws_at(void* workspace, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(workspace) + offset); }

}  // namespace
