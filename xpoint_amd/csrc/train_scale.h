// One power of two per gradient operand: the largest magnitude of the operand (partial maxima, order-free), {S, 1 / S} with max|x| S in
// [2^13, 2^14), and the operand multiplied by S in place or into a copy.  One host helper for every training entry point that gives a gradient its own
// scale; the four kernels behind it live in train_dense.hip.  Host declarations only: nothing here is part of the C ABI.
#pragma once
#include "xp_common.h"

constexpr int XP_AMAX_PARTS = 1024;                                      // partial maxima an operand's scale is taken from
constexpr size_t XP_SCALE_HEAD_BYTES = XP_AMAX_PARTS * 4 + 256;          // workspace head: the partial maxima, then the float2 {S, 1 / S}
static inline float2* xp_head_scale(void* head) { return (float2*)((char*)head + XP_AMAX_PARTS * 4); }

// blocks of an element-wise walk over (rows, C) (td_for_each, train_rows.h): four rows per block, at most one block per partial maximum
static inline int xp_elem_blocks(int64_t rows) { return (int)((rows + 3) / 4 < XP_AMAX_PARTS ? (rows + 3) / 4 : XP_AMAX_PARTS); }

// How the helper walks an operand: one or two (rows, C, ld) pieces, each with its own launch of every kernel.
struct XpScaleWalk {
    struct { int64_t off, rows; int C, ld, blocks; } piece[2];
    int npieces;
};
static inline XpScaleWalk xp_walk_rows(int64_t rows, int C, int ld) { return XpScaleWalk{{{0, rows, C, ld, xp_elem_blocks(rows)}, {}}, 1}; }
// a flat vector of n elements as n / 256 rows of 256 and one tail row; the rows leave one partial maximum to the tail
static inline XpScaleWalk xp_walk_flat(int64_t n) {
    const int64_t rows = n / 256;
    const int tail = (int)(n - rows * 256);
    XpScaleWalk w{};
    if (rows) w.piece[w.npieces++] = {0, rows, 256, 256, (int)((rows + 3) / 4 < XP_AMAX_PARTS - 1 ? (rows + 3) / 4 : XP_AMAX_PARTS - 1)};
    if (tail) w.piece[w.npieces++] = {rows * 256, 1, tail, tail, 1};
    return w;
}

enum XpScaleApply { XP_SCALE_ONLY, XP_SCALE_IN_PLACE, XP_SCALE_COPY };      // nothing; out *= S (out holds the operand); out = S x (x and out with ld == C)

// amax parts of x -> `parts` (XP_AMAX_PARTS floats), {S, 1 / S} -> `scale`, then `apply`.  Launch order: amax per piece, scale, multiply / copy per piece.
int xp_own_scale(const float* x, const XpScaleWalk& w, float* parts, float2* scale, XpScaleApply apply, float* out, hipStream_t s);
// the same from partial maxima that a kernel of the caller already wrote, one per block of the walk (BatchNorm backward)
int xp_scale_from_parts(const float* parts, const XpScaleWalk& w, float2* scale, XpScaleApply apply, const float* x, float* out, hipStream_t s);

// The shape limits the 3x3 convolution gradients share: rows indexed as int with room for the tile walk, Ci Co below 2^cico_bits
static inline bool xp_conv_grad_shape_ok(int batch, int H, int W, int Ci, int Co, int cico_bits) {
    return batch > 0 && H >= 1 && W >= 1 && Ci > 0 && Co > 0 && (int64_t)batch * H * W < ((int64_t)1 << 31) / 16 && (int64_t)Ci * Co < ((int64_t)1 << cico_bits);
}
