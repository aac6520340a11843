// Host side of the dense engines (gemm.hip, gemm_x3.hip, gemm_h2.hip, gemm_h2p.hip, gemm_f16.hip, gemm_ring.hip), written once: the argument checks and
// parameter fill of the entry points, the launch sequence, and the N-only tile ladder.  Everything an engine decides for itself — its M-dependent tile rule,
// its forcing knobs, its choice between kernels — stays in the engine's own file.  Host code only; nothing here has linkage of its own.
#pragma once
#include <string>

#include "gemm_epilogue.h"

// ---- tile ladder ---------------------------------------------------------------------------------------------------------------------------------------
// The branches every engine takes from N alone: 0 = 128 x 32, 1 = 128 x 64, 2 = 128 x 96 (N = 65..96, and N = 192: two full 96-wide tiles instead of
// 128 + 64), -1 = the engine's own M-dependent branch.
static inline int xp_tile_by_n(int N) { return N <= 32 ? 0 : N <= 64 ? 1 : (N <= 96 || (N % 96 == 0 && (N / 96) % 4 != 0)) ? 2 : -1; }

// ---- argument checks and parameter fill ----------------------------------------------------------------------------------------------------------------
// `who` is the entry point's name: the prefix of every message.  The order of the checks is part of the C ABI's behaviour (the first failing one reports).
static inline int xp_check_affine(const char* who, const float* scale, const float* shift) {
    XP_CHECK_ARG((scale == nullptr) == (shift == nullptr), "%s: scale and shift go together", who);
    return XP_OK;
}
static inline int xp_check_gemm_shape(const char* who, bool ptrs, int M, int N, int K) {
    XP_CHECK_ARG(ptrs, "%s: null pointer", who);
    XP_CHECK_ARG(M > 0 && N > 0 && K > 0, "%s: bad shape %d %d %d", who, M, N, K);
    return XP_OK;
}
static inline int xp_check_epilogue(const char* who, const float* scale, const float* shift, int act) {
    XP_TRY(xp_check_affine(who, scale, shift));
    XP_CHECK_ARG(act >= 0 && act <= 3, "%s: bad act %d", who, act);
    return XP_OK;
}
// 3 x 3 convolution over NHWC: the checks (channels in whole `ci_mult`-element loads) and the implicit GEMM's geometry, for GemmParams and gemm_f16's F16Params
template <class P>
int xp_conv3x3_geometry(const char* who, P& p, bool ptrs, int ci_mult, const float* scale, const float* shift, int batch, int Hi, int Wi, int Ci, int Co,
                        int stride, int reflect_pad, int act) {
    XP_CHECK_ARG(ptrs, "%s: null pointer", who);
    XP_CHECK_ARG(Ci % ci_mult == 0, "%s: Ci must be a multiple of %d (got %d)", who, ci_mult, Ci);
    XP_CHECK_ARG(stride == 1 || stride == 2, "%s: stride 1 or 2", who);
    XP_TRY(xp_check_affine(who, scale, shift));
    XP_CHECK_ARG(!reflect_pad || (Hi >= 2 && Wi >= 2), "%s: reflection pad needs H,W >= 2", who);
    p.Hi = Hi; p.Wi = Wi; p.Ci = Ci; p.stride = stride; p.reflect = reflect_pad;
    p.Ho = (Hi + 2 - 3) / stride + 1; p.Wo = (Wi + 2 - 3) / stride + 1;
    p.M = batch * p.Ho * p.Wo; p.N = Co; p.K = 9 * Ci; p.lda = 0; p.ldc = Co; p.ldres = 0; p.act = act;
    return XP_OK;
}
// The f32-container entry points (xp_gemm_nt, _x3, _h2 / xp_conv3x3_nhwc, _x3, _h2): checks, then a GemmParams with everything but the engine's own
// fields (wscale, r16) filled in.  Wt is the f32 matrix or the engine's weight planes.
static inline int xp_gemm_nt_params(const char* who, GemmParams& p, const float* A, const void* Wt, float* C, const float* bias, const float* scale,
                                    const float* shift, const float* res, int M, int N, int K, int lda, int ldc, int ldres, int act) {
    XP_TRY(xp_check_gemm_shape(who, A && Wt && C, M, N, K));
    XP_CHECK_ARG(K % 4 == 0 && lda % 4 == 0, "%s: K and lda must be multiples of 4 (got %d, %d)", who, K, lda);
    XP_TRY(xp_check_epilogue(who, scale, shift, act));
    p.A = A; p.Wt = (const float*)Wt; p.C = C; p.bias = bias; p.scale = scale; p.shift = shift; p.res = res;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldc = ldc; p.ldres = ldres; p.act = act; p.mode = 0;
    return XP_OK;
}
static inline int xp_conv3x3_params(const char* who, GemmParams& p, const float* x, const void* Wt, float* y, const float* bias, const float* scale,
                                    const float* shift, int batch, int Hi, int Wi, int Ci, int Co, int stride, int reflect_pad, int act) {
    XP_TRY(xp_conv3x3_geometry(who, p, x && Wt && y, 4, scale, shift, batch, Hi, Wi, Ci, Co, stride, reflect_pad, act));
    p.A = x; p.Wt = (const float*)Wt; p.C = y; p.bias = bias; p.scale = scale; p.shift = shift; p.res = nullptr; p.mode = 1;
    return XP_OK;
}

// ---- launch --------------------------------------------------------------------------------------------------------------------------------------------
// One tag per kernel instance (tile x mode), so the HIP-event averages line up with rocprofv3's per-kernel rows; XP_PROF_SHAPES adds the launch's shape.
// `gelu` is the f32-container engines' and the ring engine's act == 1.  gemm_f16 passes false: its per-shape tags never carried the suffix, and a tag is a
// name that recorded breakdowns are keyed by, so it is kept as it was rather than made uniform.
template <class Tile>
std::string xp_dense_tag(const std::string& prefix, const std::string& suffix, int M, int N, int K, bool gelu) {
    std::string tag = prefix + std::to_string(Tile::BM) + "x" + std::to_string(Tile::BN) + suffix;
    if (xp_prof_by_shape()) tag += "_M" + std::to_string(M) + "_N" + std::to_string(N) + "_K" + std::to_string(K) + (gelu ? "_gelu" : "");
    return tag;
}
// Algorithmic bytes of a launch (roofline numerator): the input (for a convolution the image, not its im2col), the weights (`w_factor` containers per
// element: 1.5 for the three bf16 planes) and the output, twice with a residual; `elem` bytes per container.
template <class P>
double xp_dense_bytes(const P& p, bool conv, double elem, double w_factor = 1.0) {
    const double in_elems = conv ? (double)p.M / (p.Ho * p.Wo) * p.Hi * p.Wi * p.Ci : (double)p.M * p.K;
    return elem * (in_elems + w_factor * (double)p.N * p.K + (double)p.M * p.N * (p.res ? 2 : 1));
}
template <auto K>
int xp_lds_opt_in(size_t bytes) {
    XP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return XP_OK;
}
// Opt in to Tile::kLdsBytes of dynamic LDS where that exceeds `opt_in_above` (once per device and kernel instance: the static lives in this template), open
// the profiling scope, launch K0 — or K1, the kernel's implicit-convolution instance, when `conv`.  An engine with one kernel passes it twice.  A failed
// opt-in is recorded and, unless `strict`, the launch goes ahead: it fails and the caller's XP_LAUNCH_CHECK returns the error.
template <auto K0, auto K1, class Tile, class P>
int xp_dense_launch(const P& p, hipStream_t s, bool conv, const std::string& tag, int K, double bytes, int threads, size_t opt_in_above, bool strict = false) {
    static XpPerDeviceOnce attr_once;
    if (Tile::kLdsBytes > opt_in_above && attr_once.need()) {
        int rc = xp_lds_opt_in<K0>(Tile::kLdsBytes);
        if (K1 != K0 && xp_lds_opt_in<K1>(Tile::kLdsBytes) != XP_OK) rc = XP_ERR_HIP;
        if (strict && rc != XP_OK) return rc;
    }
    const dim3 grid(xp_cdiv(p.N, Tile::BN) * xp_cdiv(p.M, Tile::BM));
    XpProfScope prof(tag.c_str(), s, 2.0 * p.M * p.N * K, bytes);
    if (conv) hipLaunchKernelGGL(K1, grid, dim3(threads), Tile::kLdsBytes, s, p);
    else hipLaunchKernelGGL(K0, grid, dim3(threads), Tile::kLdsBytes, s, p);
    return XP_OK;
}
