// Fused SS2D core in pixel (NHWC) layout — the MI355X-first form of reference
// VMamba.py:601-646 (forward_corev2: cross_scan -> x_proj/dt_proj -> selective_scan -> cross_merge ->
// out_norm) for d_state = 1.
//
// The four scan routes (csm_triton.py:22-53) are permutations of the same pixels and x_proj / dt_proj
// are pointwise in L, so nothing is materialised per route: `xdbl` (M, 4*(R+2)) is ONE GEMM in pixel
// layout, dt_proj + softplus + exp run inside the scan, and the four routes become four traversals
// (row-major fwd/bwd, column-major fwd/bwd) of the same NHWC buffers.  With lanes over channels every
// access is a contiguous C*4-byte segment in either traversal, so the column routes need no transpose.
//
// The recurrence is made parallel over L by chunks of T pixels:
//   pass 1  per (image, route pair, chunk, channel): a-product P and local end state S of both routes
//   pass 2  per (image, route, channel): sequential carry over chunks -> state entering each chunk
//   pass 3  per (image, route pair, chunk, channel): re-run with the true start state, forward route
//           into an LDS tile, backward route added to it; the column pair adds the row pair's result
//           in the reference's order (y0 + y2) + (y1 + y3) (csm_triton.py:60-62) and applies out_norm
//           (LayerNorm over C, VMamba.py:644) before the single store.
// Directions are stored in the order (0, 2, 1, 3) so that a pair's operands are adjacent.
//
// This file is the host side: the choice between the two forms, the chunk plan and the entry points.  The kernels and their launches are in
// ss2d_chunked.hip (the three passes above, stages 0-1) and ss2d_seq.hip (the sequential form of the deep stages); ss2d_core.h has what they share.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "ss2d_core.h"

// L bound of the sequential (one wave per route) form, per image: see ss2d_core_impl
#define XP_SS2D_SEQ_DEFAULT_MAXL 8192

// -1 (default): chosen per call shape; 0: chunked three-pass form; 1: sequential form.  XP_SS2D_SEQ=0/1 presets it.
static std::atomic<int> g_ss2d_mode{getenv("XP_SS2D_SEQ") ? atoi(getenv("XP_SS2D_SEQ")) : -1};
extern "C" int xp_ss2d_core_set_mode(int mode) {
    XP_CHECK_ARG(mode >= -1 && mode <= 1, "xp_ss2d_core_set_mode: mode must be -1 (auto), 0 (chunked) or 1 (sequential)");
    g_ss2d_mode.store(mode);
    return XP_OK;
}

// THE decision "does this per-image shape take the sequential (deep-stage) form" — the one copy of it: ss2d_core_impl, xp_ss2d_core_p32_supported and
// xp_ss2d_core_f16_wants_f32_copies all call it, so the predicates the host plans with can never disagree with what the launch does.
// Per-image quantities only (never the batch).  half_io: the fp16-storage class, which needs f32 copies of u / xdbl for this form (have_copies).
static bool ss2d_takes_seq(int H, int W, int C, int R, bool half_io, bool have_copies) {
    static const int max_l = getenv("XP_SS2D_SEQ_MAXL") ? atoi(getenv("XP_SS2D_SEQ_MAXL")) : -1;
    if (!(C <= 768 && C % 64 == 0)) return false;
    if (!SS2DRanks::has(R)) return false;
    if (!half_io && xp_amp_value()) return false;          // the f32-container mixed-precision class: chunked form only (its dt rounding lives in step_vals)
    const bool seq2 = ss2d_seq_scan2_applies(R, H, W, C);
    if (half_io && !(seq2 && have_copies)) return false;
    const int mode = g_ss2d_mode.load();
    return mode >= 0 ? mode != 0 : (seq2 && H * W <= (max_l >= 0 ? max_l : XP_SS2D_SEQ_DEFAULT_MAXL));
}

extern "C" size_t xp_ss2d_core_workspace_bytes(int batch, int H, int W, int C) {
    // P and S: (B, 2, nc, 2, C) each with the smallest chunk (T = 8) -> upper bound; + ya (B,H,W,C)
    const int64_t L = (int64_t)H * W;
    const int64_t nc = (L + 7) / 8;
    const int64_t chunked = 2 * (int64_t)batch * 2 * nc * 2 * C + (int64_t)batch * L * C;
    const int64_t sequential = 4 * (int64_t)batch * L * C;     // y of the four routes (deep stages, ss2d_seq_scan)
    return (size_t)(chunked > sequential ? chunked : sequential) * sizeof(float);
}

// The chunked form's plan for p.H x p.W x p.C: chunk slots per workgroup (p.cpb), chunk length (p.T) and chunks per image (p.nc).  Per LAYER: never the batch.
static int ss2d_chunk_plan(SS2DParams& p, const char* who) {
    const int C = p.C;
    // threads = cpb * C must be a multiple of 64 and <= 768
    int cpb = 1;
    static const int blk_threads = getenv("XP_SS2D_THREADS") ? atoi(getenv("XP_SS2D_THREADS")) : 192;      // experiments: threads per workgroup of the chunked passes
    if (C < blk_threads) { cpb = blk_threads / C; while ((cpb * C) % 64) ++cpb; }
    XP_CHECK_ARG((cpb * C) % 64 == 0 && cpb * C <= 768, "%s: unsupported C=%d", who, C);
    p.cpb = cpb;
    // chunk length per LAYER (C only, never the batch).  Round 4 re-measured it in the overlapped step instead of alone: 32 pixels at C <= 96, 16 at C = 192 / 384
    // (round 1-3: 16 / 16 / 8, chosen on the stand-alone core) — alone the core times are equal within 2 % at stages 0 - 1, but half as many chunks are half as
    // many workgroups, carry entries and aggregate stores, and with three encoders in flight that is what the step pays for: 1 674 - 1 677 -> 1 707 - 1 708
    // pairs/s on one box (64 / 32 / 16: 1 662; 64 / 64 / 32: 1 653).  XP_SS2D_TBUDGET / XP_SS2D_T ("96:16,384:8") override for A/B runs
    // within 8 / 16 / 32 (64, measured slower above, went when pass 3 began to hold a chunk's operands in registers).
    static const int t_budget = getenv("XP_SS2D_TBUDGET") ? atoi(getenv("XP_SS2D_TBUDGET")) : 6144;
    int T = t_budget / (cpb * C);
    T = T >= 32 ? 32 : (T >= 16 ? 16 : 8);              // the chunk lengths pass 3 is instantiated for (ss2d_chunked.hip: ChunkKernels)
    if (!getenv("XP_SS2D_TBUDGET") && cpb == 1 && T > 16) T = 16;          // C = 192: 16 (32 measured equal in the step, slower alone)
    if (const char* tl = getenv("XP_SS2D_T")) {          // experiments: "96:32,192:16,384:16" = chunk length per channel count
        for (const char* q = tl; q && *q;) {
            int cc = 0, tt = 0;
            if (sscanf(q, "%d:%d", &cc, &tt) == 2 && cc == C && (tt == 8 || tt == 16 || tt == 32)) T = tt;
            q = strchr(q, ',');
            if (q) ++q;
        }
    }
    XP_CHECK_ARG(T == 8 || T == 16 || T == 32, "%s: chunk length %d is not one pass 3 is instantiated for (8, 16, 32)", who, T);
    p.T = T;
    p.nc = xp_cdiv(p.H * p.W, T);
    return XP_OK;
}

static int ss2d_core_impl(const void* u, const void* xdbl, const float* u32, const float* xdbl32, const float* wdt, const float* dt_bias,
                          const float* A, const float* Ds, const float* ln_w, const float* ln_b, void* out,
                          float* workspace, size_t workspace_bytes, int batch, int H, int W, int C, int R,
                          int dstate, float eps, bool half_io, void* stream, int out_p32 = 0) {
    const char* who = half_io ? "xp_ss2d_core_fwd_f16" : "xp_ss2d_core_fwd";
    XP_CHECK_ARG(u && xdbl && wdt && dt_bias && A && Ds && ln_w && ln_b && out && workspace, "%s: null pointer", who);
    XP_CHECK_ARG(dstate == 1, "%s: only d_state == 1 (the XPoint config) is implemented in the fused core; "
                              "use xp_selective_scan_fwd for general d_state (got %d)", who, dstate);
    XP_CHECK_ARG(batch > 0 && H > 0 && W > 0, "%s: bad shape", who);
    XP_CHECK_ARG(C % 32 == 0 && C >= 32 && C <= 768, "%s: C must be a multiple of 32 in [32,768] (got %d)", who, C);
    XP_CHECK_ARG(workspace_bytes >= xp_ss2d_core_workspace_bytes(batch, H, W, C), "%s: workspace too small", who);
    XP_CHECK_ARG((int64_t)H * W * C < (1ll << 31), "%s: one image plane (H*W*C) must stay below 2^31 elements", who);
    SS2DParams p;
    p.u = (const float*)u; p.xdbl = (const float*)xdbl; p.wdt = wdt; p.dtb = dt_bias; p.A = A; p.Dp = Ds; p.ln_w = ln_w; p.ln_b = ln_b;
    p.out = (float*)out; p.out_p32 = out_p32; p.Bn = batch; p.H = H; p.W = W; p.C = C; p.eps = eps;
    if (const int rc = ss2d_chunk_plan(p, who)) return rc;
    const int64_t nps = (int64_t)batch * 2 * p.nc * 2 * C;
    p.wsP = workspace; p.wsS = workspace + nps; p.ya = workspace + 2 * nps;
    hipStream_t s = (hipStream_t)stream;
    // Deep stages -> the sequential form.  The choice uses per-image quantities only (dt_rank, L), never the batch: the two forms differ
    // by rounding (~1e-7), and a result that changed with the number of images sharing a call would make grouped / split / single-image
    // runs of the same image disagree.  tools/ss2d_bench.py: C = 768, L = 300: 44 / 46 / 56 / 103 us for 2 / 4 / 16 / 32 images against
    // 51 / 65 / 169 / 292 us chunked; C = 768, L = 1024, 8 images: 131 vs 248 us.  C = 384, L = 1200 (stage 2 of a 480 x 640 image): 148 vs 195 us alone at
    // 16 images but 117 vs 47 us at 2 — the sequential form's time is the route's length, whatever the batch.  Rounds 2-3 called it a draw in the step and kept
    // it chunked (bound 512); re-measured in round 4 in the three-stream step it is +1.6 % at 8 pairs per call (1 671-1 673 -> 1 698, three alternations), 0 at
    // 4, -0.9 % at 2 and -4.8 % at ONE pair per call (0.99 -> 1.03 ms per pair).  The bound is now 2 048 for every dt_rank >= 16 shape — the configurations
    // this path is measured on run >= 8 pairs per GPU; the wave-pipelined kernel (ss2d_seq_scan3) then removed the one-pair cost as well (965 -> 1 029 pairs/s,
    // above the chunked form's 1 022), and the bound went to 8 192: stage 2 of a 1024 x 1024 image (L = 4 096) through the pipelined kernel is +2.4 % on
    // config C4 at 4 pairs per call, +2 % at 2, +0.8 % at 1.  xp_ss2d_core_set_mode / XP_SS2D_SEQ force one form.
    // (the f32-container mixed-precision class always takes the chunked form; the fp16-storage class takes the sequential form when the caller supplied f32
    //  copies of u and xdbl — xp_ss2d_core_f16_wants_f32_copies says when it will)
    const bool seq = ss2d_takes_seq(H, W, C, R, half_io, u32 && xdbl32);
    XP_CHECK_ARG(!out_p32 || (seq && !half_io), "%s: a P32 output exists for the sequential form only (xp_ss2d_core_p32_supported)", who);
    if (!SS2DRanks::has(R)) { xp_set_error("%s: dt_rank %d not instantiated (2,4,6,8,12,16,24,48)", who, R); return XP_ERR_ARG; }
    if (!seq) return ss2d_launch_chunked(p, R, half_io, s);
    if (half_io) { p.u = u32; p.xdbl = xdbl32; }
    return ss2d_launch_seq(p, workspace, R, half_io, s);
}

extern "C" int xp_ss2d_core_fwd(const float* u, const float* xdbl, const float* wdt, const float* dt_bias,
                                const float* A, const float* Ds, const float* ln_w, const float* ln_b, float* out,
                                float* workspace, size_t workspace_bytes, int batch, int H, int W, int C, int R,
                                int dstate, float eps, void* stream) {
    return ss2d_core_impl(u, xdbl, nullptr, nullptr, wdt, dt_bias, A, Ds, ln_w, ln_b, out, workspace, workspace_bytes, batch, H, W, C, R, dstate, eps, false, stream);
}

// out_fmt 0: f32 rows (= xp_ss2d_core_fwd); 2: the P32 image of the result (the operand format of xp_gemm_nt_h2s: out_proj loads it by DMA) — only where the
// sequential form runs (xp_ss2d_core_p32_supported, a per-image predicate)
extern "C" int xp_ss2d_core_p32_supported(int H, int W, int C, int R) { return ss2d_takes_seq(H, W, C, R, false, false) ? 1 : 0; }
extern "C" int xp_ss2d_core_fwd_ex(const float* u, const float* xdbl, const float* wdt, const float* dt_bias,
                                   const float* A, const float* Ds, const float* ln_w, const float* ln_b, void* out, int out_fmt,
                                   float* workspace, size_t workspace_bytes, int batch, int H, int W, int C, int R,
                                   int dstate, float eps, void* stream) {
    XP_CHECK_ARG(out_fmt == 0 || out_fmt == 2, "xp_ss2d_core_fwd_ex: out_fmt must be 0 (f32 rows) or 2 (P32 image)");
    return ss2d_core_impl(u, xdbl, nullptr, nullptr, wdt, dt_bias, A, Ds, ln_w, ln_b, out, workspace, workspace_bytes, batch, H, W, C, R, dstate, eps, false, stream, out_fmt == 2);
}

// Would xp_ss2d_core_fwd_f16 take the sequential (deep-stage) form for this per-image shape if it is given f32 copies of u and xdbl?  (A per-image
// predicate like the f32 class's: never depends on the batch.)
extern "C" int xp_ss2d_core_f16_wants_f32_copies(int H, int W, int C, int R) { return ss2d_takes_seq(H, W, C, R, true, true) ? 1 : 0; }

// The fast mixed-precision class's core: u (batch,H,W,C) and xdbl (batch*H*W, 4*(R+2)) are fp16, out is fp16 (= out_norm's f32 result cast to half,
// VMamba.py:646); the scan state, softplus / exp and out_norm run in f32 (csms6s.py:47-67); the dt projection's output is rounded to fp16 before the f32
// bias (a half convolution under autocast).  u_f32 / xdbl_f32: optional f32 copies of the same tensors — when given and the shape is a deep-stage one
// (xp_ss2d_core_f16_wants_f32_copies) the one-wave-per-route sequential kernels run on them.
extern "C" int xp_ss2d_core_fwd_f16(const void* u, const void* xdbl, const float* u_f32, const float* xdbl_f32, const float* wdt, const float* dt_bias,
                                    const float* A, const float* Ds, const float* ln_w, const float* ln_b, void* out,
                                    float* workspace, size_t workspace_bytes, int batch, int H, int W, int C, int R,
                                    int dstate, float eps, void* stream) {
    return ss2d_core_impl(u, xdbl, u_f32, xdbl_f32, wdt, dt_bias, A, Ds, ln_w, ln_b, out, workspace, workspace_bytes, batch, H, W, C, R, dstate, eps, true, stream);
}
