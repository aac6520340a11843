/* xpoint_hip.h — C ABI of libxpoint_hip.so: the MI355X (gfx950) XPoint inference hot path.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types cross this boundary.
 *   - every function returns int: 0 = ok, <0 = error (text: xp_last_error(), thread-local),
 *     except the *_bytes / *_numel size queries (size_t) and xp_version / xp_last_error.
 *   - the CALLER owns every buffer; pointers are device pointers (hipMalloc'd or torch
 *     `tensor.data_ptr()`), contiguous float32 unless stated, 16-byte aligned.
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) and
 *     are stream-ordered; no function synchronises the device unless it says so.
 *   - the library never allocates device memory: weights and workspaces are caller buffers sized by
 *     the *_workspace_bytes queries.  A context (xp_ctx_create) is host-only metadata.
 *   - activations are NHWC (channels contiguous) inside the library.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * repo canyagmur/XPoint).
 */
#ifndef XPOINT_HIP_H
#define XPOINT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int xp_version(void);
const char* xp_last_error(void);
int xp_device_info(int device, int* cu_count, int* wave_size, char* arch, int arch_len);
/* The registry of the library's XP_* environment knobs (csrc/xp_knobs.h): tuning / A-B switches only, each read once per process; no knob changes a
 * precision class.  xp_knob_info returns static strings: the variable, the source that reads it, what it does. */
int xp_knob_count(void);
int xp_knob_info(int index, const char** name, const char** where, const char** what);

/* ---------------------------------------------------------------------------------------------
 * Selective-scan forward.  Replaces the pybind op `selective_scan_cuda_oflex.fwd(u, delta, A, B, C,
 * D, delta_bias, delta_softplus, nrows, out_float)` —
 * xpoint/models/vmamba_src/kernels/selective_scan/csrc/selective_scan/cusoflex/selective_scan_oflex.cpp:143-231,
 * kernel selective_scan_fwd_kernel_oflex.cuh:67-181; Python caller vmamba_src/csms6s.py:71-87,112-126.
 *   u (batch, dim, seqlen); delta (batch, delta_dim, seqlen), dim % delta_dim == 0;
 *   A (dim, dstate); B, C (batch, ngroups, dstate, seqlen), dim % ngroups == 0;
 *   D (dim) or NULL; delta_bias (delta_dim) or NULL; out (batch, dim, seqlen) float32 ("oflex");
 *   last_state (batch, dim, dstate) or NULL  (= the reference's x[:, :, -1, 1::2]).
 *   dstate <= 256 (reference MAX_DSTATE, selective_scan_oflex.cpp:11). */
int xp_selective_scan_fwd(const float* u, const float* delta, const float* A, const float* B, const float* C,
                          const float* D, const float* delta_bias, float* out, float* last_state,
                          int batch, int dim, int delta_dim, int seqlen, int dstate, int ngroups,
                          int delta_softplus, void* stream);

/* The same operator with the reference's other input_t instantiations (cusoflex/selective_scan_core_fwd.cu:6-10) and its
 * second output (selective_scan_oflex.cpp:206-208, kernel selective_scan_fwd_kernel_oflex.cuh:154-162):
 *   itype 0 / 1 / 2: u, delta, B, C are f32 / f16 / bf16 (A, D, delta_bias always f32; the state is always f32);
 *   out_float != 0: out is f32 (the "oflex" form the Python caller uses, csms6s.py:80), else out has the input type;
 *   x_chunks (batch, dim, ceil(seqlen / 2048), 2 * dstate) f32 or NULL: per 2048-element chunk and state n the running
 *   prefix of the scan, x[.., 2n] = prod exp(delta A_n) since the start of the row, x[.., 2n + 1] = h_n at the end of the
 *   chunk (last state = x[:, :, -1, 1::2]).  The 16-bit instantiations evaluate exp(delta A) as exp2 on the hardware unit like
 *   the reference's kernel (reference tolerances f16 rtol 3e-3 / atol 5e-3, bf16 3e-2 / 5e-2: test_selective_scan.py:401-403). */
int xp_selective_scan_fwd_typed(const void* u, const void* delta, const float* A, const void* B, const void* C, const float* D,
                                const float* delta_bias, void* out, float* x_chunks, int itype, int out_float, int batch, int dim,
                                int delta_dim, int seqlen, int dstate, int ngroups, int delta_softplus, void* stream);

/* xp_selective_scan_fwd with the per-chunk scan state of xp_selective_scan_fwd_typed as an extra output: x_chunks (batch, dim,
 * ceil(seqlen / 2048), 2 * dstate) f32, non-NULL.  out and last_state are bit-identical to xp_selective_scan_fwd's (the same kernels; the
 * chunk states are bookkeeping next to the scan).  The forward of the differentiable float32 selective_scan_fn. */
int xp_selective_scan_fwd_x(const float* u, const float* delta, const float* A, const float* B, const float* C, const float* D,
                            const float* delta_bias, float* out, float* last_state, float* x_chunks, int batch, int dim, int delta_dim,
                            int seqlen, int dstate, int ngroups, int delta_softplus, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Selective-scan backward.  Replaces the pybind op `selective_scan_cuda_oflex.bwd(u, delta, A, B, C, D, delta_bias, dout, x,
 * delta_softplus, nrows)` (selective_scan_oflex.cpp:233-350).  Inputs as the forward (itype 0 / 1 / 2 = f32 / f16 / bf16 u, delta, B, C;
 * A, D, delta_bias f32); dout (batch, dim, seqlen) f32 if dout_float else the input type; x_chunks = the forward's chunk states
 * (xp_selective_scan_fwd_typed / xp_selective_scan_fwd_x), required when seqlen > 2048 (NULL allowed otherwise: the row starts from 0).
 * Outputs: du (batch, dim, seqlen) and ddelta (batch, delta_dim, seqlen) in the input type (ddelta summed over the delta repeat);
 * dA (dim, dstate), dD (dim) or NULL, ddelta_bias (delta_dim) or NULL in f32; dB, dC (batch, ngroups, dstate, seqlen) accumulated in f32 and
 * stored in the input type.  Every sum runs in a fixed order (per-workgroup partials in the workspace and a reduce pass, no atomics):
 * two calls are bit-identical and the per-sample gradients du / ddelta / dB / dC do not depend on the other samples.
 * workspace: xp_selective_scan_bwd_workspace_bytes(...) bytes, 256-byte aligned.  dstate 1 runs a specialised kernel. */
size_t xp_selective_scan_bwd_workspace_bytes(int batch, int dim, int delta_dim, int seqlen, int dstate, int ngroups);
int xp_selective_scan_bwd_typed(const void* u, const void* delta, const float* A, const void* B, const void* C, const float* D,
                                const float* delta_bias, const void* dout, const float* x_chunks, void* du, void* ddelta, float* dA,
                                void* dB, void* dC, float* dD, float* ddelta_bias, void* workspace, size_t workspace_bytes, int itype,
                                int dout_float, int batch, int dim, int delta_dim, int seqlen, int dstate, int ngroups,
                                int delta_softplus, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stand-alone four-route cross scan / cross merge.  Replace `cross_scan_fn` / `cross_merge_fn`
 * (xpoint/models/vmamba_src/csm_triton.py:501-517; torch forms cross_scan_fwd :22-53, cross_merge_fwd :56-85, one_by_one forms :88-180;
 * Triton kernel triton_cross_scan_flex :278-400) for the operator-level drop-in; the fused encoder never materialises the routes
 * (xp_ss2d_core_fwd below).  dtype 0 / 1 / 2 = float32 / float16 / bfloat16 elements.
 *   scans 0: routes row-major, column-major and their reverses; 1: four copies of the row-major route; 2: row-major twice, reversed twice.
 *   xp_cross_scan:  x (B,C,H,W) if in_channel_first else (B,H,W,C)  [one_by_one: (B,4,C,H,W) / (B,H,W,4,C), route k reads its own slice]
 *                   -> y (B,4,C,H*W) if out_channel_first else (B,H*W,4,C).
 *   xp_cross_merge: ys in the scan's OUT layout ((B,4,C,H*W) if out_channel_first else (B,H*W,4,C)) -> out in the scan's IN layout
 *                   ((B,C,H*W) if in_channel_first else (B,H*W,C)): (ys0 + ys2) + (ys1 + ys3) at every pixel, each add rounded to the dtype
 *                   (scans 1: ((ys0 + ys1) + ys2) + ys3 in a float32 accumulator, one rounding — torch's `sum(1)`);
 *                   one_by_one: the inverse permutation per route -> (B,4,C,H*W) / (B,H*W,4,C), no adds.
 * Bit-exact against the reference functions on random data (tests/golden/g22_cross_scan_ops.npz), incl. its own check shape (27,253,57,58). */
int xp_cross_scan(const void* x, void* y, int dtype, int B, int C, int H, int W, int in_channel_first, int out_channel_first,
                  int one_by_one, int scans, void* stream);
int xp_cross_merge(const void* ys, void* out, int dtype, int B, int C, int H, int W, int in_channel_first, int out_channel_first,
                   int one_by_one, int scans, void* stream);

/* Fused SS2D core in pixel layout = cross_scan + dt_proj + selective_scan + cross_merge + out_norm of
 * xpoint/models/vmamba_src/VMamba.py:601-646 (forward_corev2) with csm_triton.py:22-85 (cross scan/merge).
 *   u (batch, H, W, C) = SiLU(dwconv(in_proj(x)));  xdbl (batch*H*W, 4*(R+2)) = u @ x_proj^T with the four
 *   directions stored in the order (0, 2, 1, 3), each [dt_rank values, B, C];  wdt (4, R, C) (= dt_projs_weight transposed: channel-contiguous), dt_bias (4, C),
 *   A (4, C) = -exp(A_logs), Ds (4, C) in the same direction order;  ln_w/ln_b = out_norm;  out (batch, H, W, C).
 *   d_state must be 1 (the XPoint config; general d_state: xp_selective_scan_fwd).
 *   Two internal forms with the same results to f32 rounding: chunked three-pass (long sequences) and sequential per
 *   (image, route, 64 channels) wave (short sequences with many channels: the deep encoder stages); chosen per call
 *   shape, or forced with xp_ss2d_core_set_mode(0 chunked / 1 sequential / -1 automatic) for tests and A/B timing. */
size_t xp_ss2d_core_workspace_bytes(int batch, int H, int W, int C);
int xp_ss2d_core_set_mode(int mode);
int xp_ss2d_core_fwd(const float* u, const float* xdbl, const float* wdt, const float* dt_bias, const float* A,
                     const float* Ds, const float* ln_w, const float* ln_b, float* out, float* workspace,
                     size_t workspace_bytes, int batch, int H, int W, int C, int R, int dstate, float eps,
                     void* stream);
/* The same core with a selectable output format: out_fmt 0 = f32 rows (identical to xp_ss2d_core_fwd), 2 = the P32 image of the (B H W, C) result
 * (see xp_gemm_nt_h2s: the SS2D out_proj then loads it by DMA).  The P32 form exists where the sequential deep-stage form runs:
 * xp_ss2d_core_p32_supported(H, W, C, R) != 0 (per-image quantities only); elsewhere out_fmt = 2 is an argument error. */
int xp_ss2d_core_p32_supported(int H, int W, int C, int R);
int xp_ss2d_core_fwd_ex(const float* u, const float* xdbl, const float* wdt, const float* dt_bias, const float* A,
                        const float* Ds, const float* ln_w, const float* ln_b, void* out, int out_fmt, float* workspace,
                        size_t workspace_bytes, int batch, int H, int W, int C, int R, int dstate, float eps,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense layers (nn.Linear / nn.Conv2d of VMamba.py:110-128,649,663,1405-1440 and XPoint.py:112-138).
 *   C[m,n] = (act(sum_k A[m,k] Wt[n,k] + bias[n]) * scale[n] + shift[n]) + res[m,n]
 *   act: 0 none, 1 GELU(erf), 2 ReLU, 3 = ReLU applied after scale/shift (conv -> BN -> ReLU);
 *   bias/scale/shift/res may be NULL (scale and shift together);
 *   K and lda multiples of 4.  xp_conv3x3_nhwc: NHWC input, weight (Co, 3, 3, Ci), pad 1 (zero or
 *   reflection), stride 1 or 2, output NHWC (batch, Ho, Wo, Co). */
int xp_gemm_nt(const float* A, const float* Wt, float* C, const float* bias, const float* scale, const float* shift,
               const float* res, int M, int N, int K, int lda, int ldc, int ldres, int act, void* stream);
int xp_conv3x3_nhwc(const float* x, const float* Wt, float* y, const float* bias, const float* scale,
                    const float* shift, int batch, int Hi, int Wi, int Ci, int Co, int stride, int reflect_pad,
                    int act, void* stream);

/* fp32-accurate variants on the bf16 matrix pipe ("x3": every f32 operand is the exact sum of three bf16
 * values; six bf16 MFMA partial products per multiply, f32 accumulate; error below an f32 FMA chain —
 * DESIGN.md §4).  Same semantics, epilogue and reference call sites as the two entry points above, but
 * the weight matrix is passed pre-split: xp_split_weights_x3 converts a row-major (N, K) f32 matrix
 * (for the conv: (Co, 3, 3, Ci) flattened, K = 9 Ci) into xp_split_weights_x3_bytes(N, K) bytes of
 * slab-major bf16 planes, once per weight upload.  K, lda (resp. Ci) multiples of 4, as above. */
size_t xp_split_weights_x3_bytes(int N, int K);
int xp_split_weights_x3(const float* W, void* out, int N, int K, void* stream);
int xp_gemm_nt_x3(const float* A, const void* Wx3, float* C, const float* bias, const float* scale,
                  const float* shift, const float* res, int M, int N, int K, int lda, int ldc, int ldres, int act,
                  void* stream);
int xp_conv3x3_nhwc_x3(const float* x, const void* Wx3, float* y, const float* bias, const float* scale,
                       const float* shift, int batch, int Hi, int Wi, int Ci, int Co, int stride, int reflect_pad,
                       int act, void* stream);
/* fp32-grade variants on the f16 matrix pipe ("h2": every f32 operand is written as the sum of two fp16 values h0 + h1, which
 * reproduces it to 2^-23 relative in the worst case (fp16 has an 11-bit significand: |x - h0| <= 2^-11 |x|, and the 12-bit remainder
 * loses at most one bit in h1), 2^-25.5 on average; three fp16 MFMA partial products per multiply (a0 b0 + a0 b1 + a1 b0; the dropped
 * a1 b1 <= 2^-22 |ab|), f32 accumulate: per product <= 2^-21 |ab| worst case, ~2^-25 typical — the error class of the f32 FMA chain the
 * reference computes (csrc/gemm_h2_core.h) at half the matrix work of the "x3" kernels, which are exact to 2^-24 per operand).
 * Same semantics, epilogue and reference call sites as
 * xp_gemm_nt / xp_conv3x3_nhwc (VMamba.py:649,663 in/out_proj; :110-128 Mlp; :605 x_proj; :1405-1440 convs;
 * XPoint.py:112-138 head convs).  The weight matrix is passed pre-split: xp_split_weights_h2 converts a row-major (N, K) f32
 * matrix into xp_split_weights_h2_bytes(N, K) bytes — slab-major fp16 planes of the rows scaled by a power of two each
 * (largest element in [2^13, 2^14): keeps the low plane out of fp16's subnormal range) followed by the N inverse scales,
 * which the epilogue applies exactly.  Activations are split unscaled: |A| must stay below 65504 (fp16 range; see
 * xp_xpoint_forward_ex for the guard); elements below 2^-3 carry an absolute error <= 2^-25. */
size_t xp_split_weights_h2_bytes(int N, int K);
int xp_split_weights_h2(const float* W, void* out, int N, int K, void* stream);
int xp_gemm_nt_h2(const float* A, const void* Wh2, float* C, const float* bias, const float* scale, const float* shift,
                  const float* res, int M, int N, int K, int lda, int ldc, int ldres, int act, void* stream);
int xp_conv3x3_nhwc_h2(const float* x, const void* Wh2, float* y, const float* bias, const float* scale, const float* shift,
                       int batch, int Hi, int Wi, int Ci, int Co, int stride, int reflect_pad, int act, void* stream);
/* The same GEMM on PRE-SPLIT activations (round 5; csrc/gemm_ring.hip, csrc/ring_core.h — the "ring" engine; same reference call sites as xp_gemm_nt_h2:
 * VMamba.py:649,663 in/out_proj, :110-128 Mlp).  A is the "P32" image of an (M, K) f32 matrix: [m][k / 32][plane 0..1][32] fp16 with
 * A[m][k] = plane0 + plane1 (the two-way split of csrc/gemm_h2_core.h) — 4 bytes per element, K % 32 == 0, xp_p32_bytes(M, K) bytes.  It is written
 * by the PRODUCER of the tensor: xp_split_activations_h2 (from f32 rows), xp_layernorm_p32, xp_ss2d_core_fwd_ex(out_fmt = 2), or this GEMM itself
 * (out_fmt = 2: C is the P32 image of the (M, N) result, N % 32 == 0, ldc == N).  out_fmt 0: C f32 rows (ldc).  Wh2: xp_split_weights_h2's buffer.
 * Both operands reach the LDS by LDS-DMA and the K loop holds matrix instructions only; same partial products, same summation order and therefore the
 * same bits as xp_gemm_nt_h2's tile kernel on A = plane0 + plane1.  N % 8 == 0; bias / scale / shift / res (f32, ldres) / act as xp_gemm_nt.
 * xp_gemm_nt_h2s_applies(N, K): does xp_xpoint_forward route a layer of this shape here (a per-layer predicate: the producers of its input must know). */
size_t xp_p32_bytes(int64_t M, int K);
int xp_split_activations_h2(const float* x, void* out_p32, int64_t M, int K, int ldx, void* stream);
int xp_gemm_nt_h2s_applies(int N, int K);
int xp_gemm_nt_h2s(const void* A_p32, const void* Wh2, void* C, int out_fmt, const float* bias, const float* scale, const float* shift,
                   const float* res, int M, int N, int K, int ldc, int ldres, int act, void* stream);
/* LayerNorm (as xp_layernorm, gelu = 0) writing the P32 image of its (rows, C) result; C % 32 == 0. */
int xp_layernorm_p32(const float* x, void* y_p32, const float* w, const float* b, int64_t rows, int C, float eps, void* stream);
/* ---------------------------------------------------------------------------------------------
 * fp16-STORAGE dense kernels of the fast mixed-precision class (csrc/gemm_f16.hip): the reference's `mixed_precision: true` deployment
 * (xpoint/models/XPoint.py:182 autocast) with half tensors in HBM.  A (M, lda) and W (N, K) are fp16, K-contiguous; one exact fp16 product per multiply on
 * v_mfma_f32_32x32x16_f16, f32 accumulate;  C = r16( r16( act( r16(acc + bias) ) * scale + shift ) + res )  with r16 = round to nearest fp16 at every
 * point where autocast ends in a half tensor (absent terms drop out with their rounding); res (M, ldres) fp16; C fp16, or f32 holding the fp16-exact values
 * when c_f32 != 0 (the heads' `.to(torch.float)`, XPoint.py:349,363).  act as xp_gemm_nt.  K, lda multiples of 8; buffers 16-byte aligned. */
int xp_f32_to_f16(const float* x, void* y, int64_t n, void* stream);
int xp_gemm_nt_f16(const void* A, const void* W, void* C, int c_f32, const float* bias, const float* scale, const float* shift, const void* res,
                   int M, int N, int K, int lda, int ldc, int ldres, int act, void* stream);
/* 3x3 convolution (stride 1 | 2, zero or reflection pad 1) over NHWC halves as an implicit GEMM of the same kernel; W (Co, 3, 3, Ci) fp16; Ci % 8 == 0. */
int xp_conv3x3_nhwc_f16(const void* x, const void* W, void* y, int y_f32, const float* bias, const float* scale, const float* shift,
                        int batch, int Hi, int Wi, int Ci, int Co, int stride, int reflect_pad, int act, void* stream);

/* Fused MLP of a VSS block in that class (csrc/mlp_f16.hip; VMamba.py:110-128, :1230-1234):  x += fc2(GELU(fc1(a)))  with a = LayerNorm(x) (M, C) fp16 given,
 * x (M, C) fp16 updated in place, W1 (4C, C), W2 (C, 4C) fp16, biases f32; the hidden activation stays on chip; roundings as the two xp_gemm_nt_f16 calls it
 * replaces.  C in {32, 64, 96, 192} (xp_mlp_fused_f16_supported). */
int xp_mlp_fused_f16_supported(int C, int H4);
int xp_mlp_fused_f16(const void* a, void* x, const void* W1, const float* b1, const void* W2, const float* b2, int M, int C, int H4, void* stream);
/* ... with norm2 folded in (a = LayerNorm(x) computed in the kernel's prologue, rounded to fp16 like xp_layernorm_f16's output). */
int xp_ln_mlp_fused_f16(void* x, const float* ln_w, const float* ln_b, float eps, const void* W1, const float* b1, const void* W2, const float* b2,
                        int M, int C, int H4, void* stream);
/* norm + in_proj of a VSS block in one launch (VMamba.py:1225, :649):  y = LayerNorm(x) W^T,  x, y (M, C) fp16, W (C, C) fp16; C in {32, 64, 96, 192}. */
int xp_ln_proj_f16(const void* x, const float* ln_w, const float* ln_b, float eps, const void* W, void* y, int M, int C, void* stream);
/* Glue kernels of the same class (csrc/elementwise_f16.hip): half tensors in HBM, f32 arithmetic, one rounding per autocast boundary (= the store). */
int xp_stem_conv_ln_gelu_f16(const float* img, const float* w9co, const float* bias, const float* ln_w, const float* ln_b, void* y,
                             int batch, int H, int W, int CO, float eps, void* stream);
int xp_layernorm_f16(const void* x, void* y, const float* w, const float* b, int64_t rows, int C, float eps, void* stream);
int xp_dwconv3x3_silu_f16(const void* x, const float* w9c, void* y, float* y_f32_copy, int batch, int H, int W, int C, void* stream);
int xp_depth_to_space_nhwc_f16(const void* x, float* y_f32, void* y_f16, int batch, int H, int W, int C, int bs, int* status, void* stream);
/* Fused SS2D core on half tensors (see xp_ss2d_core_fwd): u, xdbl, out are fp16; scan state / softplus / exp / out_norm in f32 (csms6s.py:47-67,
 * VMamba.py:644-646); dt projection rounded to fp16 before the f32 bias.  u_f32 / xdbl_f32: optional f32 copies enabling the sequential deep-stage form
 * (xp_ss2d_core_f16_wants_f32_copies tells, from per-image quantities only, whether it would be taken). */
int xp_ss2d_core_f16_wants_f32_copies(int H, int W, int C, int R);
int xp_ss2d_core_fwd_f16(const void* u, const void* xdbl, const float* u_f32, const float* xdbl_f32, const float* wdt, const float* dt_bias,
                         const float* A, const float* Ds, const float* ln_w, const float* ln_b, void* out, float* workspace, size_t workspace_bytes,
                         int batch, int H, int W, int C, int R, int dstate, float eps, void* stream);
/* The whole forward in that class (csrc/model.cpp): `weights` = the blob whose autocast-cast tensors were rounded to fp16 (host), w16 = their fp16 copies
 * (xp_f16_weights_bytes / xp_prepare_f16_weights); workspace as xp_forward_workspace_bytes; outputs as xp_xpoint_forward_ex (f32, holding fp16-exact
 * encoder values; prob / desc computed in f32 from the half head outputs, XPoint.py:349,363). */
size_t xp_f16_weights_bytes(void* ctx);
int xp_prepare_f16_weights(void* ctx, const float* weights, void* w16, size_t w16_bytes, void* stream);
int xp_xpoint_forward_f16(void* ctx, const float* weights, const void* w16, const float* images, int batch, int H, int W, void* workspace,
                          size_t workspace_bytes, float* prob, float* desc_nhwc, float* enc_nhwc, float* logits_nhwc, int* status, void* stream);

/* Precision class of the "x3" kernels (xp_gemm_nt_x3, xp_conv3x3_nhwc_x3, xp_mlp_fused_x3 and every dense layer of
 * xp_xpoint_forward with wsplit != NULL), process-wide, read at launch time:
 *   6 (default)  all six partial products of weight >= 2^-16: f32-grade (the class pinned against the reference, 1e-4 bar)
 *   3            a0 b0 + a0 b1 + a1 b0: operands carried to 16 bits, error <= 3 * 2^-16 * sum|a||b| per dot product, half the matrix work
 *   1            a0 b0: bf16 operands, f32 accumulate — the arithmetic class of the reference's `mixed_precision` autocast
 *                (XPoint.py:182); activations, LayerNorm, scan and post-processing stay f32.
 * The same weight buffers serve all three. */
int xp_set_dense_products(int n);
int xp_get_dense_products(void);
/* Engine of the dense layers of xp_xpoint_forward (wsplit != NULL), process-wide, read at launch time:
 *   1 (default)  "h2": xp_gemm_nt_h2 / xp_conv3x3_nhwc_h2 — operands as two fp16 planes, three partial products (f32-grade)
 *   0            "x3": xp_gemm_nt_x3 / xp_conv3x3_nhwc_x3 — three bf16 planes, xp_set_dense_products partial products
 * The fused block kernels (xp_mlp_fused_x3, xp_ln_proj_x3) use the x3 planes under both; the buffer prepared by
 * xp_prepare_split_weights holds both formats. */
int xp_set_dense_engine(int engine);
int xp_get_dense_engine(void);
/* Per-launch engine override inside xp_xpoint_forward(_ex) (round 6; removes the range guard's cliff): with the split-fp16 engine selected, bit i
 * of `mask` sends dense launch i of the forward to the split-bf16 planes (x3: no operand-range limit) while every other launch stays on split fp16.
 * The host finds the launches whose operands leave the fp16 range by bisection over this mask (models.XPoint.handle_status) instead of moving
 * the whole weight set to x3.  Launch numbering (XP_DENSE_LAUNCHES = 47): 0 = patch-embed conv 2; block (stage s, index j), base = 1 + 5 (2 s + j):
 * base + 0 in_proj (with its LayerNorm when fused), + 1 x_proj, + 2 out_proj, + 3 fc1, + 4 fc2 (a fused block tail = one launch: any of + 2 .. + 4
 * sends all three); 41 + s = downsample conv after stage s; 44 = head trunk conv, 45 = detector 1x1, 46 = descriptor 1x1.  Process-wide, like the
 * engine; 0 (default) = no override.  Ignored by the mixed-precision classes. */
#define XP_DENSE_LAUNCHES 47
int xp_set_dense_override(unsigned long long mask);
unsigned long long xp_get_dense_override(void);
/* Mixed-precision class "amp16" — the arithmetic of the reference's `mixed_precision: true` deployment (XPoint.py:182: torch.cuda.amp.autocast
 * around the forward; half is autocast's default dtype): process-wide, read at launch time.
 *   1  every operation that autocast ends in a half tensor rounds its output to fp16 (round to nearest even; the values stay in f32 containers):
 *      the bias add, GELU, eval-BatchNorm affine and residual add of xp_gemm_nt_h2 / xp_conv3x3_nhwc_h2, xp_layernorm, both stages of
 *      xp_dwconv3x3_silu, the three stages of xp_stem_conv_ln_gelu (which also takes the image as half), the dt projection inside
 *      xp_ss2d_core_fwd (rounded before its f32 bias is added, csms6s.py:47-50) and the SS2D output (VMamba.py:646 `y.to(x.dtype)`); the scan,
 *      out_norm, softmax and normalize stay f32, as the reference's do (csms6s.py:52, XPoint.py:349,363).  xp_xpoint_forward(_ex) then runs
 *      every block as separate launches on the split-fp16 engine; the caller passes weights whose convolution / linear tensors were rounded to
 *      fp16 (autocast casts them; models.XPoint does this for gemm_mode "amp16"), so every product is one exact fp16 x fp16 MFMA product.
 *   0  (default) off.
 * Pinned against the real reference run under fp16 CPU autocast (tests/golden/g20); never the headline class. */
int xp_set_amp_mode(int mode);
int xp_get_amp_mode(void);
/* y[i] = (float)(half)x[i] (round to nearest even), n floats, 16-byte aligned buffers; in place allowed.  The `.half()` of the class above. */
int xp_round_f16(const float* x, float* y, int64_t n, void* stream);

/* Fused VSS-block MLP branch, in place:  X <- X + fc2(GELU(fc1(LayerNorm(X)) + b1)) + b2   (reference
 * VMamba.py:1230-1234 VSSBlock.forward second residual, :110-128 Mlp; LayerNorm over C, biased variance, eps;
 * exact-erf GELU).  One launch replaces xp_layernorm + two xp_gemm_nt_x3 calls; the (M, hidden) activation is never
 * written to memory (it goes from the fc1 accumulators to the fc2 operand registers).  Same split-bf16 arithmetic
 * as xp_gemm_nt_x3.
 * Optionally the block's first residual is folded in as well: with T1 != NULL the kernel first does
 * X <- X + T1 W0^T  (VMamba.py:663 SS2D out_proj, bias-free, and :1229 x = x + op(norm(x))), T1 (M, C) not aliasing X.
 * The weight matrices are passed as ONE packed stream in the order the kernel consumes them: xp_mlp_fused_x3_pack
 * converts fc1.weight (hidden, C), fc2.weight (C, hidden) and, if W0x3 != NULL, W0 (C, C) — all already in
 * xp_split_weights_x3 layout — into xp_mlp_fused_x3_pack_bytes(C, hidden, W0x3 != NULL) bytes, once per weight upload.
 * A stream packed with W0 must be used with T1 != NULL and vice versa.
 * Supported shapes: xp_mlp_fused_x3_supported(C, hidden) != 0 (C in {32, 64, 96, 128, 192}, hidden % 32 == 0,
 * 64 <= hidden <= 4096); other shapes return an argument error — callers use the separate entry points. */
int xp_mlp_fused_x3_supported(int C, int hidden);
size_t xp_mlp_fused_x3_pack_bytes(int C, int hidden, int with_proj);
int xp_mlp_fused_x3_pack(const void* W1x3, const void* W2x3, const void* W0x3, void* out, int C, int hidden, void* stream);
int xp_mlp_fused_x3(float* X, const float* T1, const float* ln_w, const float* ln_b, const void* Wpack, const float* b1,
                    const float* b2, int M, int C, int hidden, float eps, void* stream);
/* The same fused kernels on the split-fp16 engine ("h2", csrc/gemm_h2_core.h: two fp16 planes, three products): weight
 * streams packed from xp_split_weights_h2 buffers (W1h2 (hidden, C), W2h2 (C, hidden), W0h2 (C, C) or NULL), whose power-of-two
 * row scales the kernel undoes exactly (fc1: before the GELU; fc2 and the projections: on the accumulators); the same buffers
 * are passed again at launch for those scales.  Shapes as xp_mlp_fused_x3_supported. */
size_t xp_mlp_fused_h2_pack_bytes(int C, int hidden, int with_proj);
int xp_mlp_fused_h2_pack(const void* W1h2, const void* W2h2, const void* W0h2, void* out, int C, int hidden, void* stream);
int xp_mlp_fused_h2(float* X, const float* T1, const float* ln_w, const float* ln_b, const void* Wpack, const void* W1h2, const void* W2h2,
                    const void* W0h2, const float* b1, const float* b2, int M, int C, int hidden, float eps, void* stream);
size_t xp_ln_proj_h2_pack_bytes(int C, int N);
int xp_ln_proj_h2_pack(const void* W0h2, void* out, int C, int N, void* stream);
int xp_ln_proj_h2(const float* X, const float* ln_w, const float* ln_b, const void* Wpack, const void* W0h2, float* Out, int M, int C, int N,
                  float eps, void* stream);
/* The head of the block in the same row-stationary form:  Out (M, N) = LayerNorm(X) W0^T   (VMamba.py:1229 norm + :649
 * in_proj, bias-free), one launch instead of xp_layernorm + xp_gemm_nt_x3, the normalised rows never written to memory.
 * W0 (N, C) is passed as the packed stream built by xp_ln_proj_x3_pack from its xp_split_weights_x3 form
 * (xp_ln_proj_x3_pack_bytes(C, N) bytes; 0 = unsupported: C in {32, 64, 96, 128, 192}, N % 32 == 0).  Out must not alias X. */
size_t xp_ln_proj_x3_pack_bytes(int C, int N);
int xp_ln_proj_x3_pack(const void* W0x3, void* out, int C, int N, void* stream);
int xp_ln_proj_x3(const float* X, const float* ln_w, const float* ln_b, const void* Wpack, float* Out, int M, int C, int N,
                  float eps, void* stream);

/* Glue kernels (HBM-bound). */
int xp_layernorm(const float* x, float* y, const float* w, const float* b, int64_t rows, int C, float eps, int gelu,
                 void* stream);
int xp_dwconv3x3_silu(const float* x, const float* w9c, float* y, int batch, int H, int W, int C, void* stream);
int xp_stem_conv_ln_gelu(const float* img, const float* w9co, const float* bias, const float* ln_w, const float* ln_b,
                         float* y, int batch, int H, int W, int Co, float eps, void* stream);
int xp_depth_to_space_nhwc(const float* x, float* y, int batch, int H, int W, int C, int bs, void* stream);
int xp_softmax_shuffle(const float* logits, float* prob, int batch, int Hc, int Wc, int r, int ld, int mode, void* stream);
int xp_l2norm_rows(const float* x, float* y, int64_t rows, int C, float eps, void* stream);
int xp_nhwc_to_nchw(const float* x, float* y, int batch, int HW, int C, void* stream);
int xp_mul_mask(const float* x, const uint8_t* mask, float* y, int64_t n, void* stream);
/* Batch staging of a step's inputs in ONE launch: images[0 .. n) = optical, images[n .. 2n) = thermal (f32, n = pairs*H*W elements)
   and, when the masks are given (all three or none), masks[0 .. n) = mask_optical, masks[n .. 2n) = mask_thermal (u8).  Replaces the four
   device-to-device copies of the reference's batch assembly (predict_align_image_pair.py:185-190 stacks the pair into one batch;
   ImagePairDataset collate): the runtime's blit kernel moves a 9.8 MB image block at ~130 GB/s (76 us), this kernel at HBM speed. */
int xp_stage_pair_batch(const float* optical, const float* thermal, float* images, const uint8_t* mask_optical,
                        const uint8_t* mask_thermal, uint8_t* masks, int64_t n, void* stream);
int xp_maxpool2_nhwc(const float* x, float* y, int batch, int H, int W, int C, void* stream);
/* RegNet's cost volume followed by its global average pool (reference xpoint/models/RegNet.py:44-52: bmm(x1^T, x2) -> view(N, hw, H', W') ->
   adaptive_avg_pool2d(., 1)), without materialising the (hw, hw) volume:  v[n][p] = a[n][p] . mean_q b[n][q];  a, b (batch, hw, C) row-major
   (channel-normalised feature rows of the two images), v (batch, hw). */
int xp_costvolume_mean(const float* a, const float* b, float* v, int batch, int hw, int C, void* stream);
/* Data ingest (reference datasets/ImagePairDataset.py:199-208 cv2.imread + COLOR_BGR2GRAY + / 255.0, :254-274 crop):
 * src = decoded 8-bit image on the device, (H0, W0, channels) interleaved with channels 1 (gray), 3 (R,G,B) or 4 (R,G,B,A);
 * dst (h, w) f32 = lut256[gray] of the crop at (top, left), gray = (B*1868 + G*9617 + R*4899 + 8192) >> 14 (OpenCV's 8-bit
 * fixed-point BGR2GRAY), lut256[k] = float32(k / 255.0) supplied by the host (double-precision division as numpy's). */
int xp_ingest_u8(const uint8_t* src, int H0, int W0, int channels, int top, int left, int h, int w,
                 const float* lut256, float* dst, void* stream);
/* dst[i] = (float)src[i] / 255 for a batch of 8-bit gray images already cropped (n elements): the device half of an 8-bit upload — the reference loader's
 * `astype(float32) / 255` (xpoint/datasets/ImagePairDataset.py:254-274), same IEEE division, same bits.  src 4-byte, dst 16-byte aligned. */
int xp_u8_to_unit_f32(const uint8_t* src, float* dst, int64_t n, void* stream);
/* Copy `bytes` from device memory to PINNED (device-mapped: hipHostMalloc / torch pin_memory) host memory with a kernel on `stream` instead of a copy
 * engine: small result lists of a streaming step, so that they never queue in front of the next step's image upload (predict.PairPipeline.download_async).
 * Valid on the host once an event recorded on `stream` after the call has completed.  16-byte aligned pointers. */
int xp_copy_to_mapped_host(const void* src_dev, void* dst_host, size_t bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Model forward.  Replaces xpoint.models.XPoint.forward_impl (xpoint/models/XPoint.py:283-323) with the
 * VMamba encoder (vmamba_src/VMamba.py:1507-1525) and the detector / descriptor heads (XPoint.py:348-371).
 * Device-format parameters live in ONE caller-owned float blob; xp_param_info enumerates
 * (name, offset, numel) so the host can fill it from a reference state_dict (xpoint_amd/models.py). */
typedef struct xp_model_cfg {
    int embed_dim;       /* MODEL.VSSM.EMBED_DIM (96) */
    int n_stages;        /* len(DEPTHS) */
    int depths[4];
    int d_state;         /* SSM_D_STATE (1) */
    int dt_rank;         /* 0 = "auto" = ceil(dim/16) */
    float mlp_ratio;     /* 4.0 */
    int head_channels;   /* 256 */
    int desc_size;       /* descriptor_size (256) */
    int det_channels;    /* 65 */
} xp_model_cfg;

int xp_ctx_create(const xp_model_cfg* cfg, void** ctx);
int xp_ctx_destroy(void* ctx);
int xp_param_count(void* ctx);
size_t xp_weights_numel(void* ctx);
int xp_param_info(void* ctx, int index, char* name, int name_len, size_t* offset, size_t* numel);
int xp_forward_shapes(void* ctx, int batch, int H, int W, int* Hc, int* Wc, int* enc_channels);
size_t xp_forward_workspace_bytes(void* ctx, int batch, int H, int W);
/* Split-bf16 copies of the GEMM / conv weights (xp_split_weights_x3 layout) for the fp32-accurate bf16-matrix-pipe
 * kernels: a second caller-owned device buffer of xp_split_weights_bytes(ctx) bytes, derived from the f32 blob by
 * xp_prepare_split_weights after every weight upload (the f32 blob stays the single source of truth, e.g. for the
 * RCCL broadcast). */
size_t xp_split_weights_bytes(void* ctx);
int xp_prepare_split_weights(void* ctx, const float* weights, void* wsplit, size_t wsplit_bytes, void* stream);
/* images (batch,1,H,W) in [0,1]; outputs: prob (batch,H,W) or NULL; desc_nhwc (batch,Hc,Wc,desc_size) or NULL;
 * enc_nhwc (batch,Hc,Wc,embed_dim/2) required; logits_nhwc (batch,Hc,Wc,65) or NULL.
 * wsplit: the buffer prepared by xp_prepare_split_weights -> dense layers run on xp_gemm_nt_x3 / xp_conv3x3_nhwc_x3;
 * NULL -> they run on the exact-f32 MFMA kernels (xp_gemm_nt / xp_conv3x3_nhwc).  Same results to f32 rounding.
 * With the split-fp16 engine selected (xp_set_dense_engine(1), the default of the Python host) every dense-layer INPUT must stay
 * below 65504 in magnitude; beyond it that layer's output rows turn into NaN, and because the heads apply ReLU (max(NaN, 0) = 0 on the
 * GPU) `prob` may then look finite.  xp_xpoint_forward_ex reports it: `status` (device int, caller-zeroed, may be NULL) receives, OR-ed in by
 * the kernels that write the outputs anyway (no extra pass, no host synchronisation):
 *   XP_STATUS_ENC  (1)  the encoder output (= the residual stream every dense layer of the encoder writes into, and the operand of the head
 *                       convolution) holds a non-finite element, or — split-fp16 engine only — one with |x| >= 65504
 *   XP_STATUS_PROB (2)  a heat-map cell had a non-finite logit        XP_STATUS_DESC (4)  a descriptor row had a non-finite element
 * A caller that reads a non-zero status re-runs the forward on engine 0 (split-bf16: no range limit) — the Python host does so
 * automatically and stays on that engine for the weight set (models.XPoint, PairPipeline.verify). */
int xp_xpoint_forward(void* ctx, const float* weights, const void* wsplit, const float* images, int batch, int H, int W,
                      void* workspace, size_t workspace_bytes, float* prob, float* desc_nhwc, float* enc_nhwc,
                      float* logits_nhwc, void* stream);
#define XP_STATUS_ENC 1
#define XP_STATUS_PROB 2
#define XP_STATUS_DESC 4
int xp_xpoint_forward_ex(void* ctx, const float* weights, const void* wsplit, const float* images, int batch, int H, int W,
                         void* workspace, size_t workspace_bytes, float* prob, float* desc_nhwc, float* enc_nhwc,
                         float* logits_nhwc, int* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Post-processing.
 * xp_box_nms replaces xpoint.utils.box_nms (xpoint/utils/utils.py:148-192; torchvision.ops.nms /
 * batched_nms): prob (batch,H,W) -> out (batch,H,W) with surviving scores, zeros elsewhere.
 *   size: box side (multiple of 0.5, <= 16); keep_top_k > 0 keeps the k best survivors per image (needs cap >=
 *   survivors).  Exact greedy NMS as a fixed point (round 3): a local-maximum pass, one suppression round and an in-launch finisher per
 *   image (three launches, NO sweep count) whenever an image fits the finisher's LDS as one band (480 x 640 and smaller); larger images
 *   (1024 x 1024) are finished band by band and the finisher launch is repeated — launches past convergence exit at once.
 *   max_sweeps_async == 0: synchronous like the reference (returns a finished tensor; banded images: XP_ERR_STATE if bands are still
 *   undecided after all counter slots); > 0: stream-ordered, at most that many finisher launches for banded images, no host
 *   synchronisation — verify later with xp_box_nms_check (0 undecided = exact result; one-band images always are).  Shapes the
 *   fixed-point form does not cover (fewer than 32 or more than 2048 columns, more than 32 bands) take tile sweeps with the same two
 *   modes; xp_box_nms_plan tells which form a shape takes. */
size_t xp_box_nms_workspace_bytes(int batch, int H, int W, int cap);
int xp_box_nms(const float* prob, float* out, void* workspace, size_t workspace_bytes, int batch, int H, int W,
               float size, float min_prob, float iou, int keep_top_k, int cap, int max_sweeps_async,
               int* converged_host, void* stream);
int xp_box_nms_check(const void* workspace, int batch, int H, int W, int* undecided_tiles, void* stream);
/* Which form xp_box_nms takes for (H, W, size, iou), computed by the launcher's own functions; host only, no launch, no device.
 * plan[0..4] = form (0 tile sweeps, 1 local maxima + finisher), reach (largest |dy|, |dx| at which two boxes overlap with IoU > iou),
 * bands per image, rows per band, undecided candidates per band whose list fits LDS (more go to the workspace). */
int xp_box_nms_plan(int H, int W, float size, float iou, int* plan);

/* torch.nonzero((prob > thr) [* mask]) per image (predict_align_image_pair.py:242-243, predict_keypoints.py:213-215):
 * kp (batch, cap, 2) int32 (y, x) in row-major order, counts (batch) int32 (may exceed cap: truncated list). */
size_t xp_extract_keypoints_workspace_bytes(int batch, int H, int W);
int xp_extract_keypoints(const float* prob, const uint8_t* mask, float thr, int* kp, int* counts, int batch, int H,
                         int W, int cap, void* workspace, size_t workspace_bytes, void* stream);

/* xpoint.utils.interpolate_descriptors (utils.py:229-238): bilinear grid_sample (align_corners=True) of the
 * NHWC descriptor volume (batch,Hc,Wc,D) at the keypoints + L2 normalisation -> out (batch, cap, D). */
int xp_sample_descriptors(const int* kp, const int* counts, const float* desc_nhwc, float* out, int batch, int cap,
                          int Hc, int Wc, int D, int H, int W, void* stream);

/* xpoint.utils.get_matches(d1, d2, 'bfmatcher', False, crossCheck=True) (xpoint/utils/matching.py:4-36; OpenCV
 * BFMatcher NORM_L2) for `pairs` independent pairs.  d1 (pairs,cap1,D), d2 (pairs,cap2,D); the number of valid
 * rows of pair i is counts[i*cnt_stride + which1] / [.. + which2] (counts NULL: all cap rows).
 * mode 0 = strict mutual nearest neighbour (primary), 1 = legacy cross-check.  Outputs: idx12/dist12 (pairs,cap1),
 * idx21/dist21 (pairs,cap2), matches (pairs,cap1) as (queryIdx, trainIdx, distance) ascending in queryIdx,
 * match_count (pairs).  Index results are those of exact arithmetic (first index wins exact ties): the fp16 matrix pass only nominates, the
 * nominated pairs are re-evaluated in f32 direct form and the survivors of that window in fp64 (csrc/match.hip). */
size_t xp_match_workspace_bytes(int pairs, int cap1, int cap2, int D);
int xp_match_mnn(const float* d1, const float* d2, const int* counts, int cnt_stride, int which1, int which2, int pairs,
                 int cap1, int cap2, int D, int mode, int* idx12, float* dist12, int* idx21, float* dist21,
                 int* match_q, int* match_t, float* match_d, int* match_count, void* workspace, size_t workspace_bytes,
                 void* stream);
/* `get_matches(..., knn_matches=True)` (matching.py:20-27): cv2.BFMatcher(NORM_L2).knnMatch(d1, d2, k = 2) — the two nearest targets of every query in
 * exact arithmetic (ties -> lower index); the caller applies Lowe's ratio test.  idx2 / dist2 (pairs, cap1, 2); a pair with fewer than two targets gets
 * -1 / +inf in the missing slots.  Same workspace as xp_match_mnn. */
int xp_match_knn2(const float* d1, const float* d2, const int* counts, int cnt_stride, int which1, int which2, int pairs, int cap1, int cap2,
                  int D, int* idx2, float* dist2, void* workspace, size_t workspace_bytes, void* stream);
/* `ThresholdMatcher.match` (matching.py:77-102): every (q, t) with sqrt(2 - 2 clip(<a_q, b_t>, -1, 1)) < threshold, decided in fp64 (the matrix pass only
 * nominates).  out_pairs (out_cap, 3) = (pair, query, target) in NO particular order (the reference lists them row-major: the host wrapper sorts),
 * out_dist (out_cap); out_count: EIGHT ints on the device, [0] = accepted pairs (> out_cap: list truncated), [1] = nominated pairs (> hit_cap: repeat with a
 * larger `hits` scratch of hit_cap x 2 ints — accepted pairs may be missing).  0 <= threshold <= 2. */
int xp_match_threshold(const float* d1, const float* d2, const int* counts, int cnt_stride, int which1, int which2, int pairs, int cap1, int cap2,
                       int D, double threshold, int* hits, int hit_cap, int* out_pairs, float* out_dist, int* out_count, int out_cap,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Candidate-list statistics of the latest xp_match_mnn call on `workspace` (same pairs / cap1 / cap2 / D / counts): out4 = 4 x uint64 on the device =
 * [sum of the nomination-list lengths over live rows and columns, the longest list, rows + columns whose list overflowed the inline capacity
 * (xp_match_cand_cap(); finished by the parallel overflow pass), live rows + columns].  bench.py reports them as match_candidates_per_row /
 * match_overflow_rows: the matcher's run time depends on them (clustered descriptors nominate more), its result never does. */
int xp_match_stats(void* workspace, const int* counts, int cnt_stride, int which1, int which2, int pairs, int cap1, int cap2, int D,
                   unsigned long long* out4, void* stream);
int xp_match_cand_cap(void);

/* ---------------------------------------------------------------------------------------------
 * Evaluation-harness helper: out[i] = min_j |a_i - b_j| (Euclidean, 2-D points (y, x)); +inf when
 * nb == 0.  a is f64 (warped keypoints), b f32 (pixel keypoints): the difference is formed in f64 and cast to f32, the
 * norm is taken in f32 — the arithmetic of benchmark_evaluation.py:441-450 (repeatability) and :652-659 (correct-match
 * matrix, reduced over one axis) without materialising the N x M matrix. */
int xp_points_min_dist(const double* a, int na, const float* b, int nb, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Detector evaluation against keypoint labels: the true / false positive assignment and the prediction-label distances of
 * xpoint/utils/evaluation.py:57-97 (compute_tp_fp_dist) for a batch of heat maps, without the (predictions x labels)
 * distance matrix and without a sequential walk over the predictions.  Four launches; the sort that ranks the candidates and the
 * scan of the pair counts between them are the caller's (xpoint_amd/evaluation.py uses torch on the device).  Every quantity is
 * per image: image b of a batch gets the bits it gets alone.
 *   prob (batch, H, W) f32, labels (batch, H, W) u8 (non-zero = label).  A candidate is a pixel with prob > zero_threshold
 *   (zero_threshold >= 0, so candidates are positive).  Rank order: descending prob, ties by ascending row-major pixel index
 *   (this project's rule; the reference leaves equal probabilities to torch.sort).  Rank key (u64, formed in registers): high word
 *   = ~(float bits of prob), low word = pixel index — a smaller key ranks first.  The same order over an image is a STABLE
 *   descending sort of cand_prob, which is how the caller obtains rank_pix.
 *   distance_thresh in [0, 8]; H * W must fit 32 bits; batch <= 65535.  A label is "within the radius" of a pixel when
 *   sqrtf(dy*dy + dx*dx) <= distance_thresh in f32 (torch.norm of the integer difference cast to float).
 *
 * xp_detector_eval_claim   per candidate: scans the (2 floor(distance_thresh) + 1)^2 window of the label map in row-major order;
 *                          first_label = pixel index of the first label within the radius (0xFFFFFFFF: none), n_within = their
 *                          number, and atomicMin(winner[first_label], key).  cand_prob = prob at a candidate, 0 elsewhere.
 *                          cand_prob / winner / first_label / n_within are (batch, H*W); winner is initialised here (all ones).
 *                          n_cand / n_gt (batch) int32: candidates and labels per image.
 * xp_detector_eval_resolve tp_pix (batch, H*W) u8 = the pixel is a candidate, has a first label and its key is that label's
 *                          winner — i.e. it is the best-ranked prediction claiming the label, which is what the reference's loop
 *                          computes (incl. "no label left": a label that is taken stays taken; zero labels: nothing matches).
 * xp_detector_eval_gather  rank_pix (batch, H*W) i64: the pixel index of every rank (ranks >= n_cand[b] are ignored).  Per rank:
 *                          tp_sorted = tp_pix of its pixel, cnt_sorted = n_within of its pixel; 0 past the candidates.
 * xp_detector_eval_fill_dist  dist[incl[b, i] - cnt_sorted[b, i] + k] = distance to the k-th (row-major) label within the radius
 *                          of rank i's pixel; incl = inclusive scan (i64) of cnt_sorted over the flattened (batch, H*W) array, so
 *                          dist (dist_len f32) is the reference's dist[matches] of image 0, then image 1, ...  Writes outside
 *                          [0, dist_len) are dropped. */
int xp_detector_eval_claim(const float* prob, const uint8_t* labels, int batch, int H, int W, float zero_threshold, float distance_thresh,
                           float* cand_prob, unsigned long long* winner, unsigned int* first_label, int* n_within,
                           int* n_cand, int* n_gt, void* stream);
int xp_detector_eval_resolve(const float* cand_prob, const unsigned long long* winner, const unsigned int* first_label, int batch,
                             int H, int W, uint8_t* tp_pix, void* stream);
int xp_detector_eval_gather(const long long* rank_pix, const uint8_t* tp_pix, const int* n_within, const int* n_cand, int batch, int H, int W,
                            uint8_t* tp_sorted, int* cnt_sorted, void* stream);
int xp_detector_eval_fill_dist(const long long* rank_pix, const uint8_t* labels, const long long* incl, const int* cnt_sorted,
                               int batch, int H, int W, float distance_thresh, float* dist, long long dist_len, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Robust homography from point correspondences, batched over pairs: the device-side stand-in
 * for cv2.findHomography(src, dst, cv2.USAC_MAGSAC, ransacReprojThreshold, confidence, maxIters) as called from
 * predict_align_image_pair.py:291-303 and benchmark_evaluation.py:796-812.  Same contract (H maps src -> dst, h33 = 1;
 * inlier mask at the reprojection threshold; no model below 4 correspondences -> n_inliers = 0, H = identity), a
 * different — deterministic — estimator (hash-seeded 4-point DLT hypotheses, MSAC score, least-squares refinement):
 * not bit-comparable with OpenCV.
 *   src, dst (pairs, cap, 2) f32 (x, y); counts (pairs) int32 or NULL; H (pairs, 9) f64; mask (pairs, cap) u8. */
/* Correspondences of the mutual matches for xp_find_homography (counts = match_count): kp (2*pairs, cap, 2) int32 (y, x),
 * optical images first; src / dst (pairs, cap, 2) f32 (x, y) — the optical_pts / thermal_pts lists of
 * predict_align_image_pair.py:283-284 built on the device. */
int xp_gather_match_points(const int* kp, const int* match_q, const int* match_t, const int* match_count, int pairs, int cap,
                           float* src, float* dst, void* stream);
size_t xp_find_homography_workspace_bytes(int pairs);
int xp_find_homography(const float* src, const float* dst, const int* counts, int pairs, int cap, float reproj_thr,
                       int max_iters, unsigned seed, double* H, uint8_t* mask, int* n_inliers, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Matching evaluation for a batch of pairs (csrc/pair_eval.hip; DESIGN.md "Matching evaluation"): the device work of
 * benchmark_evaluation.py's compute_repeatability_for_sample (:396-467), compute_descriptor_for_sample (:588-751) and the corner error
 * of compute_pts_dist_for_sample (:755-830) on ragged batches.  kp (2*pairs, cap, 2) int32 (y, x), optical images first; counts
 * (2*pairs) int32 (a count above cap means a truncated list: min(count, cap) rows are used); the match lists are xp_match_mnn's.
 * Image i < pairs is the optical image of pair i and image pairs + i its thermal image; "the other image" of i is (i + pairs) % (2 pairs).
 * Every quantity of pair p is what the pair gives alone; no float atomics; rows at or beyond a count are never read as data.
 *
 * xp_pair_eval_warp_near: every keypoint of image i through map1[i] and, when map2 != NULL, then map2[i] (both (2*pairs, 9) f64 row-major, acting
 *   on (x, y, 1)): hom = (x*h0 + y*h1) + h2 ..., divided by the third coordinate, in f64 without contraction (homographies.py:479-497).
 *   truncate != 0: each map is followed by numpy's astype(int) (toward zero; non-finite or beyond int64 gives INT64_MIN) — repeatability.
 *   warped (2*pairs, cap, 2) f64 (y, x); inframe (2*pairs, cap) u8 = filter_points (homographies.py:511-526) on an H x W frame;
 *   near (2*pairs, cap) f32 = min over the other image's keypoints of the norm (difference in f64, cast to f32, dx*dx + dy*dy and sqrt in f32;
 *   xp_points_min_dist's arithmetic), +inf when the other image has none.  Filler rows: warped 0, inframe 0, near +inf.
 * xp_pair_eval_match_dist: for match j of pair p (q = match_q, t = match_t): dist (2, pairs, cap) f32, [0] = |warped[p][q] - kp[pairs + p][t]|,
 *   [1] = |warped[pairs + p][t] - kp[p][q]| (f64 difference cast to f32, sqrt(dx*dx + dy*dy) in f32: the entries of the correct-match matrix the match loop reads, benchmark_evaluation.py:655-675).
 *   Filler (j >= match_count, or an index outside its list): +inf.
 * xp_pair_eval_count: thresholds (T <= 16) are HOST floats passed by value.  near_cnt (2, pairs, T) = rows of image (dir * pairs + p) with
 *   near <= th, over the rows below the count (near_inframe_only == 0) or those of them that are in frame (!= 0: repeatability counts the
 *   filtered points only); match_cnt (2, pairs, T) = matches with dist <= th (0 when dist == NULL); n_inframe (2, pairs).  Integer sums.
 * xp_pair_eval_corner_error: err (pairs) f64 = mean over the reference's point list [[0,0],[H,0],[0,W],[H,H]] (as (y, x), kept as it is) of
 *   |warp(H_est) - warp(H_gt)| in f64; 999.0 where n_inliers == 0 or match_count < 4.  H_gt, H_est (pairs, 9) f64 on the device. */
int xp_pair_eval_warp_near(const int* kp, const int* counts, int pairs, int cap, int H, int W, const double* map1, const double* map2,
                           int truncate, double* warped, uint8_t* inframe, float* near_dist, void* stream);
int xp_pair_eval_match_dist(const int* kp, const int* counts, const double* warped, const int* match_q, const int* match_t,
                            const int* match_count, int pairs, int cap, float* dist, void* stream);
int xp_pair_eval_count(const float* near_dist, const uint8_t* inframe, const int* counts, const float* dist, const int* match_count, int pairs,
                       int cap, const float* thresholds_host, int T, int near_inframe_only, int* near_cnt, int* match_cnt, int* n_inframe,
                       void* stream);
int xp_pair_eval_corner_error(const double* H_gt, const double* H_est, const int* n_inliers, const int* match_count, int pairs, int H, int W,
                              double* err, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Perspective warp — the reference's registration output:
 *     cv2.warpPerspective(im_optical, H_est, im_optical.shape[:2][::-1], borderMode=cv2.BORDER_CONSTANT)
 * (predict_align_image_pair.py:308, demo.py:225-249): INTER_LINEAR, border value 0, M (batch, 9) f64 ON THE DEVICE = the forward
 * map src -> dst (what xp_find_homography writes), inverted on the device by the closed 3 x 3 form unless inverse_map != 0
 * (cv2.WARP_INVERSE_MAP).  Arithmetic = OpenCV's documented fixed-point scheme (source coordinates rounded to 1/32 pixel in double,
 * u8: 15-bit integer weights; f32: the same 1/32 fractions as float weights) — OpenCV is absent here: parity unpinned, the oracle
 * (oracle/csrc/oracle_kernels.c: xo_warp_perspective_u8 / _f32) states the same scheme and the GPU tests demand equality with it.
 *   src (batch, Hs, Ws, channels), dst (batch, Hd, Wd, dst_channels), channel-interleaved; dst_channels == channels, or a
 *   1-channel source replicated into dst_channels (the reference warps cv2.cvtColor(gray, COLOR_GRAY2RGB)).
 *   dtype XP_WARP_U8: u8 -> u8;  XP_WARP_F32: f32 -> f32;  XP_WARP_F32_AS_U8: f32 source in [0, 1] quantised on load as
 *   (np.clip(img, 0, 1) * 255.0).astype(np.uint8) (predict_align_image_pair.py:271) -> u8.  Hs, Ws < 32768. */
#define XP_WARP_U8 0
#define XP_WARP_F32 1
#define XP_WARP_F32_AS_U8 2
int xp_warp_perspective(const void* src, void* dst, const double* M, int batch, int Hs, int Ws, int Hd, int Wd, int channels,
                        int dst_channels, int dtype, int inverse_map, void* stream);
/* The same with a valid mask (batch, Hs, Ws) u8, nonzero = valid, for XP_WARP_F32_AS_U8 only: the source is multiplied by the mask before
 * it is quantised, as the reference's `optical *= mask_optical` (predict_align_image_pair.py:267) — an invalid pixel reads 0.  mask == NULL
 * is xp_warp_perspective. */
int xp_warp_perspective_masked(const void* src, const uint8_t* mask, void* dst, const double* M, int batch, int Hs, int Ws, int Hd, int Wd,
                               int channels, int dst_channels, int dtype, int inverse_map, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Homographic adaptation (reference homographies.py:40-300; xpoint_amd/homographies.py drives these per chunk of homographies;
 * arithmetic spec in csrc/homadapt.hip and DESIGN.md "Homographic adaptation").  All pointers are device pointers, f32 unless noted.
 *   xp_ha_warp: kornia 0.1.4 warp_perspective_tensor semantics (torch.linspace grid, plain projective division, grid_sample with
 *     align_corners = False).  src (n_src, Hs, Ws) -> dst (n_dst, Hd, Wd); dst image i samples src image i % n_src with the normalised
 *     3 x 3 matrix M[i / n_src] (row-major, the matrix kornia passes to homography_warp).  mode XP_HA_NEAREST / XP_HA_BILINEAR,
 *     padding XP_HA_ZEROS / XP_HA_REFLECTION.
 *   xp_ha_valid_mask: compute_valid_mask for K homographies Hm (K, 9) f64 (forward maps): OpenCV's INTER_NEAREST warp of ones, then the
 *     (2r+1)^2 erosion, with a zero 1-pixel frame when mask_border != 0.  mask (K, H, W) u8 in {0, 1}; tmp: K * H * W bytes (unused
 *     when erosion_radius == 0).
 *   xp_ha_gaussian: depthwise ksize x ksize filter (weights row-major) behind a reflection pad of ksize / 2, (n, H, W) -> (n, H, W).
 *   xp_ha_accumulate: the fused unwarp / aggregate / accumulate over the n_views views of one chunk.  prob (n_views, S, B, H, W) with
 *     S = 1 (XP_HA_SINGLE) or 2 (optical, thermal); M (n_views - first_direct, 9) the normalised matrices of inverse(H); mask
 *     (n_views - first_direct, H, W) u8 from xp_ha_valid_mask; acc0 / acc1 (window only) / count (B, H, W) the running sums.
 *     first_direct: view 0 is the original images (sums initialised, count = 1).  finalize: divide by count, sqrt (prod) or
 *     * 0.5 (sum), zero where count < min_count (min_count > 0). */
#define XP_HA_NEAREST 0
#define XP_HA_BILINEAR 1
#define XP_HA_ZEROS 0
#define XP_HA_REFLECTION 1
#define XP_HA_SINGLE 0
#define XP_HA_PROD 1
#define XP_HA_SUM 2
#define XP_HA_WINDOW 3
int xp_ha_warp(const float* src, float* dst, const float* M, int n_src, int n_dst, int Hs, int Ws, int Hd, int Wd, int mode, int padding,
               void* stream);
int xp_ha_valid_mask(const double* Hm, uint8_t* mask, uint8_t* tmp, int K, int H, int W, int erosion_radius, int mask_border, void* stream);
int xp_ha_gaussian(const float* src, float* dst, const float* weights, int n, int H, int W, int ksize, void* stream);
int xp_ha_accumulate(const float* prob, const float* M, const uint8_t* mask, float* acc0, float* acc1, float* count, int B, int n_views,
                     int first_direct, int H, int W, int mode, int window_size, int weighted, int finalize, float min_count, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training losses.  Replace the eager XPointLoss.descriptor_loss (dense form) and XPointLoss.detector_loss
 * (xpoint/utils/losses.py:688-755, 374-576); Python caller xpoint_amd/losses.py.
 *
 * Dense descriptor loss.  d1, d2 (B, D, Hc, Wc) f32 (NCHW), D % 16 == 0, 16 <= D <= 256; w1, w2 (B, Hc*Wc, 2) f32 = the cell centres
 * (8y+4, 8x+4) carried into the common frame, (y, x) order, or NULL (the centres themselves); v1, v2 (B, Hc*Wc) f32 cell masks or NULL
 * (ones).  With j a cell of image 2 and i a cell of image 1: s = [|w1_i - w2_j| <= threshold], dot = <d2_j, d1_i>, v = v2_j v1_i,
 *   pos = lambda_d s max(0, positive_margin - dot) v,  neg = (1 - s) max(0, dot - negative_margin) v.
 * xp_descriptor_loss_fwd writes sums (B, 3) = sum_ji of (pos + neg, pos, neg) and norm (B) = sum v2 * sum v1 (no clamp), and leaves the
 * staged split-fp16 operand planes, cell data and scales in the workspace; xp_descriptor_loss_bwd takes THAT workspace unchanged (same
 * shapes and parameters) and coef (B) device f32 = dL / d(sums[b, 0]) and writes dD1 / dD2 (B, D, Hc, Wc) (either may be NULL).
 * dot is evaluated as three fp16 products of split operands with f32 accumulation (f32-grade); inputs are scaled by one power of two per
 * sample, so any finite range is accepted.  The workspace is linear in Hc*Wc (no (HW, HW) tensor is ever written); sums run in a fixed
 * order without atomics: two calls are bit-identical and sample b's results do not depend on the other samples.  256-byte aligned workspace. */
size_t xp_descriptor_loss_workspace_bytes(int B, int D, int Hc, int Wc);
int xp_descriptor_loss_fwd(const float* d1, const float* d2, const float* w1, const float* w2, const float* v1, const float* v2, int B, int D,
                           int Hc, int Wc, float threshold, float positive_margin, float negative_margin, float lambda_d, void* workspace,
                           size_t workspace_bytes, float* sums, float* norm, void* stream);
int xp_descriptor_loss_bwd(const float* coef, int B, int D, int Hc, int Wc, float threshold, float positive_margin, float negative_margin,
                           float lambda_d, const void* workspace, size_t workspace_bytes, float* dD1, float* dD2, void* stream);

/* Detector loss with 'hard_assignment'.  logits (B, 65, Hc, Wc) f32; keypoint_map (B, 8Hc, 8Wc) f32; valid_mask (B, 8Hc, 8Wc) f32 or NULL;
 * noise (B, 64, Hc, Wc) f32 = the reference's torch.rand(labels.shape).  kind 0: cross entropy with class weights [1]*64 + [dustbin_weight];
 * kind 1: focal loss alpha (1 - pt)^gamma ce.  Outputs, all (B, Hc*Wc) unless stated: labels int32 (argmax over [3 label + noise, 2.0], first
 * maximum), valid f32 (block product of the mask), cell_loss f32 (loss * valid), cell_code int32 (bit 0 correct, 1 TP, 2 FP, 3 FN, 4 TN: the
 * statistics compare argmax softmax(logits) with label * valid), stats (B, 8) f64 = [sum cell_loss, sum valid, correct, TP, FP, FN, TN, 0],
 * summed in a fixed order.  xp_detector_loss_bwd: coef (B) device f32 = dL / d(stats[b, 0]); writes dlogits (B, 65, Hc, Wc). */
int xp_detector_loss_fwd(const float* logits, const float* keypoint_map, const float* valid_mask, const float* noise, int B, int Hc, int Wc,
                         int kind, float dustbin_weight, float alpha, float gamma, int* labels, float* valid, float* cell_loss, int* cell_code,
                         double* stats, void* stream);
int xp_detector_loss_bwd(const float* logits, const int* labels, const float* valid, const float* coef, int B, int Hc, int Wc, int kind,
                         float dustbin_weight, float alpha, float gamma, float* dlogits, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training-pair augmentation (reference xpoint/datasets/augmentation/; xpoint_amd/augmentation.py drives these; csrc/augment.hip).
 * All images are (B, H, W) f32, one channel; every call is one launch sequence for the whole batch.  H, W < 32768, H * W <= 2^30.
 *   xp_aug_warp: cv2.warpPerspective(image, Hm, (W, H), INTER_LINEAR, borderMode) with the f32 arithmetic of xp_warp_perspective;
 *     border_reflect == 0: BORDER_CONSTANT (bit-equal to xp_warp_perspective), else BORDER_REFLECT_101 (cv::borderInterpolate per
 *     tap; a dimension of 1 gives 0).  Hm (B, 9) f64 forward maps.  warp (B) u8 or NULL (= all set): a sample with warp[b] == 0 is
 *     copied, and mask[b] (mask (B, H, W) u8 or NULL, filled by xp_ha_valid_mask BEFORE this call) is set to all ones.
 *   xp_aug_scatter_labels: kp_out = generate_keypoint_map(filter_points(warp_keypoints(nonzero(kp_in), Hm))): (x', y') =
 *     trunc((X / W, Y / W)) in f64, kept when inside after the truncation toward zero; kp_out is cleared first.  warp[b] == 0 copies.
 *   xp_aug_random_field: out (B, npix) f32, element p of field b from Philox4x32-10 with counter (p, 0, 0, seed >> 32) and key
 *     (seed & 0xffffffff, sample_ids[b] * 8 + primitive): XP_AUG_FIELD_UNIFORM (x0 >> 8) * 2^-24, XP_AUG_FIELD_NORMAL
 *     sqrt(-2 ln(1 - u0)) cos(2 pi u1).  sample_ids (B) int32 on the device, < 2^29.  primitive: 0..8; 8 (XP_SYNTH_KEY_TEXTURE) has the key
 *     of primitive 0 of sample id + 1: the texture of sample id and the Gaussian-noise field of sample id + 1 read one stream.
 *   xp_aug_photo_prologue: partials (B, xp_aug_partials_per_sample(H, W)) f64 partial sums of the images; shade (B, H, W) f32 or
 *     NULL: the 0/1 union of n_ellipses rotated ellipses per sample, ellipses (B, n_ellipses, 6) f64 = (cx, cy, a, b, cos, sin),
 *     inside iff ((dx cos + dy sin) / a)^2 + ((dy cos - dx sin) / b)^2 <= 1 in f64.
 *   xp_aug_blur: one pass (vertical != 0: along y) of a separable filter behind BORDER_REFLECT_101 (any radius); weights (B, kmax)
 *     f32, ksizes (B) int32 in 1..kmax, odd.
 *   xp_aug_photo_step: step `step` of every sample's program: ops (B, n_steps) int32 XP_AUG_* opcodes, params (B, n_steps) f32 (stddev,
 *     prob, delta, strength, transparency, motion ksize <= 11).  partials_in: the partial sums of src (from the prologue or the previous
 *     step; read by XP_AUG_CONTRAST in a fixed order); partials_out: those of dst.  shade: the blurred mask (XP_AUG_SHADE);
 *     motion_kernels (B, 121) f32 row-major ksize x ksize (XP_AUG_MOTION_BLUR: cv2.filter2D, correlation, centre anchor,
 *     BORDER_REFLECT_101); field_gauss / field_speckle (B, H, W) f32 or NULL = generated as xp_aug_random_field does with primitive = the
 *     opcode.  A step whose table is NULL, or whose opcode is unknown, copies. */
#define XP_AUG_GAUSSIAN_NOISE 0
#define XP_AUG_SPECKLE_NOISE 1
#define XP_AUG_BRIGHTNESS 2
#define XP_AUG_CONTRAST 3
#define XP_AUG_SHADE 4
#define XP_AUG_MOTION_BLUR 5
#define XP_AUG_FIELD_UNIFORM 0
#define XP_AUG_FIELD_NORMAL 1
int xp_aug_partials_per_sample(int H, int W);
int xp_aug_warp(const float* src, float* dst, const double* Hm, const uint8_t* warp, uint8_t* mask, int B, int H, int W, int border_reflect,
                void* stream);
int xp_aug_scatter_labels(const uint8_t* kp_in, uint8_t* kp_out, const double* Hm, const uint8_t* warp, int B, int H, int W, void* stream);
int xp_aug_random_field(float* out, unsigned long long seed, const int* sample_ids, int primitive, int kind, int B, int npix, void* stream);
int xp_aug_photo_prologue(const float* images, double* partials, const double* ellipses, float* shade, int n_ellipses, int B, int H, int W,
                          void* stream);
int xp_aug_blur(const float* src, float* dst, const float* weights, const int* ksizes, int kmax, int B, int H, int W, int vertical,
                void* stream);
int xp_aug_photo_step(const float* src, float* dst, const int* ops, const float* params, int step, int n_steps, const double* partials_in,
                      double* partials_out, const float* shade, const float* motion_kernels, const float* field_gauss,
                      const float* field_speckle, unsigned long long seed, const int* sample_ids, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense backward of head training (xpoint_amd/training.py drives these; csrc/train_dense.hip; reference call sites
 * XPoint.py:112-138 head convolutions and BatchNorms in training mode, :366 F.normalize).  All matrices are f32 rows with a leading dimension.
 *
 * xp_gemm_tn_h2: out[i][j] = sum_m P[m][i] Q[m][j] — the weight gradient of a linear layer.  P (M, I) rows with ldp is the GRADIENT operand,
 * Q (M, J) rows with ldq the activation (a column slice of a wider matrix is passed as the slice's first column and the wide ld); out (I, J)
 * rows with ldo; nothing outside that window is written.  f32-grade: both operands are split into two fp16 planes, three products per multiply
 * on the f16 matrix pipe (csrc/gemm_h2_core.h).  P is multiplied by one power of two S per call, taken on the device from its largest magnitude
 * (max|P| S in [2^13, 2^14)), and the result by 1 / S: exact, any finite range of P is accepted, an all-zero P gives exact zeros; |Q| < 65504.
 * Non-finite elements of P take no part in the choice of S (the maximum is over the finite part; an infinite maximum gives S = 1) and pass through the
 * split as they are: every output they touch is NaN / Inf, nothing is hidden.
 * p_scale NULL: S is found here.  p_scale != NULL: a device float[2] = {S, 1 / S} and P ALREADY holds S x the gradient (xp_bn_train_bwd writes both).
 * M is cut into chunks of XP_WGRAD_CHUNK rows — a constant of the build, independent of the shape and the device; the chunks' partial results go to
 * the workspace and are added in chunk order: no atomics, two calls are bit-identical.  Workspace: xp_gemm_tn_h2_workspace_bytes(M, I, J) =
 * 4352 + ceil(M / XP_WGRAD_CHUNK) I J 4 bytes, 256-byte aligned.
 * xp_conv3x3_wgrad_h2: the same with Q = the im2col view of the NHWC input x (batch, H, W, Ci) under reflection padding 1, stride 1 (columns in
 * (ky, kx, ci) order), P = dy (batch H W, Co): dw (Co, 3, 3, Ci), bit-equal to xp_gemm_tn_h2 on the materialised im2col matrix.  Any other
 * stride / reflect_pad is refused.  Workspace: xp_gemm_tn_h2_workspace_bytes(batch H W, Co, 9 Ci).  The input gradient of the reflection-padded
 * convolution is xp_conv3x3_rp_dgrad_h2 (the zero-padded one has xp_conv3x3_dgrad_h2), both below. */
#define XP_WGRAD_CHUNK 256
size_t xp_gemm_tn_h2_workspace_bytes(int M, int I, int J);
int xp_gemm_tn_h2(const float* P, const float* Q, float* out, int M, int I, int J, int ldp, int ldq, int ldo, const float* p_scale,
                  void* workspace, size_t workspace_bytes, void* stream);
int xp_conv3x3_wgrad_h2(const float* x, const float* dy, float* dw, int batch, int H, int W, int Ci, int Co, int stride, int reflect_pad,
                        const float* dy_scale, void* workspace, size_t workspace_bytes, void* stream);
/* BatchNorm in training mode over (rows, C) NHWC rows (nn.BatchNorm2d, XPoint.py:64-72,120,136).  Channel sums run in a fixed order with f64
 * accumulators (64 row groups of 8 lanes each, added in lane and group order; the statistics on data shifted by the channel's first element):
 * bit-identical between calls.  Workspace for all three entry points below: xp_bn_workspace_bytes(C), 256-byte aligned.
 * xp_bn_train_fwd: save_mean (2, C) = the f32 mean and the f32 remainder of the f64 mean (x - mean is formed from both, which keeps the data's
 *   precision when |mean| >> the deviation; row 0 is what the running statistics take), save_invstd (C) = 1 / sqrt(biased var + eps), batch_var (C)
 *   (biased; may be NULL), y = (x - mean) invstd gamma + beta.  rows >= 2.
 * xp_bn_train_bwd: dgamma = sum dy xhat, dbeta = sum dy (either may be NULL), dx = gamma invstd (dy - dbeta / rows - xhat dgamma / rows).
 *   relu_mask != 0: dx is multiplied by [x > 0] — the trunk's order is conv -> ReLU -> BatchNorm, so x is the ReLU's output and dx the gradient of
 *   the convolution's output.  dx_scale != NULL: a device float[2] that receives {S, 1 / S} with max|dx| S in [2^13, 2^14), and dx is written as
 *   S x the gradient: the operand format xp_gemm_tn_h2 (p_scale) and xp_gemm_nt_h2 (1 / S in the epilogue's scale vector) read next.
 * xp_colsum_rows: out[c] = sum_r x[r][c] by the same reduction (the bias gradients); x_scale != NULL: the sum is multiplied by x_scale[1]. */
size_t xp_bn_workspace_bytes(int C);
int xp_bn_train_fwd(const float* x, int ldx, const float* gamma, const float* beta, float* y, int ldy, float* save_mean, float* save_invstd,
                    float* batch_var, int64_t rows, int C, float eps, void* workspace, size_t workspace_bytes, void* stream);
int xp_bn_train_bwd(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* save_mean /* (2, C) */, const float* save_invstd,
                    float* dx, int lddx, float* dgamma, float* dbeta, float* dx_scale, int relu_mask, int64_t rows, int C, void* workspace,
                    size_t workspace_bytes, void* stream);
int xp_colsum_rows(const float* x, int ldx, int64_t rows, int C, const float* x_scale, float* out, void* workspace, size_t workspace_bytes,
                   void* stream);
/* Backward of xp_l2norm_rows (y = x / max(|x|, eps)): dx = (dy - y <dy, y>) / |x| for |x| >= eps, dy / eps below (torch's F.normalize: the
 * clamp passes no gradient to the norm).  x (rows, C) with ldx is the forward's INPUT; dy, dx (rows, C) contiguous. */
int xp_l2norm_rows_bwd(const float* x, int ldx, const float* dy, float* dx, int64_t rows, int C, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training of the homography head (xpoint_amd/training.py RegNetHead; csrc/train_dense.hip (weight gradient), csrc/train_dgrad.hip (input gradient), csrc/train_regnet.hip; reference
 * xpoint/models/RegNet.py:12-42 in training mode).  The head's layers are conv3x3 (ZERO padding 1, stride 1, no bias) -> BatchNorm -> ReLU, so the
 * ReLU gates below read the BatchNorm output and xp_bn_train_bwd runs with relu_mask = 0.
 *
 * xp_conv3x3_zp_wgrad_h2: dw (Co, 3, 3, Ci) of the zero-padded convolution, x (batch, H, W, Ci), dy (batch, H, W, Co).  The kernel, chunking
 *   (XP_WGRAD_CHUNK), scale contract (dy_scale NULL or {S, 1 / S}) and workspace (xp_gemm_tn_h2_workspace_bytes of (batch H W, Co, 9 Ci)) of
 *   xp_conv3x3_wgrad_h2; a tap outside the image contributes 0.  Bit-equal to xp_gemm_tn_h2 on the materialised zero-padded im2col.  H, W >= 1.
 * xp_conv3x3_dgrad_h2: the input gradient dx (batch, H, W, Ci) of the same convolution from dy (batch, H, W, Co) and w (Co, 3, 3, Ci) — the forward
 *   zero-padded convolution of dy with wr[ci][ky][kx][co] = w[co][2 - ky][2 - kx][ci] on the engine of xp_conv3x3_nhwc_h2 (f32-grade, no atomics, two
 *   calls bit-identical).  dy_scale != NULL: a device float[2] {S, 1 / S} and dy ALREADY holds S x the gradient (what xp_bn_train_bwd writes);
 *   NULL: S is taken here from the largest magnitude of dy (max|dy| S in [2^13, 2^14)) and a scaled copy in the workspace is what the engine reads,
 *   so any finite gradient range is accepted.  dx is the UNSCALED gradient (1 / S is applied, exactly, by the epilogue).  Co % 4 == 0 (the engine
 *   loads dy in 4-element channel groups); |w| is unrestricted (row scales of the offline split).  Workspace:
 *   xp_conv3x3_dgrad_h2_workspace_bytes, 256-byte aligned.  The reflection-padded convolution has xp_conv3x3_rp_dgrad_h2 and the stride-2 one
 *   xp_conv3x3_s2_dgrad_h2, both below.
 * xp_relu_fwd: y = max(x, 0) over n elements.  xp_relu_bwd: dy = dr where y > 0, else 0 (y the ReLU's input or its output).
 * xp_maxpool2_relu_bwd: backward of MaxPool2d(2) over ReLU(y), y (batch, H, W, C) the BatchNorm output, dpool (batch, H / 2, W / 2, C):
 *   dy = dpool of the window at the FIRST position, in row-major order inside the window, that attains the window's maximum, provided the maximum is
 *   > 0; 0 everywhere else, the trailing row / column of an odd H / W included (MaxPool2d floors).  torch's choice element for element: ties at 0 are
 *   closed by the ReLU, positive ties go to the first index.
 * xp_costvolume_mean_bwd: backward of xp_costvolume_mean: da[n][p][:] = dv[n][p] m[n][:] with m = mean_q b[n][q], db[n][q][:] =
 *   (sum_p dv[n][p] a[n][p][:]) / hw for every q; the sums over positions run in ascending order.  a, b, da, db (batch, hw, C), dv (batch, hw); C <= 4096.
 * xp_dropout_rows: y = x keep / (1 - p) over (rows, C) rows.  use_mask == 0: keep[r][c] = [u >= p] with u the first word of the Philox4x32-10 of
 *   csrc/philox.h (the augmentation's generator) keyed by (seed, sample_ids[r], tag) with counter c, as (word >> 8) 2^-24 — a sample's mask does
 *   not depend on its batch neighbours; mask (u8, may be NULL) receives keep.  use_mask != 0: the given mask is applied (the backward pass, and
 *   replaying recorded masks).  0 <= p < 1, 0 <= tag < 8, rows <= 65535. */
int xp_conv3x3_zp_wgrad_h2(const float* x, const float* dy, float* dw, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t xp_conv3x3_dgrad_h2_workspace_bytes(int batch, int H, int W, int Ci, int Co);
int xp_conv3x3_dgrad_h2(const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                        void* workspace, size_t workspace_bytes, void* stream);
int xp_relu_fwd(const float* x, float* y, int64_t n, void* stream);
int xp_relu_bwd(const float* dr, const float* y, float* dy, int64_t n, void* stream);
int xp_maxpool2_relu_bwd(const float* dpool, const float* y, float* dy, int batch, int H, int W, int C, void* stream);
int xp_costvolume_mean_bwd(const float* a, const float* b, const float* dv, float* da, float* db, int batch, int hw, int C, void* stream);
int xp_dropout_rows(const float* x, float* y, unsigned char* mask /* u8, in or out */, int use_mask, unsigned long long seed, const int* sample_ids,
                    int tag, float p, int rows, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training of a VSS encoder block (xpoint_amd/training.py VSSBlock; csrc/train_vss.hip, xp_scale_grad in csrc/train_dense.hip behind csrc/train_scale.h; DESIGN.md section 16;
 * reference VMamba.py:1153-1234 with the SS2D of forwardv2 / forward_corev2).  The block's dense layers run on xp_gemm_nt_h2 / xp_gemm_tn_h2 /
 * xp_colsum_rows and its SS2D core on xp_cross_scan / xp_selective_scan_fwd_x / xp_selective_scan_bwd_typed / xp_cross_merge; the entries below are
 * the HBM-bound rest.  All tensors are contiguous f32 rows; no atomics: every cross-row sum runs in a fixed order with f64 accumulators (the
 * reduction of xp_bn_train_bwd: 64 row groups of 8 lanes, lanes then groups in order), so two calls are bit-identical.
 *
 * dx_scale (xp_layernorm_bwd, xp_dwconv3x3_silu_bwd, xp_gelu_bwd): NULL, or a device float[2] that receives {S, 1 / S} with max|dx| S in
 *   [2^13, 2^14); dx is then written as S x the gradient — xp_bn_train_bwd's contract, the operand format xp_gemm_tn_h2 (p_scale) and
 *   xp_gemm_nt_h2 (1 / S in the epilogue's scale vector) read next.  An all-zero dx gives S = 1; non-finite elements take no part in S.
 * xp_scale_grad: the same for a gradient that arrives from elsewhere (the block's incoming dy, the scan / cross-merge backward): out = S g over n
 *   elements (out may be g), scale_out = {S, 1 / S}; built from the amax / power-of-two / scale kernels of xp_gemm_tn_h2.  Any finite range is
 *   accepted.  Workspace: xp_scale_grad_workspace_bytes() = 4352 bytes.
 * xp_layernorm_bwd: backward of xp_layernorm (gelu = 0) over (rows, C): x is the forward's INPUT; mean and rstd are recomputed per row with the
 *   forward's lane geometry and arithmetic, so xhat = (x - mean) rstd is the forward's xhat bit for bit.  With g = gamma dy:
 *   dx = rstd (g - mean_c(g) - xhat mean_c(g xhat)) (the row sums and the bracket in f64), dgamma = sum_r dy xhat, dbeta = sum_r dy (either may be
 *   NULL).  rows >= 1, C a multiple of 4 up to 1024, pointers 16-byte aligned.  Workspace: xp_layernorm_bwd_workspace_bytes(rows, C), 256-byte aligned.
 * xp_dwconv3x3_silu_bwd: backward of xp_dwconv3x3_silu (zero padding 1, no bias, w9c (9, C)): z = dwconv(x) is recomputed,
 *   dz = dy sigma(z) (1 + z (1 - sigma(z))) goes to the workspace, dx = the convolution of dz with the taps mirrored (a tap outside the image
 *   contributes 0; nothing crosses a sample boundary, so a sample's dx does not depend on its batch neighbours), dw9c[t][c] = sum_{b,y,x} dz
 *   x_shifted(t) (may be NULL).  C a multiple of 4, H, W >= 1.  Workspace: xp_dwconv3x3_silu_bwd_workspace_bytes(batch, H, W, C), 256-byte aligned.
 * xp_gelu_fwd: y = GELU(x) with the function of the GEMM epilogue's act = 1 (erf form), so a dense launch with act = 0 followed by xp_gelu_fwd
 *   equals the same launch with act = 1 bit for bit.  xp_gelu_bwd: dx = dy (Phi(x) + x phi(x)); workspace (4352 bytes) only with dx_scale.
 * xp_add_scaled_rows: y = x + s[b] r over (batch rows_per_sample, C) rows, s (batch) f32: the residual add under stochastic depth.  x = NULL:
 *   y = s[b] r, its backward.  y may alias x or r.  batch <= 65535. */
size_t xp_scale_grad_workspace_bytes(void);
int xp_scale_grad(const float* g, float* out, int64_t n, float* scale_out, void* workspace, size_t workspace_bytes, void* stream);
size_t xp_layernorm_bwd_workspace_bytes(int64_t rows, int C);
int xp_layernorm_bwd(const float* dy, const float* x, const float* gamma, float* dx, float* dgamma, float* dbeta, int64_t rows, int C, float eps,
                     float* dx_scale, void* workspace, size_t workspace_bytes, void* stream);
size_t xp_dwconv3x3_silu_bwd_workspace_bytes(int batch, int H, int W, int C);
int xp_dwconv3x3_silu_bwd(const float* x, const float* w9c, const float* dy, float* dx, float* dw9c, int batch, int H, int W, int C, float* dx_scale,
                          void* workspace, size_t workspace_bytes, void* stream);
int xp_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
int xp_gelu_bwd(const float* dy, const float* x, float* dx, int64_t n, float* dx_scale, void* workspace, size_t workspace_bytes, void* stream);
int xp_add_scaled_rows(const float* x, const float* r, const float* s, float* y, int batch, int64_t rows_per_sample, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The SS2D core of VSS-block training in pixel layout (xpoint_amd/training/ops.py ss2d_core, the block's `ss2d_core = "pixel"`; csrc/train_ss2d.hip;
 * DESIGN.md section 24): cross-scan, the four-route selective scan (d_state 1, softplus, D and dt bias) and cross-merge as ONE operator that reads and
 * writes rows of the (batch, H, W) pixel grid only — no (batch, 4, C, L) tensor anywhere.  M = batch H W, f32, contiguous unless a stride is named:
 *   u (M, C); dtp (M, 4, C) the dt projection BEFORE bias and softplus; bc: the B / C pair of pixel m and route k at bc[m bc_ld + k bc_kstride + {0, 1}]
 *   (the x_proj row (M, 4, R + 2) itself: bc = row + R, bc_ld = 4 (R + 2), bc_kstride = R + 2); A = -exp(A_logs), Ds, dt_bias: (4, C).
 *   Route k in the reference's order (0 row-major, 1 column-major, 2 and 3 their reverses).
 * xp_ss2d_train_fwd: ym (M, C) = (y_0 + y_2) + (y_1 + y_3), xp_cross_merge's order of additions.  It leaves the state entering every chunk of every
 *   route and the chunk's decay product in the workspace, which is all the backward needs of the forward: hand the SAME workspace, untouched, to
 *   xp_ss2d_train_bwd with the same inputs, shape and chunk.
 * xp_ss2d_train_bwd: from dym (M, C): du (M, C), ddtp (M, 4, C), dbc (M, 4, 2) = (dB, dC) per pixel and route, dA, dD, ddt_bias (4, C) each (dA is the
 *   gradient of A, not of A_logs).  h is rebuilt per chunk in LDS.
 * chunk: the number of route steps a workgroup owns: 0 = the library's choice (16 up to C = 128, 8 up to C = 512, 4 above), else a power
 *   of two in [2, 64] with chunk C <= 6144.  An argument of the call, not a process-wide setting; results of different chunks agree to rounding.
 * No atomics: two calls are bit-identical; ym, du, ddtp and dbc of a sample do not depend on the other samples of the call; an all-zero dym gives
 *   all-zero gradients; dA / dD / ddt_bias add per-(sample, chunk) partials in that order in f64.  batch in [1, 65535], C in [1, 1024],
 *   batch H W 4 C < 2^31 (32-bit element offsets), dstate must be 1.  Workspace: xp_ss2d_train_workspace_bytes(batch, H, W, C, chunk) (0 for
 *   arguments the entry points refuse), 256-byte aligned. */
size_t xp_ss2d_train_workspace_bytes(int batch, int H, int W, int C, int chunk);
int xp_ss2d_train_fwd(const float* u, const float* dtp, const float* bc, int64_t bc_ld, int64_t bc_kstride, const float* A, const float* Ds,
                      const float* dt_bias, float* ym, void* workspace, size_t workspace_bytes, int batch, int H, int W, int C, int dstate, int chunk,
                      void* stream);
int xp_ss2d_train_bwd(const float* u, const float* dtp, const float* bc, int64_t bc_ld, int64_t bc_kstride, const float* A, const float* Ds,
                      const float* dt_bias, const float* dym, float* du, float* ddtp, float* dbc, float* dA, float* dD, float* ddt_bias,
                      void* workspace, size_t workspace_bytes, int batch, int H, int W, int C, int dstate, int chunk, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training of the whole VMamba encoder (xpoint_amd/training/encoder.py VSSEncoder; csrc/train_dense.hip (weight gradients), csrc/train_dgrad.hip (input gradient), csrc/elementwise.hip; DESIGN.md section 19;
 * reference VMamba.py:1405-1440 patch embed and downsample v3, :1507-1525 VSSM.forward): the strided layers between the VSS blocks.  The convolution
 * is 3x3, ZERO padding 1, STRIDE 2: x (batch, H, W, Ci), y / dy (batch, Ho, Wo, Co) with Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, w (Co, 3, 3, Ci).
 *
 * xp_conv3x3_s2_wgrad_h2: dw (Co, 3, 3, Ci): tap (ky, kx) of output pixel (yo, xo) reads x at (2 yo + ky - 1, 2 xo + kx - 1) and contributes 0 outside
 *   the image.  A stride mode of the kernel of xp_conv3x3_wgrad_h2 with the rest of its contract: XP_WGRAD_CHUNK row chunks added in chunk order,
 *   dy_scale NULL or {S, 1 / S}, workspace xp_gemm_tn_h2_workspace_bytes(batch Ho Wo, Co, 9 Ci), bit-equal to xp_gemm_tn_h2 on the materialised
 *   stride-2 im2col matrix.  H, W >= 1, any Ci.
 * xp_conv3x3_s2_dgrad_h2: the input gradient dx (batch, H, W, Ci) from dy (batch, Ho, Wo, Co) and w; H and W are the caller's (Ho does not determine
 *   H).  A transposed convolution as FOUR implicit GEMMs on the split-fp16 engine, one per parity class of the dx pixel (y, x): a pixel receives
 *   only the taps with y + 1 - ky and x + 1 - kx even, from dy at ((y + 1 - ky) / 2, (x + 1 - kx) / 2), which is 1, 2, 2 or 4 taps; a class's
 *   reduction length is its taps x Co over its slice of one rearranged weight that xp_split_weights_h2 splits once per call.  No zero-stuffed copy of
 *   dy and no products with structural zeros.  Co % 16 == 0 with a dy below 2 GB runs the row-stationary form (a k-step lies inside one tap, so the
 *   tap and channel advance as scalars and a pixel's geometry is worked out once per tap), anything else the tile-engine form; both walk K in the same
 *   order and give the same bits.  The summation order is fixed (taps in (ky, kx) order, channels ascending), no atomics: two calls are
 *   bit-identical and a sample's dx does not depend on its batch neighbours (given dy_scale).  Scale contract of xp_conv3x3_dgrad_h2: dy_scale NULL:
 *   S is taken here and a scaled copy of dy in the workspace is what the engine reads; else dy already holds S x the gradient; dx is the unscaled
 *   gradient (1 / S applied exactly); any finite range.  Co % 4 == 0, dy 16-byte aligned.  Workspace: xp_conv3x3_s2_dgrad_h2_workspace_bytes, 256-byte
 *   aligned.
 * xp_stem_conv: the stem's convolution alone (1 -> Co channels, w9co (9, Co) the weight folded over the three identical input channels, + bias), the
 *   device definition xp_stem_conv_ln_gelu fuses with its LayerNorm and GELU (csrc/glue_core.h): xp_stem_conv -> xp_layernorm -> xp_gelu_fwd is the
 *   training forward.  f32 only (xp_set_amp_mode is not looked at); Co 48 or 16.
 * xp_stem_conv_wgrad: dw9co[t][co] = sum_{b,yo,xo} dy[b, yo, xo, co] img[b, 2 yo + ky - 1, 2 xo + kx - 1] in the fixed order and with the f64
 *   accumulators of xp_colsum_rows; dy_scale != NULL: the sums are multiplied by dy_scale[1].  The bias gradient is xp_colsum_rows; the image gets
 *   no gradient.  Workspace: xp_stem_conv_wgrad_workspace_bytes(Co). */
int xp_conv3x3_s2_wgrad_h2(const float* x, const float* dy, float* dw, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t xp_conv3x3_s2_dgrad_h2_workspace_bytes(int batch, int H, int W, int Ci, int Co);
int xp_conv3x3_s2_dgrad_h2(const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                           void* workspace, size_t workspace_bytes, void* stream);
int xp_stem_conv(const float* img, const float* w9co, const float* bias, float* y, int batch, int H, int W, int Co, void* stream);
size_t xp_stem_conv_wgrad_workspace_bytes(int Co);
int xp_stem_conv_wgrad(const float* img, const float* dy, float* dw9co, int batch, int H, int W, int Co, const float* dy_scale, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training of the whole XPoint (xpoint_amd/training/model.py XPointNet; csrc/train_dgrad.hip): the input gradient of the head
 * trunk's REFLECTION-padded 3x3 convolution (XPoint.py:112-138), which carries the heads' loss into the encoder.
 *
 * xp_conv3x3_rp_dgrad_h2: dx (batch, H, W, Ci) from dy (batch, H, W, Co) and w (Co, 3, 3, Ci), the contract of xp_conv3x3_dgrad_h2: dy_scale NULL
 *   (S is taken here from max|dy|, any finite range) or a device float[2] {S, 1 / S} for a dy that already holds S x the gradient (what
 *   xp_bn_train_bwd writes); dx is the UNSCALED gradient.  With g the zero-padded input gradient on the padded frame (rows -1 .. H, columns
 *   -1 .. W), dx[y][x] = sum of g[v][u] over v in {y} + {-1 if y == 1} + {H if y == H - 2} and u likewise: the interior term is
 *   xp_conv3x3_dgrad_h2's launch as it stands; the frame (2 (W + 2) + 2 H pixels per image, three taps each) is twelve thin implicit GEMMs (four
 *   sides x three taps, K = Co each) on the split-fp16 tile engine over the slices of one rearranged weight that is split once per call; a last
 *   kernel adds the three tap planes and the frame terms to the pixels of rows and columns 1 and n - 2 in a fixed order.  No (H + 2) x (W + 2)
 *   copy of dy or dx, no atomics: two calls are bit-identical and a sample's dx does not depend on its batch neighbours (given dy_scale).
 *   Co % 4 == 0, H, W >= 2 (reflection needs 2), the shape limits of xp_conv3x3_dgrad_h2 otherwise; beyond its contract: dy 16-byte aligned and
 *   12 Ci pad32(Co) < 2^31 (the rearranged weight's elements).
 *   Workspace: xp_conv3x3_rp_dgrad_h2_workspace_bytes, 256-byte aligned. */
size_t xp_conv3x3_rp_dgrad_h2_workspace_bytes(int batch, int H, int W, int Ci, int Co);
int xp_conv3x3_rp_dgrad_h2(const float* dy, const float* w, float* dx, int batch, int H, int W, int Ci, int Co, const float* dy_scale,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The optimiser step (xpoint_amd/training/optim.py Adam; csrc/optim.hip): the global gradient norm, a device record that
 * decides whether the step is applied, and torch.optim.Adam's update (L2 weight decay, amsgrad off) in f32 over every tensor.  The pointer and count
 * arrays are HOST arrays of n_tensors entries; they travel to the device BY VALUE in the kernel arguments, 64 tensors per launch, so the caller may
 * reuse them as soon as the call returns.  No atomics, no host read-back, no allocation: the three calls of a step may be captured.
 *
 * xp_optim_grad_sumsq: every workgroup writes ONE f64 partial sum of g^2 over its 8192 elements of one tensor into workspace[slot], the slot fixed
 *   by (tensor index, offset); *n_partials (host) receives the number of slots = sum_j ceil(counts[j] / 8192).  16-byte loads where a gradient's
 *   address allows, 4-byte ones where not (a lane owns the same elements either way).  Workspace: xp_optim_workspace_bytes(n_tensors, sum of
 *   counts) (an upper bound), 8-byte aligned.
 * xp_optim_step_header: one workgroup adds the partials in a fixed order and writes the record at `header` (xp_optim_header_bytes() = 64 bytes,
 *   8-byte aligned, zeroed by the caller before the first step), eight 8-byte words:
 *     f64 norm2 | f64 bc1 = 1 - beta1^t | f64 bc2 = 1 - beta2^t | f64 clip_coef | i64 t | i64 skipped | i64 finite | i64 applied
 *   finite = norm2 is finite (an inf or NaN in any gradient makes it not: the whole detection); applied = finite or !skip_nonfinite; t advances
 *   only when applied, else `skipped` does; clip_coef = min(1, max_norm / (sqrt(norm2) + 1e-6)), or 1 when max_norm <= 0 (clipping off).
 * xp_optim_adam_apply: reads the record; applied == 0: writes NOTHING.  Else per element, in f32 with no contraction:
 *     g' = clip_coef g + wd p;  m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 *   m, v at exp_avg / exp_avg_sq + moment_offsets[j] (flat buffers of moment_elements floats, 16-byte aligned; [offset, offset + count) must lie
 *   inside).  16-byte accesses per array where its address allows, 4-byte ones where not: any 4-byte aligned pointer and any offset are handled,
 *   and an element's result does not depend on its tensor's alignment or place in the table.
 * Null pointers, non-positive counts and a short workspace return an error. */
size_t xp_optim_header_bytes(void);
size_t xp_optim_workspace_bytes(int n_tensors, int64_t total_elements);
int xp_optim_grad_sumsq(const float* const* grads, const int64_t* counts, int n_tensors, void* workspace, size_t workspace_bytes, int64_t* n_partials,
                        void* stream);
int xp_optim_step_header(const void* workspace, int64_t n_partials, void* header, double beta1, double beta2, double max_norm, int skip_nonfinite,
                         void* stream);
int xp_optim_adam_apply(float* const* params, const float* const* grads, const int64_t* moment_offsets, const int64_t* counts, int n_tensors,
                        float* exp_avg, float* exp_avg_sq, int64_t moment_elements, const void* header, double lr, double weight_decay, double beta1,
                        double beta2, double eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SyntheticShapes on the device (xpoint_amd/synthetic_shapes.py drives these; csrc/synth_shapes.hip; DESIGN.md "Synthetic shapes"; reference
 * xpoint/utils/draw_primitives.py, xpoint/datasets/SyntheticShapes.py).  Frames are (B, H, W) f32, one channel, H, W <= 4096.  Every table is
 * per image; nothing of image b depends on its batch neighbours, no launch count depends on B, two calls agree bit for bit.
 *   xp_synth_background: frame = [u > thresholds[b]] with u the xp_aug_random_field uniform of (seed, sample_ids[b], XP_SYNTH_KEY_BACKGROUND),
 *     then n_blobs (<= 256) filled circles, the last covering one wins: blob_geom (B, n_blobs, 4) int32 = (cx, cy, r, 0), inside iff
 *     dx^2 + dy^2 <= r^2; colour = raw, or (raw + 0.5) % 1 where |raw - m| < min_contrast, m = the mean of the thresholded field (an integer
 *     count / (H W), written to field_mean (B) f64); blob_raw (B, n_blobs) f64.  count_ws: B * XP_SYNTH_PARTIALS ints.  Two launches.
 *   xp_synth_box_blur: cv2.blur(src, (k, k)) with k = ksizes[b] >= 1 (any parity, anchor k / 2, any size against the frame), normalised,
 *     BORDER_REFLECT_101; rows into tmp, columns into dst (dst may be src).  Window sums are f64.  Two launches.
 *   xp_synth_resolve_colours: bg_mean (B) f64 = the mean of `background` (f64 partial sums in a fixed order; partial_ws: B * XP_SYNTH_PARTIALS
 *     doubles), then colours (B, n_records) f32 from the rules, in order, in f64: rules (B, n_records, 4) int32 = (kind, ref0, ref1, candidate
 *     offset), rule_values (B, n_records, 2) f64 = (v, m).  XP_SYNTH_RULE_ABS: v.  _CONTRAST: v, or (v + 0.5) % 1 where |v - bg_mean| < m.
 *     _DIFFERENT: the first of the XP_SYNTH_CANDIDATES values at candidates[b][offset ..] that differs by >= m from the colours of records ref0
 *     and ref1 (each < the record's own index, or -1), else the last.  _REL: (colour[ref0] + m) % 1.  n_records <= XP_SYNTH_MAX_RECORDS.
 *   xp_synth_rasterise: in place over the frame; records (B, n_records, XP_SYNTH_RECORD_INTS) int32 = kind, bounding box x0 y0 x1 y1
 *     (inclusive), n, 16 geometry words, 2 spare.  The last record that covers a pixel gives its colour.  _CIRCLE (cx, cy; n = r):
 *     dx^2 + dy^2 <= r^2.  _SEGMENT (x1, y1, x2, y2; n = thickness t): within t / 2 of the segment: 4 |AP|^2 <= t^2 beyond either end,
 *     4 cross^2 <= t^2 len^2 between.  _POLYGON (n <= 8 vertices x, y): even-odd over half-open crossings, or on an edge.  _ELLIPSE (cx, cy,
 *     ax, ay, then cos and sin of the angle as two f64): ((dx cos + dy sin) / ax)^2 + ((dy cos - dx sin) / ay)^2 <= 1 in f64, a half axis of
 *     0 taken as 0.5.  _NOISE: every pixel = the uniform of (seed, sample_ids[b], XP_SYNTH_KEY_NOISE).  |coordinates| <= 16383.
 *   xp_synth_resize: cv2.resize INTER_LINEAR (B, H, W) -> (B, h, w): source coordinate (d + 0.5) (H / h) - 0.5 in f64, taps clamped to the
 *     frame, f32 weights, rows first: (t00 (1 - wx) + t01 wx) (1 - wy) + (t10 (1 - wx) + t11 wx) wy.
 *   xp_synth_scatter_points: map (B, h, w) u8 = 0, then 1 at the first counts[b] (<= cap) points of points (B, cap, 2) int32 (y, x) that lie
 *     inside.
 *
 * Textured polygons (draw_multiple_polygons; opt-in, a batch without a _TEXTURED record never reaches these two).  A _TEXTURED record is a
 * _POLYGON record whose word 22 is the box-blur size k and whose word 23 is its ordinal j among the textured records of its image.  Its pixels
 * take cv2.blur(T_j, (k, k)) (the definition of xp_synth_box_blur, reflected over the WHOLE frame), T_j(x, y) = the colour of the highest-index
 * blob i < nb_blobs with dx^2 + dy^2 <= r^2, else the record's resolved colour; blob i of texture j of sample id is four uniforms
 * u_c = the xp_aug_random_field uniform of (seed, id, XP_SYNTH_KEY_TEXTURE) at position (j nb_blobs + i) 4 + c: cx = floor(u0 W), cy = floor(u1 H),
 * r = floor(u2 20) (products in f64), colour = f32(u3, or (u3 + 0.5) % 1 where u3 < min_contrast).  No blob list is ever stored.
 *   xp_synth_texture: one JOB per textured record, work limited to the record's box dilated by the blur window.  jobs (n_jobs,
 *     XP_SYNTH_JOB_INTS) int32 = image b, record r, ordinal j, k, the record's box x0 y0 x1 y1 (inclusive, inside the frame), the texture box
 *     tx0 ty0 tx1 ty1 = the hull of the frame positions that the windows of the record's box reach after reflection, 4 spare.  offsets
 *     (n_jobs, 3) int64 = where, in floats from `arena`, the job keeps T_j over its texture box (th x tw), the row pass (th x bw) and the blurred
 *     box (bh x bw); a job whose extents leave the frame or the arena (arena_floats) is skipped.  units (3, n_jobs + 1) int32 = per launch the
 *     running count of workgroups before each job: 32 x 32 tiles of the texture box; rows of the texture box; 64-column by 256-row blocks of the
 *     record's box.  Three launches whatever B and n_jobs: the texture (blobs culled per tile in index order, the list holds all nb_blobs), the
 *     row windows (f64 prefix over the frame's row, zero outside the texture box), the column windows (f64 running sums).  min_ksize, max_ksize:
 *     the range of k over the jobs, inside [1, 500]; nb_blobs <= XP_SYNTH_MAX_TEXTURE_BLOBS.  n_tiles, n_rows, n_col_blocks: the last entry of
 *     each row of units, the three grids.
 *   xp_synth_rasterise_textured: xp_synth_rasterise with one more kind: a pixel inside a _TEXTURED record r of image b (the _POLYGON test) takes
 *     arena[tex_offsets[b][r] + (y - y0) bw + (x - x0)], the job's blurred box; tex_offsets (B, n_records) int64, negative = draws nothing. */
#define XP_SYNTH_PARTIALS 128
#define XP_SYNTH_MAX_RECORDS 128
#define XP_SYNTH_RECORD_INTS 24
#define XP_SYNTH_CANDIDATES 21
#define XP_SYNTH_KEY_BACKGROUND 6
#define XP_SYNTH_KEY_NOISE 7
#define XP_SYNTH_KEY_TEXTURE 8
#define XP_SYNTH_MAX_TEXTURE_BLOBS 4096
#define XP_SYNTH_MAX_KSIZE 500
#define XP_SYNTH_JOB_INTS 16
#define XP_SYNTH_NOP 0
#define XP_SYNTH_CIRCLE 1
#define XP_SYNTH_SEGMENT 2
#define XP_SYNTH_POLYGON 3
#define XP_SYNTH_ELLIPSE 4
#define XP_SYNTH_NOISE 5
#define XP_SYNTH_TEXTURED 6
#define XP_SYNTH_RULE_ABS 0
#define XP_SYNTH_RULE_CONTRAST 1
#define XP_SYNTH_RULE_DIFFERENT 2
#define XP_SYNTH_RULE_REL 3
int xp_synth_background(float* frame, unsigned long long seed, const int* sample_ids, const float* thresholds, const int* blob_geom,
                        const double* blob_raw, int n_blobs, double min_contrast, int* count_ws, double* field_mean, int B, int H, int W,
                        void* stream);
int xp_synth_box_blur(const float* src, float* tmp, float* dst, const int* ksizes, int B, int H, int W, void* stream);
int xp_synth_resolve_colours(const float* background, const int* rules, const double* rule_values, const double* candidates, int n_records,
                             int n_candidates, double* partial_ws, float* colours, double* bg_mean, int B, int H, int W, void* stream);
int xp_synth_rasterise(float* frame, const int* records, const float* colours, unsigned long long seed, const int* sample_ids, int n_records,
                       int B, int H, int W, void* stream);
int xp_synth_resize(const float* src, float* dst, int B, int H, int W, int h, int w, void* stream);
int xp_synth_scatter_points(const int* points, const int* counts, int cap, uint8_t* map, int B, int h, int w, void* stream);
int xp_synth_texture(float* arena, long long arena_floats, const int* jobs, const long long* offsets, const int* units, int n_jobs,
                     const float* colours, int n_records, unsigned long long seed, const int* sample_ids, int nb_blobs, double min_contrast,
                     int min_ksize, int max_ksize, int n_tiles, int n_rows, int n_col_blocks, int B, int H, int W, void* stream);
int xp_synth_rasterise_textured(float* frame, const int* records, const float* colours, unsigned long long seed, const int* sample_ids,
                                const float* arena, const long long* tex_offsets, int n_records, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline leg; replaces the
 * reference's wall-clock brackets, benchmark_evaluation.py:12-37).  Off by default.  xp_prof_filter(tag)
 * restricts recording to one kernel tag (NULL/"" = all).  xp_prof_count / xp_prof_get synchronise on the
 * recorded events and return, per tag: total ms, launches, algorithmic FLOPs and bytes of those launches. */
int xp_prof_enable(int on);
int xp_prof_filter(const char* tag);
int xp_prof_reset(void);
int xp_prof_count(void);
int xp_prof_get(int index, char* tag, int tag_len, double* total_ms, int* launches, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* XPOINT_HIP_H */
