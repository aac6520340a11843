// Host-side orchestration of the XPoint forward (reference XPoint.py:283-323 forward_impl with the
// VMamba encoder, VMamba.py:1507-1525): a fixed sequence of kernel launches on one HIP stream.
// The context is host-only metadata (model dims + the device-format parameter table); weights and
// workspace are caller-owned device buffers, so the library never allocates device memory.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "xp_common.h"
#include "../../include/xpoint_hip.h"

#define RUN(call) do { int rc__ = (call); if (rc__ != XP_OK) return rc__; } while (0)

namespace {

struct Param { std::string name; size_t offset; size_t numel; };      // the name table: xp_param_info only (the host packs the blob by it)

// A (N, K) matrix consumed by a GEMM / 3x3 conv: where it lives in the f32 blob (floats) and in its copies (bytes) — the split-bf16 planes (x3 region of
// the split-weights buffer), the split-fp16 planes (h2 region, which follows the x3 region) and the plain fp16 buffer — and its bit in xp_set_dense_override
struct Dense { size_t w, x3, h2, f16; int N, K, id, param; };
struct Block {      // one VSS block
    size_t ln1_w, ln1_b, dw_w, dt_w, dt_b, A, D, onorm_w, onorm_b, ln2_w, ln2_b, fc1_b, fc2_b;
    Dense in, xproj, out, fc1, fc2;
    bool packed;                                      // weight streams of the fused tail (out_proj + MLP) and head (in_proj), csrc/mlp_fused.hip:
    size_t pack, in_pack, h2_pack, h2_in_pack;        // x3 forms in the x3 region, h2 forms in the h2 region
};
struct Down { Dense w; size_t b, ln_w, ln_b; };
struct Stage { std::vector<Block> blocks; Down ds; };      // ds: every stage but the last
struct Stem { size_t w, b, ln_w, ln_b; Dense pe2; size_t pe2_b, pe2_ln_w, pe2_ln_b; };
struct Head { Dense w; size_t b, scale, shift; };

struct Ctx {
    xp_model_cfg cfg;
    int nstages, dims[4], ranks[4];
    std::vector<Param> params;
    Stem stem;
    Stage stages[4];
    Head head, det2, desc2;
    size_t total, split_bytes, h2_bytes;    // split_bytes: the x3 region (planes + fused-kernel packs); the h2 region follows it
    size_t f16_bytes;                        // plain fp16 (N, K) copies of the GEMM weights (fast mixed-precision class)
    size_t add(const std::string& n, size_t numel) {
        size_t off = total;
        params.push_back({n, off, numel});
        total += (numel + 3) / 4 * 4;   // keep every tensor 16-byte aligned inside the blob
        return off;
    }
    // a dense layer's matrix: also gets a slot in each derived buffer; id = its launch in the xp_set_dense_override numbering
    Dense add_gemm(const std::string& n, size_t N, size_t K, int id) {
        const Dense d{add(n, N * K), split_bytes, h2_bytes, f16_bytes, (int)N, (int)K, id, (int)params.size() - 1};
        f16_bytes += (N * K * 2 + 255) / 256 * 256;
        split_bytes += (xp_split_weights_x3_bytes((int)N, (int)K) + 255) / 256 * 256;
        h2_bytes += (xp_split_weights_h2_bytes((int)N, (int)K) + 255) / 256 * 256;
        return d;
    }
};

int conv_out(int x) { return (x - 1) / 2 + 1; }   // k3 s2 p1

// channels of the encoder output = last stage's channels after depth_to_space(4); the one expression the weight layout,
// xp_forward_shapes and the forward all use
int enc_channels_of(const Ctx& c) { return c.dims[c.nstages - 1] / 16; }

// The one pass that lays out the blob and the derived buffers, fills the typed table the forwards walk and numbers the dense launches
// (xp_set_dense_override, include/xpoint_hip.h): 0 = patch-embed conv 2; block b: 1 + 5 b + {0 in_proj, 1 x_proj, 2 out_proj, 3 fc1, 4 fc2};
// 41 + s = downsample after stage s; 44 = head trunk, 45 = detector 1x1, 46 = descriptor 1x1.
void build_layout(Ctx& c) {
    const size_t E = c.cfg.embed_dim, N = c.cfg.d_state;
    c.total = 0; c.split_bytes = 0; c.h2_bytes = 0; c.f16_bytes = 0;
    Stem& st = c.stem;
    st.w = c.add("stem.w", 9 * (E / 2)); st.b = c.add("stem.b", E / 2); st.ln_w = c.add("stem.ln_w", E / 2); st.ln_b = c.add("stem.ln_b", E / 2);
    st.pe2 = c.add_gemm("pe2.w", E, 9 * (E / 2), 0); st.pe2_b = c.add("pe2.b", E); st.pe2_ln_w = c.add("pe2.ln_w", E); st.pe2_ln_b = c.add("pe2.ln_b", E);
    // deeper configurations than 2, 2, 2, 2 clip the running block index to 7: late blocks share the last block's bits (coarser, still monotone for the host's bisection)
    int block_index = 0;
    for (int s = 0; s < c.nstages; ++s) {
        const size_t C = c.dims[s], R = c.ranks[s], H4 = (size_t)(C * c.cfg.mlp_ratio);
        c.stages[s].blocks.assign(c.cfg.depths[s], Block{});
        for (int j = 0; j < c.cfg.depths[s]; ++j) {
            Block& k = c.stages[s].blocks[j];
            const std::string b = "s" + std::to_string(s) + ".b" + std::to_string(j) + ".";
            const int id0 = 1 + 5 * std::min(block_index++, 7);
            k.ln1_w = c.add(b + "ln1_w", C); k.ln1_b = c.add(b + "ln1_b", C);
            k.in = c.add_gemm(b + "in_w", C, C, id0);
            k.dw_w = c.add(b + "dw_w", 9 * C);
            k.xproj = c.add_gemm(b + "xproj_w", 4 * (R + 2 * N), C, id0 + 1);
            k.dt_w = c.add(b + "dt_w", 4 * C * R); k.dt_b = c.add(b + "dt_b", 4 * C);
            k.A = c.add(b + "A", 4 * C * N); k.D = c.add(b + "D", 4 * C);
            k.onorm_w = c.add(b + "onorm_w", C); k.onorm_b = c.add(b + "onorm_b", C);
            k.out = c.add_gemm(b + "out_w", C, C, id0 + 2);
            k.ln2_w = c.add(b + "ln2_w", C); k.ln2_b = c.add(b + "ln2_b", C);
            k.fc1 = c.add_gemm(b + "fc1_w", H4, C, id0 + 3); k.fc1_b = c.add(b + "fc1_b", H4);
            k.fc2 = c.add_gemm(b + "fc2_w", C, H4, id0 + 4); k.fc2_b = c.add(b + "fc2_b", C);
            k.packed = xp_mlp_fused_x3_supported((int)C, (int)H4) != 0;      // the wide stages run the MLP as one launch (csrc/mlp_fused.hip)
            if (k.packed) {
                k.pack = c.split_bytes; c.split_bytes += (xp_mlp_fused_x3_pack_bytes((int)C, (int)H4, 1) + 255) / 256 * 256;
                k.in_pack = c.split_bytes; c.split_bytes += (xp_ln_proj_x3_pack_bytes((int)C, (int)C) + 255) / 256 * 256;
                k.h2_pack = c.h2_bytes; c.h2_bytes += (xp_mlp_fused_h2_pack_bytes((int)C, (int)H4, 1) + 255) / 256 * 256;
                k.h2_in_pack = c.h2_bytes; c.h2_bytes += (xp_ln_proj_h2_pack_bytes((int)C, (int)C) + 255) / 256 * 256;
            }
        }
        if (s < c.nstages - 1) {
            Down& d = c.stages[s].ds;
            const std::string n = "s" + std::to_string(s) + ".ds.";
            d.w = c.add_gemm(n + "w", 2 * C, 9 * C, 41 + s); d.b = c.add(n + "b", 2 * C); d.ln_w = c.add(n + "ln_w", 2 * C); d.ln_b = c.add(n + "ln_b", 2 * C);
        }
    }
    const size_t HC = c.cfg.head_channels, EC = enc_channels_of(c), DS = c.cfg.desc_size, DET = c.cfg.det_channels;
    c.head = {c.add_gemm("head.w", 2 * HC, 9 * EC, 44), c.add("head.b", 2 * HC), c.add("head.scale", 2 * HC), c.add("head.shift", 2 * HC)};
    c.det2 = {c.add_gemm("det2.w", DET, HC, 45), c.add("det2.b", DET), c.add("det2.scale", DET), c.add("det2.shift", DET)};
    c.desc2 = {c.add_gemm("desc2.w", DS, HC, 46), c.add("desc2.b", DS), c.add("desc2.scale", DS), c.add("desc2.shift", DS)};
}

// every dense layer, in layout order (the order the prepare functions convert them in)
template <class F> int each_dense(const Ctx& c, F f) {
    RUN(f(c.stem.pe2));
    for (int s = 0; s < c.nstages; ++s) {
        for (const Block& k : c.stages[s].blocks)
            for (const Dense* d : {&k.in, &k.xproj, &k.out, &k.fc1, &k.fc2}) RUN(f(*d));
        if (s < c.nstages - 1) RUN(f(c.stages[s].ds.w));
    }
    for (const Dense* d : {&c.head.w, &c.det2.w, &c.desc2.w}) RUN(f(*d));
    return XP_OK;
}
// every VSS block that has fused-kernel packs
template <class F> int each_packed(const Ctx& c, F f) {
    for (int s = 0; s < c.nstages; ++s)
        for (const Block& k : c.stages[s].blocks) if (k.packed) RUN(f(k));
    return XP_OK;
}

struct Shapes {
    int Hs, Ws;            // stem output
    int H[4], W[4];        // per stage
    int Hc, Wc;            // encoder output (x4 of the last stage)
    int64_t M[4];
};

bool shapes_of(const Ctx& c, int batch, int H, int W, Shapes& s) {
    s.Hs = conv_out(H); s.Ws = conv_out(W);
    s.H[0] = conv_out(s.Hs); s.W[0] = conv_out(s.Ws);
    for (int i = 1; i < c.nstages; ++i) { s.H[i] = conv_out(s.H[i - 1]); s.W[i] = conv_out(s.W[i - 1]); }
    for (int i = 0; i < c.nstages; ++i) s.M[i] = (int64_t)batch * s.H[i] * s.W[i];
    s.Hc = s.H[c.nstages - 1] * 4; s.Wc = s.W[c.nstages - 1] * 4;
    return s.H[c.nstages - 1] > 0 && s.W[c.nstages - 1] > 0;
}

struct WsPlan { size_t X, T1, T2, T3, HB, XD, SS, total_floats; size_t ss_bytes; };

WsPlan plan_ws(const Ctx& c, int batch, const Shapes& s) {
    WsPlan w{};
    size_t mc = 0, mh = 0, mx = 0, ss = 0;
    for (int i = 0; i < c.nstages; ++i) {
        const size_t MC = (size_t)s.M[i] * c.dims[i];
        mc = std::max(mc, MC);
        mh = std::max(mh, (size_t)(MC * c.cfg.mlp_ratio));
        mx = std::max(mx, (size_t)s.M[i] * 4 * (c.ranks[i] + 2 * c.cfg.d_state));
        ss = std::max(ss, xp_ss2d_core_workspace_bytes(batch, s.H[i], s.W[i], c.dims[i]));
    }
    mh = std::max(mh, (size_t)batch * s.Hs * s.Ws * (c.cfg.embed_dim / 2));           // stem output aliases HB
    mh = std::max(mh, (size_t)batch * s.Hc * s.Wc * 2 * c.cfg.head_channels);         // head trunk aliases HB
    mc = std::max(mc, (size_t)batch * s.Hc * s.Wc * (size_t)std::max(c.cfg.desc_size, c.cfg.det_channels + 3));
    auto al = [](size_t n) { return (n + 63) / 64 * 64; };
    size_t o = 0;
    w.X = o; o += al(mc); w.T1 = o; o += al(mc); w.T2 = o; o += al(mc); w.T3 = o; o += al(mc);
    w.HB = o; o += al(mh); w.XD = o; o += al(mx); w.SS = o; o += al(ss / 4 + 1);
    w.total_floats = o; w.ss_bytes = ss;
    return w;
}

// What the two forwards share: the argument checks (messages prefixed with the entry point's name), the shapes and the workspace plan.
struct Fwd { const Ctx* c; Shapes sh; WsPlan wp; };
int forward_prologue(const char* fn, void* ctx, bool pointers, int batch, int H, int W, size_t workspace_bytes, int embed_multiple, Fwd& f) {
    XP_CHECK_ARG(ctx && pointers, "%s: null pointer", fn);
    XP_CHECK_ARG(batch > 0, "%s: empty batch", fn);
    f.c = (const Ctx*)ctx;
    XP_CHECK_ARG(shapes_of(*f.c, batch, H, W, f.sh), "%s: image too small", fn);
    // The reference mis-sizes its outputs when H or W is not a multiple of 32; the drop-in refuses instead.
    XP_CHECK_ARG(H % 32 == 0 && W % 32 == 0, "%s: H and W must be multiples of 32 for the VMamba encoder (got %dx%d)", fn, H, W);
    XP_CHECK_ARG(f.sh.Hc * 8 == H && f.sh.Wc * 8 == W, "%s: encoder output %dx%d is not 1/8 of the image", fn, f.sh.Hc, f.sh.Wc);
    XP_CHECK_ARG(f.c->cfg.embed_dim % embed_multiple == 0, "%s: embed_dim must be a multiple of %d", fn, embed_multiple);
    f.wp = plan_ws(*f.c, batch, f.sh);
    XP_CHECK_ARG(workspace_bytes >= f.wp.total_floats * sizeof(float), "%s: workspace too small", fn);
    return XP_OK;
}

}  // namespace

extern "C" int xp_ctx_create(const xp_model_cfg* cfg, void** ctx_out) {
    XP_CHECK_ARG(cfg && ctx_out, "xp_ctx_create: null pointer");
    // The heads hang off depth_to_space(4) of the LAST stage and the detector's PixelShuffle(8) (XPoint.py:112-125, VMamba.py:1500-1505):
    // enc channels = dims[L] / 16 must equal embed_dim / 2 and Hc * 8 must equal H, which holds for 4 stages only.  The reference
    // raises a channel mismatch for any other depth list; so does this.
    XP_CHECK_ARG(cfg->n_stages == 4, "xp_ctx_create: the XPoint VMamba encoder has exactly 4 stages (got n_stages = %d): the head convolution "
                 "expects embed_dim / 2 channels at 1/8 resolution", cfg->n_stages);
    XP_CHECK_ARG(cfg->embed_dim % 32 == 0 && (cfg->embed_dim == 96 || cfg->embed_dim == 32),
                 "xp_ctx_create: embed_dim must be 96 (XPoint config) or 32 (reduced test model), got %d", cfg->embed_dim);
    XP_CHECK_ARG(cfg->d_state == 1, "xp_ctx_create: the fused encoder implements d_state == 1 (XPoint config); got %d", cfg->d_state);
    XP_CHECK_ARG(cfg->head_channels % 4 == 0 && cfg->desc_size > 0 && cfg->det_channels == 65, "xp_ctx_create: bad head dims");
    Ctx* c = new Ctx();
    c->cfg = *cfg;
    c->nstages = cfg->n_stages;
    for (int s = 0; s < c->nstages; ++s) {
        c->dims[s] = cfg->embed_dim << s;
        c->ranks[s] = cfg->dt_rank > 0 ? cfg->dt_rank : (c->dims[s] + 15) / 16;   // "auto" = ceil(d_model / 16), VMamba.py:414
        XP_CHECK_ARG(cfg->depths[s] >= 0, "xp_ctx_create: negative depth");
    }
    build_layout(*c);
    *ctx_out = c;
    return XP_OK;
}

extern "C" int xp_ctx_destroy(void* ctx) { delete (Ctx*)ctx; return XP_OK; }

extern "C" int xp_param_count(void* ctx) { return ctx ? (int)((Ctx*)ctx)->params.size() : -1; }
extern "C" size_t xp_weights_numel(void* ctx) { return ctx ? ((Ctx*)ctx)->total : 0; }

extern "C" int xp_param_info(void* ctx, int index, char* name, int name_len, size_t* offset, size_t* numel) {
    XP_CHECK_ARG(ctx && name && offset && numel, "xp_param_info: null pointer");
    Ctx* c = (Ctx*)ctx;
    XP_CHECK_ARG(index >= 0 && index < (int)c->params.size(), "xp_param_info: index out of range");
    const Param& p = c->params[index];
    strncpy(name, p.name.c_str(), name_len - 1); name[name_len - 1] = 0;
    *offset = p.offset; *numel = p.numel;
    return XP_OK;
}

extern "C" int xp_forward_shapes(void* ctx, int batch, int H, int W, int* Hc, int* Wc, int* enc_channels) {
    XP_CHECK_ARG(ctx, "xp_forward_shapes: null ctx");
    Ctx* c = (Ctx*)ctx; Shapes s;
    XP_CHECK_ARG(shapes_of(*c, batch, H, W, s), "xp_forward_shapes: image too small");
    if (Hc) *Hc = s.Hc; if (Wc) *Wc = s.Wc; if (enc_channels) *enc_channels = enc_channels_of(*c);
    return XP_OK;
}

extern "C" size_t xp_forward_workspace_bytes(void* ctx, int batch, int H, int W) {
    if (!ctx) return 0;
    Ctx* c = (Ctx*)ctx; Shapes s;
    if (!shapes_of(*c, batch, H, W, s)) return 0;
    return plan_ws(*c, batch, s).total_floats * sizeof(float);
}

extern "C" size_t xp_split_weights_bytes(void* ctx) { return ctx ? ((Ctx*)ctx)->split_bytes + ((Ctx*)ctx)->h2_bytes : 0; }

extern "C" int xp_prepare_split_weights(void* ctx, const float* weights, void* wsplit, size_t wsplit_bytes, void* stream) {
    XP_CHECK_ARG(ctx && weights && wsplit, "xp_prepare_split_weights: null pointer");
    Ctx* c = (Ctx*)ctx;
    XP_CHECK_ARG(wsplit_bytes >= c->split_bytes + c->h2_bytes, "xp_prepare_split_weights: buffer too small");
    XP_CHECK_ARG(((uintptr_t)wsplit & 15) == 0, "xp_prepare_split_weights: buffer must be 16-byte aligned");
    char *x3 = (char*)wsplit, *h2 = x3 + c->split_bytes;      // the two regions
    RUN(each_dense(*c, [&](const Dense& e) -> int {
        XP_CHECK_ARG(e.K % 4 == 0, "xp_prepare_split_weights: %s has K = %d, not a multiple of 4", c->params[e.param].name.c_str(), e.K);
        RUN(xp_split_weights_x3(weights + e.w, x3 + e.x3, e.N, e.K, stream));
        return xp_split_weights_h2(weights + e.w, h2 + e.h2, e.N, e.K, stream);
    }));
    RUN(each_packed(*c, [&](const Block& k) { return xp_mlp_fused_x3_pack(x3 + k.fc1.x3, x3 + k.fc2.x3, x3 + k.out.x3, x3 + k.pack, k.fc1.K, k.fc1.N, stream); }));
    RUN(each_packed(*c, [&](const Block& k) { return xp_ln_proj_x3_pack(x3 + k.in.x3, x3 + k.in_pack, k.in.N, k.in.K, stream); }));
    return each_packed(*c, [&](const Block& k) -> int {
        RUN(xp_mlp_fused_h2_pack(h2 + k.fc1.h2, h2 + k.fc2.h2, h2 + k.out.h2, h2 + k.h2_pack, k.fc1.K, k.fc1.N, stream));
        return xp_ln_proj_h2_pack(h2 + k.in.h2, h2 + k.h2_in_pack, k.in.N, k.in.K, stream);
    });
}

extern "C" int xp_xpoint_forward(void* ctx, const float* weights, const void* wsplit, const float* images, int batch, int H, int W,
                                 void* workspace, size_t workspace_bytes, float* prob, float* desc_nhwc, float* enc_nhwc,
                                 float* logits_nhwc, void* stream) {
    return xp_xpoint_forward_ex(ctx, weights, wsplit, images, batch, H, W, workspace, workspace_bytes, prob, desc_nhwc, enc_nhwc, logits_nhwc, nullptr, stream);
}

extern "C" int xp_xpoint_forward_ex(void* ctx, const float* weights, const void* wsplit, const float* images, int batch, int H, int W,
                                    void* workspace, size_t workspace_bytes, float* prob, float* desc_nhwc, float* enc_nhwc,
                                    float* logits_nhwc, int* status, void* stream) {
    // the process-wide switches, read once: engine and products, the mixed-precision class, the per-launch override, the A/B knobs
    const bool h2 = xp_dense_engine_value() == 1 && xp_dense_products_value() == 6;    // the reduced-product classes are x3 classes
    // Mixed-precision class (xp_set_amp_mode(1)): needs the split-fp16 engine (its kernels carry the fp16 output rounding); every block
    // runs as separate launches, because the rounding points of the reference's autocast recipe sit BETWEEN the operations the fused kernels merge
    const bool amp = xp_amp_value() != 0;
    // Per-launch override (xp_set_dense_override; numbered in build_layout): a launch whose bit is set runs on the split-bf16 planes although the
    // engine is split fp16 — how the host keeps ONE out-of-range layer from moving the whole weight set to x3.  Never for the mixed-precision classes.
    const unsigned long long ovmask = (h2 && !amp) ? xp_dense_override_value() : 0ull;
    static const bool no_fused_mlp = getenv("XP_NO_FUSED_MLP") != nullptr && atoi(getenv("XP_NO_FUSED_MLP")) != 0;      // keeps the three-launch form (A/B timing, tests)
    static const int fuse_max_c = getenv("XP_FUSE_MAXC") ? atoi(getenv("XP_FUSE_MAXC")) : 1 << 30;      // A/B: blocks wider than this run unfused
    static const bool fused_x3 = getenv("XP_FUSED_X3") != nullptr && atoi(getenv("XP_FUSED_X3")) != 0;     // A/B: fused block kernels on the x3 planes under the h2 engine
    Fwd f;
    RUN(forward_prologue("xp_xpoint_forward", ctx, weights && images && workspace && enc_nhwc, batch, H, W, workspace_bytes, 1, f));
    const Ctx* c = f.c; const Shapes& sh = f.sh; const WsPlan& wp = f.wp;
    const int E = c->cfg.embed_dim;
    float* ws = (float*)workspace;
    float *X = ws + wp.X, *T1 = ws + wp.T1, *T2 = ws + wp.T2, *T3 = ws + wp.T3, *HB = ws + wp.HB, *XD = ws + wp.XD, *SS = ws + wp.SS;
    auto X3 = [&](size_t off) { return (const char*)wsplit + off; };                         // the two regions of the split-weights buffer
    auto H2 = [&](size_t off) { return (const char*)wsplit + c->split_bytes + off; };
    auto P = [&](size_t off) { return weights + off; };
    auto ov = [&](const Dense& d) { return ((ovmask >> d.id) & 1ull) != 0; };
    // dense layers: the split-bf16 kernels when the caller passed split weights, else the exact-f32 MFMA kernels
    auto gemm = [&](const float* A, const Dense& d, float* C, const float* bias, const float* scale, const float* shift,
                    const float* res, int M, int lda, int ldc, int ldres, int act) -> int {
        if (wsplit && h2 && !ov(d)) return xp_gemm_nt_h2(A, H2(d.h2), C, bias, scale, shift, res, M, d.N, d.K, lda, ldc, ldres, act, stream);
        if (wsplit) return xp_gemm_nt_x3(A, X3(d.x3), C, bias, scale, shift, res, M, d.N, d.K, lda, ldc, ldres, act, stream);
        return xp_gemm_nt(A, P(d.w), C, bias, scale, shift, res, M, d.N, d.K, lda, ldc, ldres, act, stream);
    };
    auto conv = [&](const float* x, const Dense& d, float* y, const float* bias, const float* scale, const float* shift,
                    int Hi, int Wi, int Ci, int Co, int stride, int reflect, int act) -> int {
        if (wsplit && h2 && !ov(d)) return xp_conv3x3_nhwc_h2(x, H2(d.h2), y, bias, scale, shift, batch, Hi, Wi, Ci, Co, stride, reflect, act, stream);
        if (wsplit) return xp_conv3x3_nhwc_x3(x, X3(d.x3), y, bias, scale, shift, batch, Hi, Wi, Ci, Co, stride, reflect, act, stream);
        return xp_conv3x3_nhwc(x, P(d.w), y, bias, scale, shift, batch, Hi, Wi, Ci, Co, stride, reflect, act, stream);
    };
    const float eps = 1e-5f;
    XP_CHECK_ARG(!amp || (wsplit && h2), "xp_xpoint_forward: the mixed-precision class (xp_set_amp_mode) runs on the split-fp16 engine: pass wsplit and "
                 "select xp_set_dense_engine(1) with xp_set_dense_products(6)");
    const bool fuse_mlp = wsplit != nullptr && !no_fused_mlp && !amp;

    // patch embed (VMamba.py:1405-1420)
    const Stem& st = c->stem;
    RUN(xp_stem_conv_ln_gelu(images, P(st.w), P(st.b), P(st.ln_w), P(st.ln_b), HB, batch, H, W, E / 2, eps, stream));
    RUN(conv(HB, st.pe2, T1, P(st.pe2_b), nullptr, nullptr, sh.Hs, sh.Ws, E / 2, E, 2, 0, 0));
    RUN(xp_layernorm(T1, X, P(st.pe2_ln_w), P(st.pe2_ln_b), sh.M[0], E, eps, 0, stream));

    for (int s = 0; s < c->nstages; ++s) {
        const int C = c->dims[s], R = c->ranks[s], H4 = (int)(C * c->cfg.mlp_ratio);
        const int M = (int)sh.M[s], XW = 4 * (R + 2);
        for (const Block& k : c->stages[s].blocks) {
            // x = x + SS2D(LN(x))      (VMamba.py:1222-1229, :648-664)
            const bool fused_block = fuse_mlp && C <= fuse_max_c && k.packed;
            // Stages 2 - 3 on the split-fp16 engine: the ring GEMM (csrc/gemm_ring.hip) takes its activation operand as a P32 image written by the producer
            // (LayerNorm, the SS2D out_norm, fc1's epilogue), so its K loop is DMA + matrix instructions only.  Per-layer predicates (N, K): never the batch.
            const bool ring_ok = wsplit && h2 && !amp && !fused_block;
            const bool ring_in = ring_ok && xp_gemm_nt_h2s_applies(C, C) && !ov(k.in);
            const bool ring_out = ring_ok && xp_gemm_nt_h2s_applies(C, C) && !ov(k.out) && xp_ss2d_core_p32_supported(sh.H[s], sh.W[s], C, R);
            const bool ring_mlp = ring_ok && xp_gemm_nt_h2s_applies(H4, C) && xp_gemm_nt_h2s_applies(C, H4) && !ov(k.fc1) && !ov(k.fc2);
            const bool tail_x3 = ov(k.out) || ov(k.fc1) || ov(k.fc2);      // a fused block tail is ONE launch
            if (fused_block) {      // norm + in_proj in one row-stationary launch (csrc/mlp_fused.hip, MODE 2)
                if (h2 && !fused_x3 && !ov(k.in)) RUN(xp_ln_proj_h2(X, P(k.ln1_w), P(k.ln1_b), H2(k.h2_in_pack), H2(k.in.h2), T2, M, C, C, eps, stream));
                else RUN(xp_ln_proj_x3(X, P(k.ln1_w), P(k.ln1_b), X3(k.in_pack), T2, M, C, C, eps, stream));
            } else if (ring_in) {
                RUN(xp_layernorm_p32(X, T1, P(k.ln1_w), P(k.ln1_b), M, C, eps, stream));
                RUN(xp_gemm_nt_h2s(T1, H2(k.in.h2), T2, 0, nullptr, nullptr, nullptr, nullptr, M, C, C, C, 0, 0, stream));
            } else {
                RUN(xp_layernorm(X, T1, P(k.ln1_w), P(k.ln1_b), M, C, eps, 0, stream));
                RUN(gemm(T1, k.in, T2, nullptr, nullptr, nullptr, nullptr, M, C, C, 0, 0));
            }
            RUN(xp_dwconv3x3_silu(T2, P(k.dw_w), T3, batch, sh.H[s], sh.W[s], C, stream));
            RUN(gemm(T3, k.xproj, XD, nullptr, nullptr, nullptr, nullptr, M, C, XW, 0, 0));
            RUN(xp_ss2d_core_fwd_ex(T3, XD, P(k.dt_w), P(k.dt_b), P(k.A), P(k.D), P(k.onorm_w), P(k.onorm_b),
                                    T1, ring_out ? 2 : 0, SS, wp.ss_bytes, batch, sh.H[s], sh.W[s], C, R, 1, eps, stream));
            if (amp) RUN(xp_round_f16(T1, T1, (int64_t)M * C, stream));      // forward_corev2 returns y.to(x.dtype): out_norm's f32 result as a half tensor (VMamba.py:646)
            if (fused_block) {
                // out_proj + first residual + LN + MLP + second residual in one launch; the (M, 4C) hidden activation stays in
                // registers (csrc/mlp_fused.hip)
                if (h2 && !fused_x3 && !tail_x3) RUN(xp_mlp_fused_h2(X, T1, P(k.ln2_w), P(k.ln2_b), H2(k.h2_pack), H2(k.fc1.h2), H2(k.fc2.h2),
                                                         H2(k.out.h2), P(k.fc1_b), P(k.fc2_b), M, C, H4, eps, stream));
                else RUN(xp_mlp_fused_x3(X, T1, P(k.ln2_w), P(k.ln2_b), X3(k.pack), P(k.fc1_b), P(k.fc2_b), M, C, H4, eps, stream));
                continue;
            }
            if (ring_out) RUN(xp_gemm_nt_h2s(T1, H2(k.out.h2), X, 0, nullptr, nullptr, nullptr, X, M, C, C, C, C, 0, stream));
            else RUN(gemm(T1, k.out, X, nullptr, nullptr, nullptr, X, M, C, C, C, 0));
            // x = x + fc2(GELU(fc1(LN(x))))      (VMamba.py:1230-1234, :110-128)
            if (ring_mlp) {      // the hidden activation crosses HBM as the P32 image fc2 loads by DMA (same bytes as f32)
                RUN(xp_layernorm_p32(X, T1, P(k.ln2_w), P(k.ln2_b), M, C, eps, stream));
                RUN(xp_gemm_nt_h2s(T1, H2(k.fc1.h2), HB, 2, P(k.fc1_b), nullptr, nullptr, nullptr, M, H4, C, H4, 0, 1, stream));
                RUN(xp_gemm_nt_h2s(HB, H2(k.fc2.h2), X, 0, P(k.fc2_b), nullptr, nullptr, X, M, C, H4, C, C, 0, stream));
                continue;
            }
            RUN(xp_layernorm(X, T1, P(k.ln2_w), P(k.ln2_b), M, C, eps, 0, stream));
            RUN(gemm(T1, k.fc1, HB, P(k.fc1_b), nullptr, nullptr, nullptr, M, C, H4, 0, 1));
            RUN(gemm(HB, k.fc2, X, P(k.fc2_b), nullptr, nullptr, X, M, H4, C, C, 0));
        }
        if (s < c->nstages - 1) {   // downsample v3 (VMamba.py:1432-1440)
            const Down& d = c->stages[s].ds;
            RUN(conv(X, d.w, T1, P(d.b), nullptr, nullptr, sh.H[s], sh.W[s], C, 2 * C, 2, 0, 0));
            RUN(xp_layernorm(T1, X, P(d.ln_w), P(d.ln_b), sh.M[s + 1], 2 * C, eps, 0, stream));
        }
    }
    const int L = c->nstages - 1;
    // VMamba.py:1500-1505.  Range guard: a dense-layer operand beyond the split-fp16 engine's range (|x| >= 65504) turns that layer's output rows
    // into NaN, and every dense output of the encoder reaches the residual stream (directly, or through a scan / LayerNorm that keeps NaN), so the
    // stream itself carries the evidence; its magnitude is also what the head convolution is about to split.  Checked where it is copied anyway.
    RUN(xp_depth_to_space_nhwc_st(X, enc_nhwc, batch, sh.H[L], sh.W[L], c->dims[L], 4, (wsplit && h2 && !ov(c->head.w)) ? 65504.f : INFINITY, status, stream));

    // heads (XPoint.py:112-138, :348-371): shared 3x3 trunk GEMM for both heads, then the two 1x1 convs
    const Head &hd = c->head, &det = c->det2, &dsc = c->desc2;
    const int EC = enc_channels_of(*c), HC = c->cfg.head_channels, DET = c->cfg.det_channels, DS = c->cfg.desc_size;
    const int Mc = batch * sh.Hc * sh.Wc;
    if (prob || logits_nhwc || desc_nhwc) RUN(conv(enc_nhwc, hd.w, HB, P(hd.b), P(hd.scale), P(hd.shift), sh.Hc, sh.Wc, EC, 2 * HC, 1, 1, 2));
    if (prob || logits_nhwc) {
        float* lg = logits_nhwc ? logits_nhwc : T2;
        RUN(gemm(HB, det.w, lg, P(det.b), P(det.scale), P(det.shift), nullptr, Mc, 2 * HC, DET, 0, 0));
        if (prob) RUN(xp_softmax_shuffle_st(lg, prob, batch, sh.Hc, sh.Wc, 8, DET, 0, status, stream));
    }
    if (desc_nhwc) {
        RUN(gemm(HB + HC, dsc.w, T1, P(dsc.b), P(dsc.scale), P(dsc.shift), nullptr, Mc, 2 * HC, DS, 0, 0));
        RUN(xp_l2norm_rows_st(T1, desc_nhwc, Mc, DS, 1e-12f, status, stream));
    }
    return XP_OK;
}


// ---------------------------------------------------------------------------------------------------------------------------------------------
// Fast mixed-precision class ("amp16f"): the reference's `mixed_precision: true` deployment (XPoint.py:182 autocast, half by default)
// with HALF STORAGE — every tensor between two operations lives in HBM as fp16, dense layers are one-product fp16 MFMA GEMMs fed by LDS-DMA
// (csrc/gemm_f16.hip), the scan state / softplus / exp / out_norm / softmax / normalize stay f32 exactly where the recipe keeps them
// (csms6s.py:47-67, VMamba.py:644-646, XPoint.py:349,363).  Same rounding points as the round-3 parity class (xp_set_amp_mode(1), f32 containers):
// pinned by the same fixture, tests/golden/g20.  `weights` must be the blob whose autocast-cast tensors were rounded to fp16 on the host
// (models.XPoint.pack_weights(amp=True)); w16 = their fp16 copies (xp_prepare_f16_weights).
// ---------------------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t xp_f16_weights_bytes(void* ctx) { return ctx ? ((Ctx*)ctx)->f16_bytes : 0; }

extern "C" int xp_prepare_f16_weights(void* ctx, const float* weights, void* w16, size_t w16_bytes, void* stream) {
    XP_CHECK_ARG(ctx && weights && w16, "xp_prepare_f16_weights: null pointer");
    Ctx* c = (Ctx*)ctx;
    XP_CHECK_ARG(w16_bytes >= c->f16_bytes, "xp_prepare_f16_weights: buffer too small");
    XP_CHECK_ARG(((uintptr_t)w16 & 255) == 0, "xp_prepare_f16_weights: buffer must be 256-byte aligned");
    return each_dense(*c, [&](const Dense& e) -> int {
        XP_CHECK_ARG(e.K % 8 == 0, "xp_prepare_f16_weights: %s has K = %d, not a multiple of 8", c->params[e.param].name.c_str(), e.K);
        return xp_f32_to_f16(weights + e.w, (char*)w16 + e.f16, (int64_t)e.N * e.K, stream);
    });
}

extern "C" int xp_xpoint_forward_f16(void* ctx, const float* weights, const void* w16, const float* images, int batch, int H, int W,
                                     void* workspace, size_t workspace_bytes, float* prob, float* desc_nhwc, float* enc_nhwc,
                                     float* logits_nhwc, int* status, void* stream) {
    // the A/B knobs, read once per process; this class has its own entry point and reads none of the process-wide arithmetic switches
    static const bool no_lnproj16 = getenv("XP_NO_LN_PROJ_F16") != nullptr && atoi(getenv("XP_NO_LN_PROJ_F16")) != 0;      // LayerNorm and in_proj as two launches
    static const int no_fused16 = getenv("XP_NO_FUSED_MLP_F16") ? atoi(getenv("XP_NO_FUSED_MLP_F16")) : 0;      // 1 = the two-GEMM form everywhere, 2 = fused MLP behind a separate LayerNorm launch
    Fwd f;
    RUN(forward_prologue("xp_xpoint_forward_f16", ctx, weights && w16 && images && workspace && enc_nhwc, batch, H, W, workspace_bytes, 16, f));
    const Ctx* c = f.c; const Shapes& sh = f.sh; const WsPlan& wp = f.wp;
    const int E = c->cfg.embed_dim;
    // the f32 plan's regions, used as half buffers (each holds twice the elements it needs); T3 / XD double as the f32 copies the sequential
    // deep-stage scan reads (upper halves of their regions)
    float* ws = (float*)workspace;
    typedef unsigned short h16;      // opaque fp16 storage on the host side
    h16 *X = (h16*)(ws + wp.X), *T1 = (h16*)(ws + wp.T1), *T2 = (h16*)(ws + wp.T2), *T3 = (h16*)(ws + wp.T3), *HB = (h16*)(ws + wp.HB), *XD = (h16*)(ws + wp.XD);
    float* SS = ws + wp.SS;
    auto P = [&](size_t off) { return weights + off; };
    auto WH = [&](const Dense& d) -> const void* { return (const char*)w16 + d.f16; };
    auto gemm = [&](const void* A, const Dense& d, void* C, int c_f32, const float* bias, const float* scale, const float* shift,
                    const void* res, int M, int lda, int ldc, int ldres, int act) -> int {
        return xp_gemm_nt_f16(A, WH(d), C, c_f32, bias, scale, shift, res, M, d.N, d.K, lda, ldc, ldres, act, stream);
    };
    auto conv = [&](const void* x, const Dense& d, void* y, const float* bias, const float* scale, const float* shift,
                    int Hi, int Wi, int Ci, int Co, int stride, int reflect, int act) -> int {
        return xp_conv3x3_nhwc_f16(x, WH(d), y, 0, bias, scale, shift, batch, Hi, Wi, Ci, Co, stride, reflect, act, stream);
    };
    const float eps = 1e-5f;

    // patch embed (VMamba.py:1405-1420)
    const Stem& st = c->stem;
    RUN(xp_stem_conv_ln_gelu_f16(images, P(st.w), P(st.b), P(st.ln_w), P(st.ln_b), HB, batch, H, W, E / 2, eps, stream));
    RUN(conv(HB, st.pe2, T1, P(st.pe2_b), nullptr, nullptr, sh.Hs, sh.Ws, E / 2, E, 2, 0, 0));
    RUN(xp_layernorm_f16(T1, X, P(st.pe2_ln_w), P(st.pe2_ln_b), sh.M[0], E, eps, stream));

    for (int s = 0; s < c->nstages; ++s) {
        const int C = c->dims[s], R = c->ranks[s], H4 = (int)(C * c->cfg.mlp_ratio);
        const int M = (int)sh.M[s], XW = 4 * (R + 2);
        // deep stages: the scan's sequential form reads f32 copies of u and xdbl, written beside the half tensors by their producers (upper halves of
        // the T3 / XD regions: a region holds M * C floats = twice the halves)
        const bool seq = xp_ss2d_core_f16_wants_f32_copies(sh.H[s], sh.W[s], C, R) != 0;
        float* T3f = seq ? (ws + wp.T3 + ((size_t)M * C / 2 + 63) / 64 * 64) : nullptr;
        float* XDf = seq ? (ws + wp.XD + ((size_t)M * XW / 2 + 63) / 64 * 64) : nullptr;
        // the f32 copies live in the upper part of the T3 / XD regions, behind this stage's half tensors: that needs 1.5 x the stage's tensor, which the plan
        // only guarantees for stages smaller than the one that sizes the region (stage 0 in sequential form would overrun into the next region)
        XP_CHECK_ARG(!seq || (((size_t)M * C / 2 + 63) / 64 * 64 + (size_t)M * C <= wp.HB - wp.T3 && ((size_t)M * XW / 2 + 63) / 64 * 64 + (size_t)M * XW <= wp.SS - wp.XD),
                     "xp_xpoint_forward_f16: stage %d takes the sequential scan form but its f32 copies do not fit the workspace regions", s);
        const bool fused16 = xp_mlp_fused_f16_supported(C, H4) != 0;      // stages 0 - 1 (C <= 192): the row-stationary fused launches (csrc/mlp_f16.hip)
        for (const Block& k : c->stages[s].blocks) {
            // x = x + SS2D(LN(x))      (VMamba.py:1222-1229, :648-664)
            if (!no_lnproj16 && fused16) {     // norm + in_proj in one launch
                RUN(xp_ln_proj_f16(X, P(k.ln1_w), P(k.ln1_b), eps, WH(k.in), T2, M, C, stream));
            } else {
                RUN(xp_layernorm_f16(X, T1, P(k.ln1_w), P(k.ln1_b), M, C, eps, stream));
                RUN(gemm(T1, k.in, T2, 0, nullptr, nullptr, nullptr, nullptr, M, C, C, 0, 0));
            }
            RUN(xp_dwconv3x3_silu_f16(T2, P(k.dw_w), T3, T3f, batch, sh.H[s], sh.W[s], C, stream));
            RUN(gemm(T3, k.xproj, XD, 0, nullptr, nullptr, nullptr, nullptr, M, C, XW, 0, 0));
            if (seq) RUN(gemm(T3, k.xproj, XDf, 1, nullptr, nullptr, nullptr, nullptr, M, C, XW, 0, 0));     // the same half values in f32 containers (M <= a few thousand rows)
            RUN(xp_ss2d_core_fwd_f16(T3, XD, T3f, XDf, P(k.dt_w), P(k.dt_b), P(k.A), P(k.D), P(k.onorm_w), P(k.onorm_b),
                                     T1, SS, wp.ss_bytes, batch, sh.H[s], sh.W[s], C, R, 1, eps, stream));
            RUN(gemm(T1, k.out, X, 0, nullptr, nullptr, nullptr, X, M, C, C, C, 0));
            // x = x + fc2(GELU(fc1(LN(x))))      (VMamba.py:1230-1234, :110-128)
            if (no_fused16 != 1 && fused16) {      // norm2 + fc1 + GELU + fc2 + residual in one launch, hidden activation on chip
                if (no_fused16 == 2) {
                    RUN(xp_layernorm_f16(X, T1, P(k.ln2_w), P(k.ln2_b), M, C, eps, stream));
                    RUN(xp_mlp_fused_f16(T1, X, WH(k.fc1), P(k.fc1_b), WH(k.fc2), P(k.fc2_b), M, C, H4, stream));
                } else RUN(xp_ln_mlp_fused_f16(X, P(k.ln2_w), P(k.ln2_b), eps, WH(k.fc1), P(k.fc1_b), WH(k.fc2), P(k.fc2_b), M, C, H4, stream));
                continue;
            }
            RUN(xp_layernorm_f16(X, T1, P(k.ln2_w), P(k.ln2_b), M, C, eps, stream));
            RUN(gemm(T1, k.fc1, HB, 0, P(k.fc1_b), nullptr, nullptr, nullptr, M, C, H4, 0, 1));
            RUN(gemm(HB, k.fc2, X, 0, P(k.fc2_b), nullptr, nullptr, X, M, H4, C, C, 0));
        }
        if (s < c->nstages - 1) {   // downsample v3 (VMamba.py:1432-1440)
            const Down& d = c->stages[s].ds;
            RUN(conv(X, d.w, T1, P(d.b), nullptr, nullptr, sh.H[s], sh.W[s], C, 2 * C, 2, 0, 0));
            RUN(xp_layernorm_f16(T1, X, P(d.ln_w), P(d.ln_b), sh.M[s + 1], 2 * C, eps, stream));
        }
    }
    const int L = c->nstages - 1;
    // VMamba.py:1500-1505; a half overflow anywhere upstream reaches the residual stream as inf / NaN and is reported here (XP_STATUS_ENC)
    RUN(xp_depth_to_space_nhwc_f16(X, enc_nhwc, T2, batch, sh.H[L], sh.W[L], c->dims[L], 4, status, stream));

    // heads (XPoint.py:112-138, :348-371): shared 3x3 trunk for both heads, the two 1x1 convolutions end in `.to(torch.float)` (c_f32)
    const Head &hd = c->head, &det = c->det2, &dsc = c->desc2;
    const int EC = enc_channels_of(*c), HC = c->cfg.head_channels, DET = c->cfg.det_channels, DS = c->cfg.desc_size;
    const int Mc = batch * sh.Hc * sh.Wc;
    if (prob || logits_nhwc || desc_nhwc) RUN(conv(T2, hd.w, HB, P(hd.b), P(hd.scale), P(hd.shift), sh.Hc, sh.Wc, EC, 2 * HC, 1, 1, 2));
    if (prob || logits_nhwc) {
        float* lg = logits_nhwc ? logits_nhwc : (float*)(ws + wp.T3);
        RUN(gemm(HB, det.w, lg, 1, P(det.b), P(det.scale), P(det.shift), nullptr, Mc, 2 * HC, DET, 0, 0));
        if (prob) RUN(xp_softmax_shuffle_st(lg, prob, batch, sh.Hc, sh.Wc, 8, DET, 0, status, stream));
    }
    if (desc_nhwc) {
        float* dtmp = (float*)(ws + wp.T1);
        RUN(gemm(HB + HC, dsc.w, dtmp, 1, P(dsc.b), P(dsc.scale), P(dsc.shift), nullptr, Mc, 2 * HC, DS, 0, 0));
        RUN(xp_l2norm_rows_st(dtmp, desc_nhwc, Mc, DS, 1e-12f, status, stream));
    }
    return XP_OK;
}
