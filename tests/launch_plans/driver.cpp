// Launch-plan driver (tests/test_cpu_launch_plan.py): calls one entry point of csrc/model.cpp with fake device pointers and prints what it
// launches.  Linked against libxpoint_hip.so together with a generated stub translation unit that DEFINES every launching entry point, so the
// library's calls land in the stubs (ELF symbol interposition) and no HIP call is ever made: the fake pointers are never dereferenced.
//   driver <ex|f16|prepare_split|prepare_f16> [key=value ...]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "xpoint_hip.h"

extern "C" int plan_silent = 0;      // 1: the stubs print nothing (host-cost timing)

namespace {
const uint64_t SPAN = 1ull << 40;
struct Base { const char* name; uint64_t addr; };
const Base BASES[] = {{"WEIGHTS", 1 * SPAN}, {"WSPLIT", 2 * SPAN}, {"IMAGES", 3 * SPAN}, {"WS", 4 * SPAN}, {"PROB", 5 * SPAN},
                      {"DESC", 6 * SPAN}, {"ENC", 7 * SPAN}, {"LOGITS", 8 * SPAN}, {"STATUS", 9 * SPAN}, {"STREAM", 10 * SPAN}};
template <class T> T* fake(int i) { return (T*)(uintptr_t)BASES[i].addr; }
}  // namespace

// a pointer as BASE+offset (one of a small ring of buffers, so one printf can format several)
extern "C" const char* plan_ptr(const void* p) {
    static char buf[32][48];
    static int k = 0;
    char* b = buf[k++ & 31];
    const uint64_t a = (uint64_t)(uintptr_t)p;
    if (!a) return "NULL";
    for (const Base& e : BASES)
        if (a >= e.addr && a - e.addr < SPAN) { snprintf(b, 48, "%s+%llu", e.name, (unsigned long long)(a - e.addr)); return b; }
    snprintf(b, 48, "WILD:0x%llx", (unsigned long long)a);
    return b;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: driver <ex|f16|prepare_split|prepare_f16> [key=value ...]\n"); return 2; }
    const std::string entry = argv[1];
    long embed = 96, batch = 2, H = 64, W = 96, wsplit = 1, products = 6, engine = 1, amp = 0, outs = 15, ws_delta = 0, reps = 0;
    int depths[4] = {2, 2, 2, 2};
    std::vector<unsigned long long> masks;
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
        const std::string k(argv[i], eq - argv[i]); const char* v = eq + 1;
        if (k == "embed") embed = atol(v); else if (k == "batch") batch = atol(v); else if (k == "H") H = atol(v); else if (k == "W") W = atol(v);
        else if (k == "wsplit") wsplit = atol(v); else if (k == "products") products = atol(v); else if (k == "engine") engine = atol(v);
        else if (k == "amp") amp = atol(v); else if (k == "outs") outs = atol(v); else if (k == "ws_delta") ws_delta = atol(v);
        else if (k == "reps") reps = atol(v);
        else if (k == "depths") sscanf(v, "%d,%d,%d,%d", &depths[0], &depths[1], &depths[2], &depths[3]);
        else if (k == "masks") { for (const char* p = v; *p;) { char* e; masks.push_back(strtoull(p, &e, 16)); p = *e ? e + 1 : e; } }
        else { fprintf(stderr, "unknown key %s\n", k.c_str()); return 2; }
    }
    xp_model_cfg cfg{};
    cfg.embed_dim = (int)embed; cfg.n_stages = 4; memcpy(cfg.depths, depths, sizeof depths); cfg.d_state = 1; cfg.dt_rank = 0; cfg.mlp_ratio = 4.f;
    cfg.head_channels = 256; cfg.desc_size = 256; cfg.det_channels = 65;
    void* ctx = nullptr;
    if (xp_ctx_create(&cfg, &ctx) != 0) { printf("xp_ctx_create failed: %s\n", xp_last_error()); return 1; }
    printf("xp_weights_numel %zu\n", xp_weights_numel(ctx));
    const int np = xp_param_count(ctx);
    printf("xp_param_count %d\n", np);
    for (int i = 0; i < np; ++i) {
        char name[128]; size_t off = 0, num = 0;
        xp_param_info(ctx, i, name, 128, &off, &num);
        printf("xp_param_info %d %s %zu %zu\n", i, name, off, num);
    }
    const size_t ws_bytes = xp_forward_workspace_bytes(ctx, (int)batch, (int)H, (int)W);
    printf("xp_forward_workspace_bytes %zu\n", ws_bytes);
    printf("xp_split_weights_bytes %zu\n", xp_split_weights_bytes(ctx));
    printf("xp_f16_weights_bytes %zu\n", xp_f16_weights_bytes(ctx));
    xp_set_dense_products((int)products); xp_set_dense_engine((int)engine); xp_set_amp_mode((int)amp);

    const float* weights = fake<const float>(0);
    void* wsp = wsplit ? fake<void>(1) : nullptr;
    float* prob = (outs & 1) ? fake<float>(4) : nullptr;
    float* desc = (outs & 2) ? fake<float>(5) : nullptr;
    float* enc = (outs & 4) ? fake<float>(6) : nullptr;
    float* logits = (outs & 8) ? fake<float>(7) : nullptr;
    void* stream = fake<void>(9);
    auto call = [&]() -> int {
        if (entry == "ex") return xp_xpoint_forward_ex(ctx, weights, wsp, fake<const float>(2), (int)batch, (int)H, (int)W, fake<void>(3), ws_bytes + ws_delta,
                                                       prob, desc, enc, logits, fake<int>(8), stream);
        if (entry == "f16") return xp_xpoint_forward_f16(ctx, weights, wsp, fake<const float>(2), (int)batch, (int)H, (int)W, fake<void>(3), ws_bytes + ws_delta,
                                                         prob, desc, enc, logits, fake<int>(8), stream);
        if (entry == "prepare_split") return xp_prepare_split_weights(ctx, weights, wsp, xp_split_weights_bytes(ctx), stream);
        if (entry == "prepare_f16") return xp_prepare_f16_weights(ctx, weights, wsp, xp_f16_weights_bytes(ctx), stream);
        fprintf(stderr, "unknown entry %s\n", entry.c_str());
        exit(2);
    };
    if (reps > 0) {      // host cost of one enqueue: stubs silent
        plan_silent = 1;
        const auto t0 = std::chrono::steady_clock::now();
        int rc = 0;
        for (long i = 0; i < reps; ++i) rc |= call();
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        printf("reps %ld rc %d us_per_call %.3f\n", reps, rc, us / reps);
        return rc != 0;
    }
    if (masks.empty()) masks.push_back(0);
    for (size_t i = 0; i < masks.size(); ++i) {
        if (masks.size() > 1 || masks[0]) printf("== override %llx\n", masks[i]);
        xp_set_dense_override(masks[i]);
        const int rc = call();
        printf("rc %d\nxp_last_error %s\n", rc, xp_last_error());
    }
    xp_ctx_destroy(ctx);
    return 0;
}
