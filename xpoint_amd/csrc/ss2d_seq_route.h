// A wave's walk along its route in the dt_rank >= 16 sequential kernels — the ONE text of it, included INSIDE the bodies of ss2d_seq_scan2 and
// ss2d_seq_scan3 (ss2d_seq.hip; no include guard on purpose).  A struct with these members compiled to other registers and more instructions in every
// instance (profiles/ss2d_split_resources.txt); the same text in both bodies compiles to the code each had when it carried its own copy.
// Expects in scope: p, ys, lane-derived fr / fh, pair, back, L, XD, RW, NP, NPL, c, d, b and XP_SEQ_ROUTE_SX(buf), the wave's LDS tile buffer `buf`.
// Defines: ru, ry, cbyte (the buffer resources of the image's u plane and the route's y plane), ucur / unext, xreg, tile_offsets, load_tile, store_x.
    const int plane_bytes = L * p.C * 4;                                // host: < 2^31
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)(p.u + (int64_t)b * L * p.C), 0, plane_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(ys + ((int64_t)d * p.Bn + b) * L * p.C), 0, plane_bytes, 0x00020000);
    const int cbyte = c * 4;
    const char* xb = reinterpret_cast<const char*>(p.xdbl + (int64_t)b * L * XD + pair * 2 * RW + back * RW) + fh * (NPL * 8);
    const float invH = 1.f / (float)p.H;
    // tile t, pixel (lane & 31) of the route's sequence: byte offset of its row in a (L, C) plane (out of range past the end) and of its xdbl row
    auto tile_offsets = [&](int t, int& off_uy, int& off_x) {
        const int i = t * SEQ_TP + fr;
        const int ic = min(i, L - 1);
        const int l = back ? L - 1 - ic : ic;                           // backward routes walk the flipped sequence (csm_triton.py:33-36)
        int px = l;
        if (pair == 1) {                                                // column-major routes: l = w * H + h
            const int ww = (int)(((float)l + 0.5f) * invH);             // exact: (l + 0.5) / H is at least 0.5 / H away from an integer
            px = (l - ww * p.H) * p.W + ww;
        }
        off_uy = i < L ? px * (p.C * 4) : 0x7fffffff;
        off_x = px * (XD * 4);
    };
    float ucur[SEQ_TP], unext[SEQ_TP];
    float2 xreg[NPL];
    auto load_tile = [&](int off_uy, int off_x, float (&uv)[SEQ_TP]) {
#pragma unroll
        for (int j = 0; j < SEQ_TP; ++j)
            uv[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ru, cbyte, __builtin_amdgcn_readlane(off_uy, j), 0));
        const char* xr = xb + off_x;
#pragma unroll
        for (int e = 0; e < NPL; ++e) {
            // the upper half-wave fetches pieces NPL .. NP-1; when NP is odd its last slot repeats piece NP-1 (same data, same LDS address)
            const int pe = (e == NPL - 1 && 2 * NPL > NP) ? (fh ? e - 1 : e) : e;
            xreg[e] = *reinterpret_cast<const float2*>(xr + pe * 8);
        }
    };
    const int xdst = fr * RW + fh * (NPL * 2);
    auto store_x = [&](int buf) {
#pragma unroll
        for (int e = 0; e < NPL; ++e) {
            const int pe = (e == NPL - 1 && 2 * NPL > NP) ? (fh ? e - 1 : e) : e;
            *reinterpret_cast<float2*>(&XP_SEQ_ROUTE_SX(buf)[xdst + pe * 2]) = xreg[e];
        }
    };
