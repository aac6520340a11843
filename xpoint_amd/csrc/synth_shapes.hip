// SyntheticShapes on the device (include/xpoint_hip.h, xp_synth_*; DESIGN.md "Synthetic shapes"; reference xpoint/utils/draw_primitives.py
// and xpoint/datasets/SyntheticShapes.py).  The host (xpoint_amd/synthetic_shapes.py) draws every random scalar and emits one draw list per
// image; every pixel is touched here.  No launch count depends on the batch size, nothing is accumulated with float atomics, and image b reads
// only tables of image b: an image is the same alone and inside any batch, and two calls agree bit for bit.
//
//   xp_synth_background       the Philox uniform field against the threshold, then the blobs: "last covering circle wins" with the integer
//                             test dx^2 + dy^2 <= r^2.  A blob's colour is CONTRAST(raw, min_contrast) against the mean of the thresholded field,
//                             which is an integer count: one counting launch, then the painting launch.
//   xp_synth_box_blur         cv2.blur: normalised box, BORDER_REFLECT_101, per-sample kernel size (even sizes: anchor k / 2).  Rows: an f64
//                             prefix sum of the row in LDS (a coalesced load, then per-thread chunks), a window is a difference of two prefixes (the reflected extension is periodic and
//                             even, so any kernel size folds onto the one prefix).  Columns: one lane per column, an f64 running sum that is
//                             restarted from a direct sum every SY_VSEG rows.  f64 keeps both at ~1e-13, far under the f32 store.
//   xp_synth_resolve_colours  f64 partial sums of the blurred background in a fixed order, then one thread per image walks the colour rules.
//   xp_synth_rasterise        one thread per pixel, the image's records in LDS, bounding box first, the last covering record wins.  Integer
//                             inside tests (64-bit); the ellipse alone is f64, evaluated as written (-ffp-contract=off).
//   xp_synth_texture          draw_multiple_polygons' textures, one job per textured record, three launches for any batch: T_j on the job's texture
//                             box (the blobs come out of Philox per 32 x 32 tile, culled, kept in index order), then the box blur's two passes
//                             restricted to what the record's box needs.  The host lays the jobs out in one arena and gives every launch a table
//                             of running workgroup counts; a workgroup finds its job by bisection.
//   xp_synth_rasterise_textured  the rasteriser with the TEXTURED kind: such a polygon's pixels are read from its job's blurred box.
//   xp_synth_resize           cv2.resize INTER_LINEAR: source coordinate (d + 0.5) scale - 0.5, clamped taps, f32 weights.
//   xp_synth_scatter_points   the keypoint map from the host's integer points: the constant byte 1, collisions are benign.
#include "cv_geom.h"
#include "philox.h"
#include "../../include/xpoint_hip.h"

namespace {

constexpr int SY_PART = XP_SYNTH_PARTIALS;     // blocks per image of the counting / summing launches
constexpr int SY_MAX_BLOBS = 256;
constexpr int SY_MAX_REC = XP_SYNTH_MAX_RECORDS;
constexpr int SY_REC = XP_SYNTH_RECORD_INTS;
constexpr int SY_MAX_W = 4096;                  // the row prefix lives in LDS as f64
constexpr int SY_VSEG = 64;                     // rows per restart of the column pass

__device__ __forceinline__ bool sy_field_bit(uint64_t seed, int id, int p, float thr) {
    return aug_uniform(aug_philox(seed, (uint32_t)id, XP_SYNTH_KEY_BACKGROUND, (uint32_t)p).x) > thr;          // cv2.threshold THRESH_BINARY
}

// sum of v over the 256 lanes in a fixed order (LDS tree); thread 0 holds the result
template <typename T>
__device__ __forceinline__ T sy_block_sum(T v, T* s_red) {
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if ((int)threadIdx.x < n) s_red[threadIdx.x] = s_red[threadIdx.x] + s_red[threadIdx.x + n];
        __syncthreads();
    }
    return s_red[0];
}

// get_random_color: raw where it contrasts with the background, (raw + 0.5) % 1 where it does not
__device__ __forceinline__ double sy_contrast(double raw, double mean, double mc) { return fabs(raw - mean) < mc ? fmod(raw + 0.5, 1.0) : raw; }

// grid (SY_PART, B): block k counts the set pixels p = k * 256 + t, + SY_PART * 256, ...
__global__ __launch_bounds__(256) void synth_count_kernel(uint64_t seed, const int* __restrict__ ids, const float* __restrict__ thr, int npix,
                                                          int* __restrict__ counts) {
    __shared__ int s_red[256];
    const int b = blockIdx.y, id = ids[b];
    const float t = thr[b];
    int acc = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (int64_t)SY_PART * 256) acc += sy_field_bit(seed, id, (int)p, t) ? 1 : 0;
    const int total = sy_block_sum(acc, s_red);
    if (threadIdx.x == 0) counts[(size_t)b * SY_PART + blockIdx.x] = total;
}

// blobs: geom (B, NB, 4) int32 = cx, cy, r, 0; raw (B, NB) f64
__global__ __launch_bounds__(256) void synth_paint_kernel(float* __restrict__ frame, uint64_t seed, const int* __restrict__ ids,
                                                          const float* __restrict__ thr, const int* __restrict__ counts,
                                                          const int* __restrict__ geom, const double* __restrict__ raw, int NB, double mc,
                                                          double* __restrict__ field_mean, int H, int W) {
    __shared__ int s_red[256];
    __shared__ int s_g[SY_MAX_BLOBS][4];
    __shared__ float s_col[SY_MAX_BLOBS];
    const int b = blockIdx.z;
    const int total = sy_block_sum((int)threadIdx.x < SY_PART ? counts[(size_t)b * SY_PART + threadIdx.x] : 0, s_red);
    const double mean = (double)total / (double)((int64_t)H * W);
    if ((int)threadIdx.x < NB) {
        const int* g = geom + ((size_t)b * NB + threadIdx.x) * 4;
        s_g[threadIdx.x][0] = g[0]; s_g[threadIdx.x][1] = g[1]; s_g[threadIdx.x][2] = g[2];
        s_col[threadIdx.x] = (float)sy_contrast(raw[(size_t)b * NB + threadIdx.x], mean, mc);
    }
    if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) field_mean[b] = mean;
    __syncthreads();
    const int x = xp_tile_x(), y = xp_tile_y();
    if (x >= W || y >= H) return;
    float v = sy_field_bit(seed, ids[b], y * W + x, thr[b]) ? 1.f : 0.f;
    for (int k = NB - 1; k >= 0; --k) {
        const int64_t dx = x - s_g[k][0], dy = y - s_g[k][1], r = s_g[k][2];
        if (dx * dx + dy * dy <= r * r) { v = s_col[k]; break; }
    }
    frame[((size_t)b * H + y) * W + x] = v;
}

// sum of the reflected extension E(i) = row[reflect101(i)] over i = 0 .. n (n >= 0), from the inclusive prefix P of the row
__device__ __forceinline__ double sy_ext_prefix(const double* __restrict__ P, int W, int n) {
    const int period = 2 * (W - 1);
    const int q = n / period, r = n - q * period;
    const double part = r < W ? P[r] : P[W - 1] + (P[W - 2] - P[period - r - 1]);
    if (q == 0) return part;
    const double sp = P[W - 1] + (P[W - 2] - P[0]);          // one period: row[0 .. W-1] then row[W-2 .. 1]
    return (double)q * sp + part;
}

// the row s_p[0 .. W) in LDS becomes its inclusive f64 prefix, in a fixed order: per-thread chunks, then the 256 chunk totals in ascending order.
// Every thread of the block calls it after the barrier that follows the load; it ends on a barrier.
__device__ __forceinline__ void sy_row_prefix(double* __restrict__ s_p, double* __restrict__ s_part, int W) {
    const int t = threadIdx.x, C = (W + 255) / 256, i0 = t * C, i1 = min(i0 + C, W);
    double acc = 0.0;
    for (int i = i0; i < i1; ++i) { acc = acc + s_p[i]; s_p[i] = acc; }
    s_part[t] = acc;
    __syncthreads();
    if (t == 0) {
        double run = 0.0;
        for (int k = 0; k < 256; ++k) { const double c = s_part[k]; s_part[k] = run; run = run + c; }
    }
    __syncthreads();
    const double base = s_part[t];
    for (int i = i0; i < i1; ++i) s_p[i] = base + s_p[i];
    __syncthreads();
}

// the sum of the row's reflected extension over the window [x - a, x - a + ks - 1], from the row's prefix
__device__ __forceinline__ double sy_row_window(const double* __restrict__ s_p, int W, int x, int a, int ks) {
    if (W == 1) return (double)ks * s_p[0];
    const int lo = x - a, hi = x - a + ks - 1;
    double sum = sy_ext_prefix(s_p, W, hi);
    if (lo > 0) sum = sum - sy_ext_prefix(s_p, W, lo - 1);
    else if (lo < 0) sum = sum + (sy_ext_prefix(s_p, W, -lo) - s_p[0]);          // E is even about 0
    return sum;
}

// one lane's column windows of the rows y0 .. y1 - 1: an f64 running sum started from a direct sum.  load(i): the column at frame row i in [0, H)
template <typename Load, typename Store>
__device__ __forceinline__ void sy_col_windows(Load load, Store store, int y0, int y1, int ks, int H) {
    const int a = ks / 2;
    const double inv = (double)ks;
    double run = 0.0;
    for (int i = y0 - a; i <= y0 - a + ks - 1; ++i) run = run + (double)load(xp_cv_reflect101(i, H));
    store(y0, (float)(run / inv));
    for (int y = y0 + 1; y < y1; ++y) {
        run = run + (double)load(xp_cv_reflect101(y - a + ks - 1, H));
        run = run - (double)load(xp_cv_reflect101(y - 1 - a, H));
        store(y, (float)(run / inv));
    }
}

// grid (H, B): one block per row
__global__ __launch_bounds__(256) void synth_box_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ ksizes,
                                                             int H, int W) {
    __shared__ double s_p[SY_MAX_W];
    __shared__ double s_part[256];
    const int b = blockIdx.y, y = blockIdx.x, t = threadIdx.x;
    const float* s = src + ((size_t)b * H + y) * W;
    float* d = dst + ((size_t)b * H + y) * W;
    const int ks = max(ksizes[b], 1), a = ks / 2;
    for (int i = t; i < W; i += 256) s_p[i] = (double)s[i];          // consecutive lanes on consecutive pixels
    __syncthreads();
    sy_row_prefix(s_p, s_part, W);
    const double inv = (double)ks;
    for (int x = t; x < W; x += 256) d[x] = (float)(sy_row_window(s_p, W, x, a, ks) / inv);
}

// grid (ceil(W / 64), ceil(H / (4 SY_VSEG)), B): lane = column, the block's 4 waves take 4 consecutive row segments
__global__ __launch_bounds__(256) void synth_box_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ ksizes,
                                                             int H, int W) {
    const int b = blockIdx.z, x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * SY_VSEG, y1 = min(y0 + SY_VSEG, H);
    if (x >= W || y0 >= H) return;
    const float* s = src + (size_t)b * H * W + x;
    float* d = dst + (size_t)b * H * W + x;
    sy_col_windows([&](int i) { return s[(size_t)i * W]; }, [&](int y, float v) { d[(size_t)y * W] = v; }, y0, y1, max(ksizes[b], 1), H);
}

// grid (SY_PART, B): f64 partial sums in a fixed order
__global__ __launch_bounds__(256) void synth_partial_sum_kernel(const float* __restrict__ img, int npix, double* __restrict__ partials) {
    __shared__ double s_red[256];
    const int b = blockIdx.y;
    double acc = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (int64_t)SY_PART * 256) acc = acc + (double)img[(size_t)b * npix + p];
    const double total = sy_block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[(size_t)b * SY_PART + blockIdx.x] = total;
}

// grid (B): rules (B, R, 4) int32 = kind, ref0, ref1, candidate offset; vals (B, R, 2) f64 = value, min_contrast or delta; cands (B, NC) f64
__global__ __launch_bounds__(256) void synth_resolve_kernel(const double* __restrict__ partials, const int* __restrict__ rules,
                                                            const double* __restrict__ vals, const double* __restrict__ cands, int R, int NC,
                                                            int npix, float* __restrict__ colours, double* __restrict__ bg_mean) {
    __shared__ double s_red[256];
    __shared__ double s_c[SY_MAX_REC];
    const int b = blockIdx.x;
    const double total = sy_block_sum((int)threadIdx.x < SY_PART ? partials[(size_t)b * SY_PART + threadIdx.x] : 0.0, s_red);
    if (threadIdx.x != 0) return;
    const double mean = total / (double)npix;
    bg_mean[b] = mean;
    for (int r = 0; r < R; ++r) {
        const int* q = rules + ((size_t)b * R + r) * 4;
        const double v = vals[((size_t)b * R + r) * 2], m = vals[((size_t)b * R + r) * 2 + 1];
        const int kind = q[0], r0 = q[1], r1 = q[2], off = q[3];
        const bool h0 = r0 >= 0 && r0 < r, h1 = r1 >= 0 && r1 < r;
        double c = v;
        if (kind == XP_SYNTH_RULE_CONTRAST) {
            c = sy_contrast(v, mean, m);
        } else if (kind == XP_SYNTH_RULE_DIFFERENT && off >= 0 && off + XP_SYNTH_CANDIDATES <= NC) {
            const double* cd = cands + (size_t)b * NC + off;
            const double n0 = h0 ? s_c[r0] : 0.0, n1 = h1 ? s_c[r1] : 0.0;
            c = cd[XP_SYNTH_CANDIDATES - 1];
            for (int k = 0; k < XP_SYNTH_CANDIDATES - 1; ++k) {
                const double t = cd[k];
                if (!((h0 && fabs(n0 - t) < m) || (h1 && fabs(n1 - t) < m))) { c = t; break; }
            }
        } else if (kind == XP_SYNTH_RULE_REL && h0) {
            c = fmod(s_c[r0] + m, 1.0);
        }
        s_c[r] = c;
        colours[(size_t)b * R + r] = (float)c;
    }
}

__device__ __forceinline__ bool sy_in_segment(int64_t px, int64_t py, const int* g, int64_t t) {
    const int64_t ax = g[0], ay = g[1], dx = g[2] - ax, dy = g[3] - ay, ux = px - ax, uy = py - ay;
    const int64_t len2 = dx * dx + dy * dy, proj = ux * dx + uy * dy, t2 = t * t;
    if (len2 == 0 || proj < 0) return 4 * (ux * ux + uy * uy) <= t2;
    if (proj > len2) { const int64_t vx = px - g[2], vy = py - g[3]; return 4 * (vx * vx + vy * vy) <= t2; }
    const int64_t cr = dx * uy - dy * ux;
    return (uint64_t)(cr * cr) <= (uint64_t)(t2 * len2) / 4;          // 4 cross^2 <= t^2 len^2, without the overflow of the left side
}

__device__ __forceinline__ bool sy_in_polygon(int64_t px, int64_t py, const int* g, int n) {
    bool odd = false;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        const int64_t ax = g[2 * i], ay = g[2 * i + 1], bx = g[2 * j], by = g[2 * j + 1];
        const int64_t t = (bx - ax) * (py - ay) - (px - ax) * (by - ay);
        if (t == 0 && px >= min(ax, bx) && px <= max(ax, bx) && py >= min(ay, by) && py <= max(ay, by)) return true;      // on the edge
        if ((ay <= py) != (by <= py) && ((by > ay) ? t > 0 : t < 0)) odd = !odd;                                         // half-open crossing to the right
    }
    return odd;
}

__device__ __forceinline__ bool sy_in_ellipse(int px, int py, const int* g) {
    const double co = *reinterpret_cast<const double*>(g + 4), si = *reinterpret_cast<const double*>(g + 6);
    const double dx = (double)(px - g[0]), dy = (double)(py - g[1]);
    const double ax = fmax((double)g[2], 0.5), ay = fmax((double)g[3], 0.5);
    const double u = (dx * co + dy * si) / ax, w = (dy * co - dx * si) / ay;
    return u * u + w * w <= 1.0;
}

// records (B, R, SY_REC) int32: kind, bbox x0 y0 x1 y1 (inclusive), n (radius / thickness / vertex count), 16 geometry words, 2 spare
// TEX: the list may hold XP_SYNTH_TEXTURED records, polygons whose pixels come from the blurred box of their job (arena + tex_off[b][r], rows of
// the bbox's width) instead of a colour; without TEX the two tables are not read.
template <bool TEX>
__global__ __launch_bounds__(256) void synth_raster_kernel(float* __restrict__ frame, const int* __restrict__ records, const float* __restrict__ colours,
                                                           uint64_t seed, const int* __restrict__ ids, const float* __restrict__ arena,
                                                           const long long* __restrict__ tex_off, int R, int H, int W) {
    __shared__ __attribute__((aligned(8))) int s_rec[SY_MAX_REC * SY_REC];
    __shared__ float s_col[SY_MAX_REC];
    const int b = blockIdx.z;
    for (int i = threadIdx.x; i < R * SY_REC; i += 256) s_rec[i] = records[(size_t)b * R * SY_REC + i];
    for (int i = threadIdx.x; i < R; i += 256) s_col[i] = colours[(size_t)b * R + i];
    __syncthreads();
    const int x = xp_tile_x(), y = xp_tile_y();
    if (x >= W || y >= H) return;
    for (int r = R - 1; r >= 0; --r) {
        const int* q = s_rec + r * SY_REC;
        const int kind = q[0];
        if (kind == XP_SYNTH_NOP) continue;
        if (kind == XP_SYNTH_NOISE) {
            frame[((size_t)b * H + y) * W + x] = aug_uniform(aug_philox(seed, (uint32_t)ids[b], XP_SYNTH_KEY_NOISE, (uint32_t)(y * W + x)).x);
            return;
        }
        if (x < q[1] || y < q[2] || x > q[3] || y > q[4]) continue;
        const int* g = q + 6;
        bool in = false;
        if (kind == XP_SYNTH_CIRCLE) {
            const int64_t dx = x - g[0], dy = y - g[1], rr = q[5];
            in = dx * dx + dy * dy <= rr * rr;
        } else if (kind == XP_SYNTH_SEGMENT) {
            in = sy_in_segment(x, y, g, q[5]);
        } else if (kind == XP_SYNTH_POLYGON || (TEX && kind == XP_SYNTH_TEXTURED)) {
            in = sy_in_polygon(x, y, g, min(max(q[5], 0), 8));
        } else if (kind == XP_SYNTH_ELLIPSE) {
            in = sy_in_ellipse(x, y, g);
        }
        if (TEX && in && kind == XP_SYNTH_TEXTURED) {
            const long long off = tex_off[(size_t)b * R + r];
            if (off < 0) continue;          // a record without a job draws nothing
            frame[((size_t)b * H + y) * W + x] = arena[off + (long long)(y - q[2]) * (q[3] - q[1] + 1) + (x - q[1])];
            return;
        }
        if (in) { frame[((size_t)b * H + y) * W + x] = s_col[r]; return; }
    }
}

// ---------------------------------------------------------------------------------------------------------------- textured polygons
constexpr int SY_TEX_BLOBS = XP_SYNTH_MAX_TEXTURE_BLOBS;
constexpr int SY_TEX_TILE = 32;                 // the texture launch culls the blobs once per 32 x 32 tile
constexpr int SY_JOB = XP_SYNTH_JOB_INTS;

// one textured record's work item: see xp_synth_texture in include/xpoint_hip.h
struct SyJob {
    int b, r, j, ks, x0, y0, x1, y1, tx0, ty0, tx1, ty1, unit;      // unit: this workgroup's index among the job's
    long long off_tex, off_rows, off_out;
    bool ok;
    __device__ __forceinline__ int bw() const { return x1 - x0 + 1; }
    __device__ __forceinline__ int bh() const { return y1 - y0 + 1; }
    __device__ __forceinline__ int tw() const { return tx1 - tx0 + 1; }
    __device__ __forceinline__ int th() const { return ty1 - ty0 + 1; }
};

// the job of workgroup `wg` of one launch: units (n_jobs + 1) is that launch's running count of workgroups, so the job is the last one that
// starts at or before wg.  ok = every extent lies inside the frame and the arena; a workgroup of a job that is not ok does nothing.
__device__ __forceinline__ SyJob sy_job_of(const int* __restrict__ jobs, const long long* __restrict__ offsets, const int* __restrict__ units,
                                           int n_jobs, int wg, long long arena_floats, int B, int R, int H, int W) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (units[mid] <= wg) lo = mid; else hi = mid - 1;
    }
    const int* q = jobs + (size_t)lo * SY_JOB;
    SyJob j;
    j.b = q[0]; j.r = q[1]; j.j = q[2]; j.ks = min(max(q[3], 1), XP_SYNTH_MAX_KSIZE);
    j.x0 = q[4]; j.y0 = q[5]; j.x1 = q[6]; j.y1 = q[7]; j.tx0 = q[8]; j.ty0 = q[9]; j.tx1 = q[10]; j.ty1 = q[11];
    j.unit = wg - units[lo];
    j.off_tex = offsets[(size_t)lo * 3]; j.off_rows = offsets[(size_t)lo * 3 + 1]; j.off_out = offsets[(size_t)lo * 3 + 2];
    j.ok = j.b >= 0 && j.b < B && j.r >= 0 && j.r < R && j.j >= 0 && j.j < SY_MAX_REC && j.unit >= 0 &&
           0 <= j.tx0 && j.tx0 <= j.x0 && j.x0 <= j.x1 && j.x1 <= j.tx1 && j.tx1 < W &&
           0 <= j.ty0 && j.ty0 <= j.y0 && j.y0 <= j.y1 && j.y1 <= j.ty1 && j.ty1 < H &&
           j.off_tex >= 0 && j.off_tex + (long long)j.tw() * j.th() <= arena_floats &&
           j.off_rows >= 0 && j.off_rows + (long long)j.bw() * j.th() <= arena_floats &&
           j.off_out >= 0 && j.off_out + (long long)j.bw() * j.bh() <= arena_floats;
    return j;
}

__device__ __forceinline__ float sy_tex_uniform(uint64_t seed, int id, int j, int NB, int i, int c) {
    return aug_uniform(aug_philox(seed, (uint32_t)id, XP_SYNTH_KEY_TEXTURE, (uint32_t)((j * NB + i) * 4 + c)).x);
}

// grid (tiles of every job): T_j over one 32 x 32 tile of the job's texture box.  The blobs come out of Philox here: thread t decodes the blobs
// t C .. t C + C - 1 (C = ceil(NB / 256)), keeps those whose disc reaches the tile, and an ordered compaction (a scan of the 256 counts) leaves
// the survivors in index order, so "the highest index wins" is the first hit of a walk from the list's end.  The list holds all NB blobs: on a
// small frame every blob reaches every tile.  Only the winner's colour is drawn.  A blob is packed as cx | cy << 12 | r << 24 (cx, cy < 4096, r < 20).
__global__ __launch_bounds__(256) void synth_texture_kernel(float* __restrict__ arena, long long arena_floats, const int* __restrict__ jobs,
                                                            const long long* __restrict__ offsets, const int* __restrict__ units, int n_jobs,
                                                            const float* __restrict__ colours, int R, uint64_t seed, const int* __restrict__ ids,
                                                            int NB, double mc, int B, int H, int W) {
    __shared__ uint32_t s_raw[SY_TEX_BLOBS];
    __shared__ uint32_t s_list[SY_TEX_BLOBS];
    __shared__ uint16_t s_idx[SY_TEX_BLOBS];
    __shared__ int s_cnt[257];
    const SyJob jb = sy_job_of(jobs, offsets, units, n_jobs, blockIdx.x, arena_floats, B, R, H, W);
    if (!jb.ok) return;
    const int t = threadIdx.x, tw = jb.tw(), tiles_x = (tw + SY_TEX_TILE - 1) / SY_TEX_TILE;
    const int ox = jb.tx0 + (jb.unit % tiles_x) * SY_TEX_TILE, oy = jb.ty0 + (jb.unit / tiles_x) * SY_TEX_TILE;
    if (oy > jb.ty1) return;
    const int ex = min(ox + SY_TEX_TILE - 1, jb.tx1), ey = min(oy + SY_TEX_TILE - 1, jb.ty1);
    const int id = ids[jb.b];
    const int C = (NB + 255) / 256, i0 = t * C, i1 = min(i0 + C, NB);
    int cnt = 0;
    for (int i = i0; i < i1; ++i) {
        const int cx = (int)floor((double)sy_tex_uniform(seed, id, jb.j, NB, i, 0) * (double)W);
        const int cy = (int)floor((double)sy_tex_uniform(seed, id, jb.j, NB, i, 1) * (double)H);
        const int rr = (int)floor((double)sy_tex_uniform(seed, id, jb.j, NB, i, 2) * 20.0);
        const int dx = max(max(ox - cx, cx - ex), 0), dy = max(max(oy - cy, cy - ey), 0);          // to the nearest pixel of the tile
        const bool keep = dx * dx + dy * dy <= rr * rr;
        s_raw[i] = keep ? ((uint32_t)cx | ((uint32_t)cy << 12) | ((uint32_t)rr << 24)) : 0xFFFFFFFFu;
        cnt += keep ? 1 : 0;
    }
    s_cnt[t] = cnt;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < 256; ++k) { const int c = s_cnt[k]; s_cnt[k] = run; run += c; }
        s_cnt[256] = run;
    }
    __syncthreads();
    int pos = s_cnt[t];
    for (int i = i0; i < i1; ++i) {
        const uint32_t g = s_raw[i];
        if (g != 0xFFFFFFFFu) { s_list[pos] = g; s_idx[pos] = (uint16_t)i; ++pos; }
    }
    __syncthreads();
    const int n = s_cnt[256];
    const float base = colours[(size_t)jb.b * R + jb.r];
    const int px = ox + (t & 31);
    if (px > ex) return;
    for (int py = oy + (t >> 5); py <= ey; py += 8) {
        int win = -1;
        for (int m = n - 1; m >= 0; --m) {
            const uint32_t g = s_list[m];
            const int dx = px - (int)(g & 0xFFFu), dy = py - (int)((g >> 12) & 0xFFFu), rr = (int)(g >> 24);
            if (dx * dx + dy * dy <= rr * rr) { win = s_idx[m]; break; }
        }
        const float v = win < 0 ? base : (float)sy_contrast((double)sy_tex_uniform(seed, id, jb.j, NB, win, 3), 0.0, mc);
        arena[jb.off_tex + (long long)(py - jb.ty0) * tw + (px - jb.tx0)] = v;
    }
}

// grid (rows of every job's texture box): the row windows of the columns x0 .. x1.  The row is laid over the frame's width, zero outside the
// texture box (no window of the record's box reaches there), so the prefix and the reflection are those of the whole-frame blur.
__global__ __launch_bounds__(256) void synth_texture_rows_kernel(float* __restrict__ arena, long long arena_floats, const int* __restrict__ jobs,
                                                                 const long long* __restrict__ offsets, const int* __restrict__ units, int n_jobs,
                                                                 int B, int R, int H, int W) {
    __shared__ double s_p[SY_MAX_W];
    __shared__ double s_part[256];
    const SyJob jb = sy_job_of(jobs, offsets, units, n_jobs, blockIdx.x, arena_floats, B, R, H, W);
    if (!jb.ok || jb.unit >= jb.th()) return;
    const int t = threadIdx.x, tw = jb.tw(), bw = jb.bw();
    const float* s = arena + jb.off_tex + (long long)jb.unit * tw;
    float* d = arena + jb.off_rows + (long long)jb.unit * bw;
    for (int i = t; i < W; i += 256) s_p[i] = (i >= jb.tx0 && i <= jb.tx1) ? (double)s[i - jb.tx0] : 0.0;
    __syncthreads();
    sy_row_prefix(s_p, s_part, W);
    const double inv = (double)jb.ks;
    for (int x = jb.x0 + t; x <= jb.x1; x += 256) d[x - jb.x0] = (float)(sy_row_window(s_p, W, x, jb.ks / 2, jb.ks) / inv);
}

// grid (64-column x 4 SY_VSEG-row blocks of every job's box): lane = column, the block's 4 waves take 4 consecutive row segments
__global__ __launch_bounds__(256) void synth_texture_cols_kernel(float* __restrict__ arena, long long arena_floats, const int* __restrict__ jobs,
                                                                 const long long* __restrict__ offsets, const int* __restrict__ units, int n_jobs,
                                                                 int B, int R, int H, int W) {
    const SyJob jb = sy_job_of(jobs, offsets, units, n_jobs, blockIdx.x, arena_floats, B, R, H, W);
    if (!jb.ok) return;
    const int bw = jb.bw(), blocks_x = (bw + 63) / 64;
    const int x = (jb.unit % blocks_x) * 64 + (threadIdx.x & 63);                                  // relative to x0
    const int y0 = jb.y0 + ((jb.unit / blocks_x) * 4 + (threadIdx.x >> 6)) * SY_VSEG, y1 = min(y0 + SY_VSEG, jb.y1 + 1);
    if (x >= bw || y0 > jb.y1) return;
    const float* s = arena + jb.off_rows + x;
    float* d = arena + jb.off_out + x;
    sy_col_windows([&](int i) { return s[(long long)(min(max(i, jb.ty0), jb.ty1) - jb.ty0) * bw]; },
                   [&](int y, float v) { d[(long long)(y - jb.y0) * bw] = v; }, y0, y1, jb.ks, H);
}

__device__ __forceinline__ void sy_resize_tap(int d, double scale, int n, int& i0, int& i1, float& w) {
    const double f = ((double)d + 0.5) * scale - 0.5;
    const double fl = floor(f);
    int i = (int)fl;
    w = (float)(f - fl);
    if (i < 0) { i = 0; w = 0.f; }
    if (i >= n - 1) { i = n - 1; w = 0.f; }
    i0 = i;
    i1 = min(i + 1, n - 1);
}

__global__ __launch_bounds__(256) void synth_resize_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int h, int w) {
    const int b = blockIdx.z, x = xp_tile_x(), y = xp_tile_y();
    if (x >= w || y >= h) return;
    int x0, x1, y0, y1;
    float wx, wy;
    sy_resize_tap(x, (double)W / (double)w, W, x0, x1, wx);
    sy_resize_tap(y, (double)H / (double)h, H, y0, y1, wy);
    const float* s = src + (size_t)b * H * W;
    const float top = s[(size_t)y0 * W + x0] * (1.f - wx) + s[(size_t)y0 * W + x1] * wx;
    const float bot = s[(size_t)y1 * W + x0] * (1.f - wx) + s[(size_t)y1 * W + x1] * wx;
    dst[((size_t)b * h + y) * w + x] = top * (1.f - wy) + bot * wy;
}

// grid (ceil(cap / 256), B): points (B, cap, 2) int32 (y, x)
__global__ __launch_bounds__(256) void synth_scatter_kernel(const int* __restrict__ points, const int* __restrict__ counts, int cap,
                                                            uint8_t* __restrict__ map, int h, int w) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(counts[b], cap)) return;
    const int y = points[((size_t)b * cap + i) * 2], x = points[((size_t)b * cap + i) * 2 + 1];
    if (y >= 0 && y < h && x >= 0 && x < w) map[((size_t)b * h + y) * w + x] = 1;
}

#define SY_NOT_NULL(p) XP_CHECK_ARG((p) != nullptr, "%s: null pointer: %s", fn, #p)

#define SY_ALIGNED8(p) XP_CHECK_ARG(((uintptr_t)(p) & 7) == 0, "%s: misaligned pointer (8 bytes): %s", fn, #p)

int sy_check_frame(const char* fn, int B, int H, int W, const char* h_name = "H", const char* w_name = "W") {
    XP_CHECK_ARG(B >= 1 && B <= 65535, "%s: B must be in [1, 65535] (got %d)", fn, B);
    XP_CHECK_ARG(H >= 1 && H <= SY_MAX_W, "%s: %s must be in [1, %d] (got %d)", fn, h_name, SY_MAX_W, H);
    XP_CHECK_ARG(W >= 1 && W <= SY_MAX_W, "%s: %s must be in [1, %d] (got %d)", fn, w_name, SY_MAX_W, W);
    return XP_OK;
}

}  // namespace

extern "C" int xp_synth_background(float* frame, unsigned long long seed, const int* sample_ids, const float* thresholds, const int* blob_geom,
                                   const double* blob_raw, int n_blobs, double min_contrast, int* count_ws, double* field_mean, int B, int H, int W,
                                   void* stream) {
    const char* fn = "xp_synth_background";
    if (int rc = sy_check_frame(fn, B, H, W)) return rc;
    XP_CHECK_ARG(n_blobs >= 0 && n_blobs <= SY_MAX_BLOBS, "%s: n_blobs must be in [0, %d] (got %d)", fn, SY_MAX_BLOBS, n_blobs);
    XP_CHECK_ARG(min_contrast >= 0.0 && min_contrast <= 1.0, "%s: min_contrast must be in [0, 1] (got %g)", fn, min_contrast);
    SY_NOT_NULL(frame); SY_NOT_NULL(sample_ids); SY_NOT_NULL(thresholds); SY_NOT_NULL(count_ws); SY_NOT_NULL(field_mean);
    if (n_blobs > 0) { SY_NOT_NULL(blob_geom); SY_NOT_NULL(blob_raw); }
    SY_ALIGNED8(blob_raw); SY_ALIGNED8(field_mean);
    XpProfScope prof("synth_background", (hipStream_t)stream, 0.0, 4.0 * B * H * W);
    hipLaunchKernelGGL(synth_count_kernel, dim3(SY_PART, B), dim3(256), 0, (hipStream_t)stream, (uint64_t)seed, sample_ids, thresholds, H * W, count_ws);
    hipLaunchKernelGGL(synth_paint_kernel, xp_tile_grid(W, H, B), dim3(256), 0, (hipStream_t)stream, frame, (uint64_t)seed, sample_ids, thresholds,
                       (const int*)count_ws, blob_geom, blob_raw, n_blobs, min_contrast, field_mean, H, W);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_synth_box_blur(const float* src, float* tmp, float* dst, const int* ksizes, int B, int H, int W, void* stream) {
    const char* fn = "xp_synth_box_blur";
    if (int rc = sy_check_frame(fn, B, H, W)) return rc;
    SY_NOT_NULL(src); SY_NOT_NULL(tmp); SY_NOT_NULL(dst); SY_NOT_NULL(ksizes);
    XP_CHECK_ARG(tmp != src && tmp != dst, "%s: tmp must be a buffer of its own", fn);
    XpProfScope prof("synth_box_blur", (hipStream_t)stream, 0.0, 16.0 * B * H * W);
    hipLaunchKernelGGL(synth_box_rows_kernel, dim3(H, B), dim3(256), 0, (hipStream_t)stream, src, tmp, ksizes, H, W);
    hipLaunchKernelGGL(synth_box_cols_kernel, dim3(xp_cdiv(W, 64), xp_cdiv(H, 4 * SY_VSEG), B), dim3(256), 0, (hipStream_t)stream, (const float*)tmp, dst,
                       ksizes, H, W);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_synth_resolve_colours(const float* background, const int* rules, const double* rule_values, const double* candidates, int n_records,
                                        int n_candidates, double* partial_ws, float* colours, double* bg_mean, int B, int H, int W, void* stream) {
    const char* fn = "xp_synth_resolve_colours";
    if (int rc = sy_check_frame(fn, B, H, W)) return rc;
    XP_CHECK_ARG(n_records >= 1 && n_records <= SY_MAX_REC, "%s: n_records must be in [1, %d] (got %d)", fn, SY_MAX_REC, n_records);
    XP_CHECK_ARG(n_candidates >= 0, "%s: n_candidates must not be negative (got %d)", fn, n_candidates);
    SY_NOT_NULL(background); SY_NOT_NULL(rules); SY_NOT_NULL(rule_values); SY_NOT_NULL(partial_ws); SY_NOT_NULL(colours); SY_NOT_NULL(bg_mean);
    if (n_candidates > 0) SY_NOT_NULL(candidates);
    SY_ALIGNED8(rule_values); SY_ALIGNED8(candidates); SY_ALIGNED8(partial_ws); SY_ALIGNED8(bg_mean);
    XpProfScope prof("synth_resolve_colours", (hipStream_t)stream, 0.0, 4.0 * B * H * W);
    hipLaunchKernelGGL(synth_partial_sum_kernel, dim3(SY_PART, B), dim3(256), 0, (hipStream_t)stream, background, H * W, partial_ws);
    hipLaunchKernelGGL(synth_resolve_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const double*)partial_ws, rules, rule_values, candidates,
                       n_records, n_candidates, H * W, colours, bg_mean);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_synth_rasterise(float* frame, const int* records, const float* colours, unsigned long long seed, const int* sample_ids, int n_records,
                                  int B, int H, int W, void* stream) {
    const char* fn = "xp_synth_rasterise";
    if (int rc = sy_check_frame(fn, B, H, W)) return rc;
    XP_CHECK_ARG(n_records >= 1 && n_records <= SY_MAX_REC, "%s: n_records must be in [1, %d] (got %d)", fn, SY_MAX_REC, n_records);
    SY_NOT_NULL(frame); SY_NOT_NULL(records); SY_NOT_NULL(colours); SY_NOT_NULL(sample_ids);
    SY_ALIGNED8(records);
    XpProfScope prof("synth_rasterise", (hipStream_t)stream, 0.0, 8.0 * B * H * W);
    hipLaunchKernelGGL(synth_raster_kernel<false>, xp_tile_grid(W, H, B), dim3(256), 0, (hipStream_t)stream, frame, records, colours, (uint64_t)seed,
                       sample_ids, (const float*)nullptr, (const long long*)nullptr, n_records, H, W);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_synth_texture(float* arena, long long arena_floats, const int* jobs, const long long* offsets, const int* units, int n_jobs,
                                const float* colours, int n_records, unsigned long long seed, const int* sample_ids, int nb_blobs, double min_contrast,
                                int min_ksize, int max_ksize, int n_tiles, int n_rows, int n_col_blocks, int B, int H, int W, void* stream) {
    const char* fn = "xp_synth_texture";
    if (int rc = sy_check_frame(fn, B, H, W)) return rc;
    XP_CHECK_ARG(n_jobs >= 1 && n_jobs <= B * SY_MAX_REC, "%s: n_jobs must be in [1, B * %d] (got %d)", fn, SY_MAX_REC, n_jobs);
    XP_CHECK_ARG(n_records >= 1 && n_records <= SY_MAX_REC, "%s: n_records must be in [1, %d] (got %d)", fn, SY_MAX_REC, n_records);
    XP_CHECK_ARG(nb_blobs >= 0 && nb_blobs <= SY_TEX_BLOBS, "%s: nb_blobs must be in [0, %d] (got %d)", fn, SY_TEX_BLOBS, nb_blobs);
    XP_CHECK_ARG(min_contrast >= 0.0 && min_contrast <= 1.0, "%s: min_contrast must be in [0, 1] (got %g)", fn, min_contrast);
    XP_CHECK_ARG(min_ksize >= 1 && min_ksize <= max_ksize && max_ksize <= XP_SYNTH_MAX_KSIZE, "%s: ksize must be in [1, %d] (got %d .. %d)", fn,
                 XP_SYNTH_MAX_KSIZE, min_ksize, max_ksize);
    XP_CHECK_ARG(arena_floats >= 1, "%s: arena_floats must be positive (got %lld)", fn, arena_floats);
    SY_NOT_NULL(arena); SY_NOT_NULL(jobs); SY_NOT_NULL(offsets); SY_NOT_NULL(units); SY_NOT_NULL(colours); SY_NOT_NULL(sample_ids);
    SY_ALIGNED8(offsets);
    XP_CHECK_ARG(n_tiles >= n_jobs && n_rows >= n_jobs && n_col_blocks >= n_jobs, "%s: n_tiles, n_rows and n_col_blocks count at least one "
                 "workgroup per job (got %d, %d, %d for %d jobs)", fn, n_tiles, n_rows, n_col_blocks, n_jobs);
    const hipStream_t s = (hipStream_t)stream;
    // algorithmic bytes: the texture, the row pass and the blurred boxes are each written once and read once
    XpProfScope prof("synth_texture", s, 0.0, 8.0 * (double)arena_floats);
    hipLaunchKernelGGL(synth_texture_kernel, dim3(n_tiles), dim3(256), 0, s, arena, arena_floats, jobs, offsets, units, n_jobs, colours, n_records,
                       (uint64_t)seed, sample_ids, nb_blobs, min_contrast, B, H, W);
    hipLaunchKernelGGL(synth_texture_rows_kernel, dim3(n_rows), dim3(256), 0, s, arena, arena_floats, jobs, offsets, units + (n_jobs + 1), n_jobs,
                       B, n_records, H, W);
    hipLaunchKernelGGL(synth_texture_cols_kernel, dim3(n_col_blocks), dim3(256), 0, s, arena, arena_floats, jobs, offsets, units + 2 * (n_jobs + 1),
                       n_jobs, B, n_records, H, W);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_synth_rasterise_textured(float* frame, const int* records, const float* colours, unsigned long long seed, const int* sample_ids,
                                           const float* arena, const long long* tex_offsets, int n_records, int B, int H, int W, void* stream) {
    const char* fn = "xp_synth_rasterise_textured";
    if (int rc = sy_check_frame(fn, B, H, W)) return rc;
    XP_CHECK_ARG(n_records >= 1 && n_records <= SY_MAX_REC, "%s: n_records must be in [1, %d] (got %d)", fn, SY_MAX_REC, n_records);
    SY_NOT_NULL(frame); SY_NOT_NULL(records); SY_NOT_NULL(colours); SY_NOT_NULL(sample_ids); SY_NOT_NULL(arena); SY_NOT_NULL(tex_offsets);
    SY_ALIGNED8(records); SY_ALIGNED8(tex_offsets);
    XpProfScope prof("synth_rasterise_textured", (hipStream_t)stream, 0.0, 12.0 * B * H * W);
    hipLaunchKernelGGL(synth_raster_kernel<true>, xp_tile_grid(W, H, B), dim3(256), 0, (hipStream_t)stream, frame, records, colours, (uint64_t)seed,
                       sample_ids, arena, tex_offsets, n_records, H, W);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_synth_resize(const float* src, float* dst, int B, int H, int W, int h, int w, void* stream) {
    const char* fn = "xp_synth_resize";
    if (int rc = sy_check_frame(fn, B, H, W)) return rc;
    XP_CHECK_ARG(h >= 1 && h <= SY_MAX_W, "%s: h must be in [1, %d] (got %d)", fn, SY_MAX_W, h);
    XP_CHECK_ARG(w >= 1 && w <= SY_MAX_W, "%s: w must be in [1, %d] (got %d)", fn, SY_MAX_W, w);
    SY_NOT_NULL(src); SY_NOT_NULL(dst);
    XP_CHECK_ARG(src != dst, "%s: in-place resize is not supported", fn);
    XpProfScope prof("synth_resize", (hipStream_t)stream, 0.0, 4.0 * B * ((double)H * W + (double)h * w));
    hipLaunchKernelGGL(synth_resize_kernel, xp_tile_grid(w, h, B), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, h, w);
    XP_LAUNCH_CHECK();
    return XP_OK;
}

extern "C" int xp_synth_scatter_points(const int* points, const int* counts, int cap, uint8_t* map, int B, int h, int w, void* stream) {
    const char* fn = "xp_synth_scatter_points";
    if (int rc = sy_check_frame(fn, B, h, w, "h", "w")) return rc;
    XP_CHECK_ARG(cap >= 1, "%s: cap must be positive (got %d)", fn, cap);
    SY_NOT_NULL(points); SY_NOT_NULL(counts); SY_NOT_NULL(map);
    XpProfScope prof("synth_scatter_points", (hipStream_t)stream, 0.0, (double)B * ((double)h * w + 8.0 * cap));
    XP_HIP(hipMemsetAsync(map, 0, (size_t)B * h * w, (hipStream_t)stream));
    hipLaunchKernelGGL(synth_scatter_kernel, dim3(xp_cdiv(cap, 256), B), dim3(256), 0, (hipStream_t)stream, points, counts, cap, map, h, w);
    XP_LAUNCH_CHECK();
    return XP_OK;
}
