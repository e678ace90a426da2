// tk_envmap.h — the sampling tables of an environment map (EnvMap, tk_scene.h) built on the device: what
// take_hip_scene_set_envmap* replace in a resident scene (include/take_hip.h; specification: DESIGN.md §4o).  The bodies
// below are TK_HD and written once: the kernels at the end of this file run them on the device, tk_host_scene.h's
// env_tables and guide_table run the same text on the host (scene creation), tests/envbuild_host runs them in the
// kernels' loop structure.  Launched from tk_envmap.hip.
//
// Arithmetic: every + - * / is one operation in the order written (-ffp-contract=off), all of it in double whatever
// the scene's precision; a side's tables are the doubles rounded to its Real once.  The running sum of a row is the
// serial sum from its left end — floating-point addition does not re-associate — so the rows are what runs in
// parallel, one lane per row; the row weights sin(theta) come from the host (a device sin may differ in the last place).
#pragma once
#include <stdint.h>

#include "tk_common.h"

namespace tk {
namespace em {

// what texel (r, g, b) of a row of weight wy = sin(theta of the row's centre) adds to its row's sum: luminance, negatives
// (and NaN) counting as 0
TK_HD double texel_weight(double r, double g, double b, double wy) {
    const double lum = 0.2126 * r + 0.7152 * g + 0.0722 * b;
    return (lum > 0 ? lum : 0.0) * wy;
}

// entry x (0 .. w) of a row's conditional CDF from the sum `prefix` left of x and the row's sum `run`: a row whose sum
// is not > 0 is sampled uniformly
TK_HD double cond_entry(double prefix, double run, int x, int w) { return x == w ? 1.0 : (run > 0 ? prefix / run : (double)x / w); }

// the marginal CDF (h + 1 entries) from the h row sums: h serial adds in row order; false (marg unspecified) when the
// total is not > 0 — an all-black map, or a NaN total
TK_HD bool marginal_cdf(const double *row_sum, int h, double *marg) {
    double total = 0;
    for (int y = 0; y < h; y++) {
        marg[y] = total;
        total += row_sum[y];
    }
    if (!(total > 0)) return false;
    for (int y = 0; y < h; y++) marg[y] /= total;
    marg[h] = 1.0;
    return true;
}

// entry k (0 .. g) of the guide table over an R-typed CDF of n intervals: the interval that holds k / g (exact: g is a
// power of two)
template <class R> TK_HD int32_t guide_entry(const R *cdf, int n, int g, int k) {
    const R xi = R(k) / R(g);
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= xi) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- the row scan.  A block takes ROWS rows and walks them in tiles of COLS columns: every thread loads texels of the
// tile — consecutive lanes consecutive texels of a row —, converts them for the resident sides and puts their weights
// into tile[row][column]; then lane r of the first wave adds row r's run of the tile in order, leaving in place of each
// weight the sum left of it; then every thread stores prefixes, again along the rows.  TILE_LD: one double of padding,
// lane r's walk then starts on bank 2 r (+ 2 per column): no two of the 16 lanes on one bank.
constexpr int ROWS = 16, COLS = 64, TILE_LD = COLS + 1, BLOCK = 256;

// element e (0 .. ROWS * COLS) of the tile at (y0, x0) of a w x h image of T texels: the load phase
template <class T> TK_HD void tile_load(const T *in, int w, int h, int y0, int64_t x0, int e, const double *wy, double *tile, float *tex_f, double *tex_d) {
    const int r = e / COLS, c = e - r * COLS;
    const int y = y0 + r;
    const int64_t x = x0 + c;
    if (y >= h || x >= w) return;
    const int64_t p = 3 * ((int64_t)y * w + x);
    const double t0 = (double)in[p], t1 = (double)in[p + 1], t2 = (double)in[p + 2];
    if (tex_f) tex_f[p] = (float)t0, tex_f[p + 1] = (float)t1, tex_f[p + 2] = (float)t2;
    if (tex_d) tex_d[p] = t0, tex_d[p + 1] = t1, tex_d[p + 2] = t2;
    tile[r * TILE_LD + c] = texel_weight(t0, t1, t2, wy[y]);
}
// one row's nc columns of the tile: weights in, the sums left of them out -> the running sum behind the tile
TK_HD double tile_scan(double *row, int nc, double run) {
    for (int c = 0; c < nc; c++) {
        const double v = row[c];
        row[c] = run;
        run += v;
    }
    return run;
}
// element e of the tile -> prefix[y * w + x]: the store phase
TK_HD void tile_store(const double *tile, int w, int h, int y0, int64_t x0, int e, double *prefix) {
    const int r = e / COLS, c = e - r * COLS;
    const int y = y0 + r;
    const int64_t x = x0 + c;
    if (y < h && x < w) prefix[(int64_t)y * w + x] = tile[r * TILE_LD + c];
}

#if defined(__HIPCC__)
constexpr int MAX_GRID_Y = 32768;

// Convert, weigh and scan: tex_f / tex_d = the image as float / double texels (either may be null), prefix[y][x] = the
// sum of row y's weights left of x, row_sum[y] = the row's sum; wy: h row weights.
template <class T>
__global__ __launch_bounds__(BLOCK) void k_env_weigh_scan(const T *in, int w, int h, const double *wy, float *tex_f, double *tex_d, double *prefix, double *row_sum) {
    __shared__ double tile[ROWS * TILE_LD];
    const int tid = threadIdx.x;
    for (int64_t yb = (int64_t)blockIdx.x * ROWS; yb < h; yb += (int64_t)gridDim.x * ROWS) {
        const int y0 = (int)yb;
        const bool scans = tid < ROWS && y0 + tid < h;
        double run = 0;
        for (int64_t x0 = 0; x0 < w; x0 += COLS) {
            for (int e = tid; e < ROWS * COLS; e += BLOCK) tile_load(in, w, h, y0, x0, e, wy, tile, tex_f, tex_d);
            __syncthreads();
            if (scans) run = tile_scan(tile + tid * TILE_LD, (int)(w - x0 < COLS ? w - x0 : COLS), run);
            __syncthreads();
            for (int e = tid; e < ROWS * COLS; e += BLOCK) tile_store(tile, w, h, y0, x0, e, prefix);
            __syncthreads();  // (before the next tile is loaded over this one)
        }
        if (scans) row_sum[y0 + tid] = run;
    }
}

// cond[y][x] (w + 1 entries per row) = R(cond_entry): one entry per lane, a wave along a row
template <class R> __global__ __launch_bounds__(BLOCK) void k_env_conditional(const double *prefix, const double *row_sum, int w, int h, R *cond) {
    const int64_t x = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x > w) return;
    for (int y = blockIdx.y; y < h; y += gridDim.y)
        cond[(int64_t)y * ((int64_t)w + 1) + x] = R(cond_entry(x < w ? prefix[(int64_t)y * w + x] : 0.0, row_sum[y], (int)x, w));
}

// out[row][k] (g + 1 entries per row) = guide_entry over row `row` of cdf (n + 1 entries per row): one entry per lane
template <class R> __global__ __launch_bounds__(BLOCK) void k_env_guides(const R *cdf, int rows, int n, int g, int32_t *out) {
    const int k = (int)blockIdx.x * BLOCK + threadIdx.x;
    if (k > g) return;
    for (int row = blockIdx.y; row < rows; row += gridDim.y) out[(int64_t)row * ((int64_t)g + 1) + k] = guide_entry(cdf + (int64_t)row * ((int64_t)n + 1), n, g, k);
}
#endif  // __HIPCC__

}  // namespace em
}  // namespace tk
