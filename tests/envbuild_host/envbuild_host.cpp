// envbuild_host.cpp — TEST INFRASTRUCTURE.  The bodies of take_amd/csrc/tk_envmap.h built for the host and run in the
// loop structure of its kernels' launches — blocks of ROWS rows striding over the image, tiles of COLS columns, the load,
// scan and store phases of a tile each over all of a block's threads, one "lane" per table entry afterwards — so that
// tests/test_envbuild_cpu.py can hold what take_hip_scene_set_envmap builds on the device to what scene creation builds
// on the host (env_tables and guide_table of tk_host_scene.h), byte for byte, without a GPU.  With -DENVBUILD_MAIN a
// stand-alone program that runs the same comparison on seeded maps of the test's sizes (the sanitizer build of the
// Makefile).  Never loaded by the product.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "tk_envmap.h"
#include "tk_host_scene.h"

namespace {
using namespace tk;

// k_env_weigh_scan as `grid` blocks of BLOCK threads run it; tex_f / tex_d may be null
template <class T> void weigh_scan(const T *in, int w, int h, int grid, float *tex_f, double *tex_d, std::vector<double> &prefix, std::vector<double> &row_sum) {
    const double PI_D = 3.14159265358979323846;
    std::vector<double> wy((size_t)h);
    for (int y = 0; y < h; y++) wy[y] = std::sin(PI_D * (y + 0.5) / h);
    prefix.assign((size_t)w * h, std::numeric_limits<double>::quiet_NaN());
    row_sum.assign((size_t)h, std::numeric_limits<double>::quiet_NaN());
    std::vector<double> tile((size_t)em::ROWS * em::TILE_LD);
    for (int block = 0; block < grid; block++)
        for (int64_t yb = (int64_t)block * em::ROWS; yb < h; yb += (int64_t)grid * em::ROWS) {
            const int y0 = (int)yb;
            double run[em::ROWS] = {};
            for (int64_t x0 = 0; x0 < w; x0 += em::COLS) {
                std::fill(tile.begin(), tile.end(), std::numeric_limits<double>::quiet_NaN());  // (what a phase must not read)
                for (int tid = 0; tid < em::BLOCK; tid++)
                    for (int e = tid; e < em::ROWS * em::COLS; e += em::BLOCK) em::tile_load(in, w, h, y0, x0, e, wy.data(), tile.data(), tex_f, tex_d);
                for (int tid = 0; tid < em::ROWS && y0 + tid < h; tid++)
                    run[tid] = em::tile_scan(tile.data() + tid * em::TILE_LD, (int)(w - x0 < em::COLS ? w - x0 : em::COLS), run[tid]);
                for (int tid = 0; tid < em::BLOCK; tid++)
                    for (int e = tid; e < em::ROWS * em::COLS; e += em::BLOCK) em::tile_store(tile.data(), w, h, y0, x0, e, prefix.data());
            }
            for (int tid = 0; tid < em::ROWS && y0 + tid < h; tid++) row_sum[y0 + tid] = run[tid];
        }
}

// the tables of one side from the shared doubles: k_env_conditional and k_env_guides, one entry at a time
template <class R> void side_tables(const std::vector<double> &prefix, const std::vector<double> &row_sum, const std::vector<double> &marg, int w, int h, int gm, int gc,
                                    R *marginal, R *conditional, int32_t *guide_m, int32_t *guide_c) {
    for (int y = 0; y <= h; y++) marginal[y] = R(marg[y]);
    for (int y = 0; y < h; y++)
        for (int64_t x = 0; x <= w; x++)
            conditional[(int64_t)y * ((int64_t)w + 1) + x] = R(em::cond_entry(x < w ? prefix[(int64_t)y * w + x] : 0.0, row_sum[y], (int)x, w));
    for (int k = 0; k <= gm; k++) guide_m[k] = em::guide_entry((const R *)marginal, h, gm, k);
    for (int row = 0; row < h; row++)
        for (int k = 0; k <= gc; k++) guide_c[(int64_t)row * ((int64_t)gc + 1) + k] = em::guide_entry((const R *)conditional + (int64_t)row * ((int64_t)w + 1), w, gc, k);
}

// -> 0, 1 = refused (no positive luminance)
template <class T, class R>
int device_build(const T *in, int w, int h, int grid, int gm, int gc, R *marginal, R *conditional, int32_t *guide_m, int32_t *guide_c, float *tex_f, double *tex_d) {
    std::vector<double> prefix, row_sum, marg((size_t)h + 1);
    weigh_scan(in, w, h, grid, tex_f, tex_d, prefix, row_sum);
    if (!em::marginal_cdf(row_sum.data(), h, marg.data())) return 1;
    side_tables(prefix, row_sum, marg, w, h, gm, gc, marginal, conditional, guide_m, guide_c);
    return 0;
}
// what scene creation makes of a double image: env_tables, rounded to R, guide_table
template <class R> int host_build(const double *rgb, int w, int h, int gm, int gc, R *marginal, R *conditional, int32_t *guide_m, int32_t *guide_c) {
    std::vector<double> marg, cond;
    if (!env_tables(rgb, w, h, marg, cond)) return 1;
    for (size_t i = 0; i < marg.size(); i++) marginal[i] = R(marg[i]);
    for (size_t i = 0; i < cond.size(); i++) conditional[i] = R(cond[i]);
    guide_table((const R *)marginal, h, gm, guide_m);
    for (int y = 0; y < h; y++) guide_table((const R *)conditional + (size_t)y * (w + 1), w, gc, guide_c + (size_t)y * (gc + 1));
    return 0;
}
int default_grid(int h) { return (int)std::min<int64_t>(((int64_t)h + em::ROWS - 1) / em::ROWS, 1 << 20); }
}  // namespace

extern "C" {
// the sizes of the guide tables of a w x h map (creation's rule, TAKE_HIP_ENV_GUIDE included)
void envbuild_guide_sizes(int w, int h, int32_t *gm, int32_t *gc) {
    int a, b;
    tk::env_guide_sizes(w, h, a, b);
    *gm = a, *gc = b;
}
// in_real / side_real: 0 float, 1 double.  grid <= 0: the launch's own grid.  marginal h + 1, conditional h * (w + 1)
// Reals of the side; guide_m gm + 1, guide_c h * (gc + 1); tex_f / tex_d: 3 * w * h converted texels, either may be null.
// -> 0, 1 = refused (no positive luminance), -1 bad argument
int envbuild_device(int32_t in_real, const void *img, int w, int h, int grid, int32_t side_real, int gm, int gc, void *marginal, void *conditional, int32_t *guide_m,
                    int32_t *guide_c, float *tex_f, double *tex_d) {
    if (!img || w <= 0 || h <= 0 || gm <= 0 || gc <= 0 || !marginal || !conditional || !guide_m || !guide_c) return -1;
    if (grid <= 0) grid = default_grid(h);
    if (in_real)
        return side_real ? device_build((const double *)img, w, h, grid, gm, gc, (double *)marginal, (double *)conditional, guide_m, guide_c, tex_f, tex_d)
                         : device_build((const double *)img, w, h, grid, gm, gc, (float *)marginal, (float *)conditional, guide_m, guide_c, tex_f, tex_d);
    return side_real ? device_build((const float *)img, w, h, grid, gm, gc, (double *)marginal, (double *)conditional, guide_m, guide_c, tex_f, tex_d)
                     : device_build((const float *)img, w, h, grid, gm, gc, (float *)marginal, (float *)conditional, guide_m, guide_c, tex_f, tex_d);
}
// the same tables as scene creation makes them from a double image
int envbuild_host(const double *img, int w, int h, int32_t side_real, int gm, int gc, void *marginal, void *conditional, int32_t *guide_m, int32_t *guide_c) {
    if (!img || w <= 0 || h <= 0 || gm <= 0 || gc <= 0 || !marginal || !conditional || !guide_m || !guide_c) return -1;
    return side_real ? host_build(img, w, h, gm, gc, (double *)marginal, (double *)conditional, guide_m, guide_c)
                     : host_build(img, w, h, gm, gc, (float *)marginal, (float *)conditional, guide_m, guide_c);
}
}

#ifdef ENVBUILD_MAIN
namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
double draw() {  // (xorshift64*: any fixed sequence will do)
    g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}
// random positive, a fifth of the texels zero, one all-black row
std::vector<double> random_map(int w, int h) {
    std::vector<double> m((size_t)3 * w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const bool black = (draw() < 0.2 && x + y > 0) || (h > 1 && y == h / 2);  // (texel (0, 0) of a one-row map stays lit)
            for (int c = 0; c < 3; c++) m[3 * ((size_t)y * w + x) + c] = black ? 0.0 : 0.05 + 1.95 * draw();
        }
    return m;
}
template <class R> bool same(const std::vector<R> &a, const std::vector<R> &b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(R)) == 0; }
// -> the number of mismatches (0 or 1); want_refused: both builds must refuse
int compare(const std::vector<double> &img, int w, int h, bool want_refused, int grid) {
    int32_t gm, gc;
    envbuild_guide_sizes(w, h, &gm, &gc);
    int bad = 0;
    for (int side = 0; side < 2; side++) {
        const size_t rb = side ? 8 : 4;
        std::vector<char> m[2], c[2];
        std::vector<int32_t> a[2], b[2];
        for (int k = 0; k < 2; k++) m[k].assign(((size_t)h + 1) * rb, 0), c[k].assign((size_t)h * (w + 1) * rb, 0), a[k].assign((size_t)gm + 1, -1), b[k].assign((size_t)h * (gc + 1), -1);
        std::vector<float> tf((size_t)3 * w * h);
        std::vector<double> td((size_t)3 * w * h);
        const int r0 = envbuild_device(1, img.data(), w, h, grid, side, gm, gc, m[0].data(), c[0].data(), a[0].data(), b[0].data(), tf.data(), td.data());
        const int r1 = envbuild_host(img.data(), w, h, side, gm, gc, m[1].data(), c[1].data(), a[1].data(), b[1].data());
        bool ok = r0 == r1 && r0 == (want_refused ? 1 : 0);
        if (ok && !want_refused) ok = same(m[0], m[1]) && same(c[0], c[1]) && same(a[0], a[1]) && same(b[0], b[1]) && std::memcmp(td.data(), img.data(), td.size() * 8) == 0;
        for (size_t i = 0; ok && !want_refused && i < tf.size(); i++) ok = tf[i] == (float)img[i];
        if (!ok) std::printf("MISMATCH %d x %d, f%d, grid %d (device %d, host %d)\n", w, h, side ? 64 : 32, grid, r0, r1), bad = 1;
    }
    return bad;
}
}  // namespace

int main() {
    int bad = 0, cases = 0;
    const int widths[] = {1, 63, 64, 65, 129}, heights[] = {1, 2, 63, 64, 65};
    for (int w : widths)
        for (int h : heights) bad += compare(random_map(w, h), w, h, false, 0), cases++;
    bad += compare(random_map(130, 67), 130, 67, false, 0), cases++;
    bad += compare(random_map(130, 67), 130, 67, false, 2), cases++;  // (blocks that stride over the rows)
    bad += compare(random_map(9000, 2), 9000, 2, false, 0), cases++;
    bad += compare(random_map(2, 16500), 2, 16500, false, 0), cases++;
    std::vector<double> black((size_t)3 * 65 * 17, 0.0);
    bad += compare(black, 65, 17, true, 0), cases++;
    black[3 * 70 + 1] = std::numeric_limits<double>::quiet_NaN();  // (its luminance is NaN, which counts as 0: the total stays 0)
    bad += compare(black, 65, 17, true, 0), cases++;
    std::printf("envbuild_host: %d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
