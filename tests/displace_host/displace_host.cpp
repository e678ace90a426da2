// displace_host.cpp — TEST INFRASTRUCTURE.  take_amd/csrc/tk_displace.h built for the host: its creation-time check,
// rows of faces and lookup coordinates as they are, and its body — with tk_subdiv.h's two normal bodies in front of and
// behind it — run in the loop structure of the launches: blocks of BLOCK threads, one vertex or face per thread, the
// blocks striding when the grid is smaller than the work, the tail block partly idle, a guard element behind every
// output array that must stay untouched — so that tests/test_displace_cpu.py can hold what take_hip_displace_apply
// computes to tests/displace_ref.py bit for bit without a GPU, and tests/test_gpu_displace.py the device's output to
// this.  With -DDISPLACE_HOST_MAIN a stand-alone program that runs the bodies over meshes and images it makes itself and
// checks bounds and a few exact properties (the sanitizer build of the Makefile).  Never loaded by the product.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tk_displace.h"
#include "tk_subdiv.h"

namespace {
using namespace tk;
static_assert(displace::BLOCK == subdiv::BLOCK && displace::MAX_BLOCKS == subdiv::MAX_BLOCKS, "one launch shape for the three kernels");

// a kernel as `grid` blocks of BLOCK threads run it over n entries (grid <= 0: the launch's own)
template <class F> void launch(int64_t n, int grid, F &&body) {
    if (grid <= 0) grid = (int)displace::blocks_for(n);
    for (int block = 0; block < grid; block++)
        for (int tid = 0; tid < displace::BLOCK; tid++)
            for (int64_t i = (int64_t)block * displace::BLOCK + tid; i < n; i += (int64_t)grid * displace::BLOCK) body(i);
}
const double GUARD = -7.25e77;
std::string g_message;

struct Mesh {
    int64_t nv, nf;
    const int32_t *indices;
    std::vector<int32_t> face_start, faces;
};
// the two normal launches over p -> n (nv x 3 + guard); -> 256 when a guard was written
int normals(const Mesh &m, const double *p, int grid, std::vector<double> &n) {
    std::vector<double> fn(3 * (size_t)m.nf + 1, GUARD);
    n.assign(3 * (size_t)m.nv + 1, GUARD);
    launch(m.nf, grid, [&](int64_t f) { subdiv::face_normal(m.indices, p, f, fn.data()); });
    launch(m.nv, grid, [&](int64_t v) { subdiv::vertex_normal(m.face_start.data(), m.faces.data(), fn.data(), v, n.data()); });
    return fn.back() != GUARD || n.back() != GUARD ? 256 : 0;
}
}  // namespace

extern "C" {
const char *displace_host_message() { return g_message.c_str(); }
// What take_hip_displace_create checks and builds, then one call as the library launches it.  real: 0 float texels,
// 1 double texels; lookup: uscale, vscale, uoffset, voffset; normals null: the direction is the own normals of
// `positions`; grid <= 0: every launch's own grid.
// -> out_p (nv x 3), dir_n (nv x 3: the direction that was used), out_n (unless null), and per vertex what the lookup
// did: cells (nv x 4 int32: x1, x2, y1, y2) and fractions (nv x 3: fx, fy, h), unless null.
// -> 0; 1, 2: a refusal of the description (displace_host_message has its words); 256: a write behind an output array
int displace_host_apply(int64_t nv, int64_t nf, const int32_t *indices, const double *uvs, int32_t width, int32_t height, const void *texels, int32_t real,
                        const double *lookup, const double *positions, const double *normals_in, double scale, double bias, int grid, double *out_p, double *dir_n,
                        double *out_n, int32_t *cells, double *fractions) {
    if (int rc = displace::check_inputs(nv, nf, indices, uvs, width, height, texels, real, 0, 0, lookup, g_message)) return rc;
    std::vector<displace::Source> src;
    if (int rc = displace::build_sources(nv, uvs, lookup, src, g_message)) return rc;
    Mesh m{nv, nf, indices, {}, {}};
    displace::build_rows(nv, nf, indices, m.face_start, m.faces);
    int bad = 0;
    std::vector<double> own, after, p(3 * (size_t)nv + 1, GUARD);
    const double *n = normals_in;
    if (!n) {
        bad |= normals(m, positions, grid, own);
        n = own.data();
    }
    if (real == 1)
        launch(nv, grid, [&](int64_t v) { displace::displace_vertex(src.data(), (const double *)texels, width, height, scale, bias, positions, n, v, p.data()); });
    else
        launch(nv, grid, [&](int64_t v) { displace::displace_vertex(src.data(), (const float *)texels, width, height, scale, bias, positions, n, v, p.data()); });
    if (p.back() != GUARD) bad |= 256;
    std::memcpy(out_p, p.data(), sizeof(double) * 3 * (size_t)nv);
    std::memcpy(dir_n, n, sizeof(double) * 3 * (size_t)nv);
    if (out_n) {
        bad |= normals(m, p.data(), grid, after);
        std::memcpy(out_n, after.data(), sizeof(double) * 3 * (size_t)nv);
    }
    for (int64_t v = 0; v < nv && (cells || fractions); v++) {
        int32_t x1, x2, y1, y2;
        double fx, fy;
        displace::cell(src[v].a, width, x1, x2, fx);
        displace::cell(src[v].b, height, y1, y2, fy);
        if (cells) cells[4 * v] = x1, cells[4 * v + 1] = x2, cells[4 * v + 2] = y1, cells[4 * v + 3] = y2;
        if (fractions) {
            fractions[3 * v] = fx, fractions[3 * v + 1] = fy;
            fractions[3 * v + 2] = real == 1 ? displace::height_at((const double *)texels, width, height, src[v]) : displace::height_at((const float *)texels, width, height, src[v]);
        }
    }
    return bad;
}
}

#ifdef DISPLACE_HOST_MAIN
namespace {
struct Surface {  // every array sized exactly: a read behind one is the sanitizer's to find
    std::vector<double> pos, uv;
    std::vector<int32_t> idx;
    int64_t nv() const { return (int64_t)pos.size() / 3; }
    int64_t nf() const { return (int64_t)idx.size() / 3; }
};
Surface strip(int nv, int unused) {
    Surface c;
    for (int i = 0; i < nv; i++) c.pos.insert(c.pos.end(), {0.125 * (i / 2), 0.5 * (i % 2), 0.03125 * ((i * 7) % 5)});
    for (int k = 0; k + 2 < nv; k++) c.idx.insert(c.idx.end(), {k % 2 ? k + 1 : k, k % 2 ? k : k + 1, k + 2});
    for (int i = 0; i < unused; i++) c.pos.insert(c.pos.end(), {9.0, 9.0, 9.0});
    const double corner[][2] = {{0.0, 0.0}, {1.0, 1.0}, {-1e-20, 0.5}, {0.999, -0.3}, {1.6, 0.97}, {-0.75, 2.25}, {-3.0, 3.0}, {1e300, -1e300}};
    for (int64_t i = 0; i < c.nv(); i++) {
        if (i < 8)
            c.uv.insert(c.uv.end(), {corner[i][0], corner[i][1]});
        else
            c.uv.insert(c.uv.end(), {-3.0 + 6.0 * std::fmod(i * 0.61803, 1.0), 3.0 - 6.0 * std::fmod(i * 0.41421, 1.0)});
    }
    return c;
}
template <class T> std::vector<T> image(int w, int h) {
    std::vector<T> t((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) t[(size_t)y * w + x] = (T)(0.6 * std::sin(1.3 * x + 0.4) * std::cos(0.9 * y - 0.2) + 0.05 * ((3 * x + 5 * y) % 7) - 0.1);
    return t;
}
}  // namespace

int main() {
    int bad = 0, cases = 0;
    const Surface surfaces[] = {strip(3, 0), strip(9, 1), strip(23, 0), strip(600, 0)};
    const int shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {5, 3}, {16, 16}, {64, 33}};
    const double lookups[][4] = {{1.0, 1.0, 0.0, 0.0}, {1.7, -0.6, 0.25, 0.4}};
    for (const Surface &c : surfaces)
        for (const auto &wh : shapes)
            for (int real = 0; real < 2; real++)
                for (int grid : {0, 1, 2, 3}) {
                    const int w = wh[0], h = wh[1];
                    const std::vector<float> tf = image<float>(w, h);
                    const std::vector<double> td = image<double>(w, h);
                    const void *texels = real ? (const void *)td.data() : (const void *)tf.data();
                    double lo = real ? td[0] : (double)tf[0], hi = lo;
                    for (size_t k = 0; k < td.size(); k++) {
                        const double t = real ? td[k] : (double)tf[k];
                        lo = t < lo ? t : lo, hi = t > hi ? t : hi;
                    }
                    const int64_t nv = c.nv();
                    std::vector<double> p(3 * (size_t)nv), dn(3 * (size_t)nv), n(3 * (size_t)nv), fr(3 * (size_t)nv);
                    std::vector<int32_t> cells(4 * (size_t)nv);
                    int rc = 0;
                    for (int own = 0; own < 2 && !rc; own++) {
                        std::vector<double> given(3 * (size_t)nv, 0.0);
                        for (int64_t v = 0; v < nv; v++) given[3 * v + 2] = 1.0;
                        rc = displace_host_apply(nv, c.nf(), c.idx.data(), c.uv.data(), w, h, texels, real, lookups[(cases + own) % 2], c.pos.data(), own ? nullptr : given.data(),
                                                 0.25, -0.05, grid, p.data(), dn.data(), own ? n.data() : nullptr, cells.data(), fr.data());
                        for (double x : p)
                            if (!rc && !std::isfinite(x)) rc = 2048;
                        for (int64_t v = 0; v < nv && !rc; v++) {
                            const int32_t *q = &cells[4 * v];
                            if (q[0] < 0 || q[0] >= w || q[1] < 0 || q[1] >= w || q[2] < 0 || q[2] >= h || q[3] < 0 || q[3] >= h) rc = 4096;
                            if (!(fr[3 * v] >= 0 && fr[3 * v] < 1 && fr[3 * v + 1] >= 0 && fr[3 * v + 1] < 1)) rc = 8192;
                            if (!(fr[3 * v + 2] >= lo - 1e-12 && fr[3 * v + 2] <= hi + 1e-12)) rc = 16384;  // (never outside the image's range)
                        }
                    }
                    if (rc) std::printf("MISMATCH mesh of %lld vertices, image %d x %d, real %d, grid %d: %d %s\n", (long long)nv, w, h, real, grid, rc, displace_host_message()), bad++;
                    cases++;
                }
    {  // what creation refuses
        Surface c = strip(9, 0);
        const std::vector<double> t = image<double>(2, 2);
        std::vector<double> out(3 * 9);
        const double ok[4] = {1.0, 1.0, 0.0, 0.0}, nan[4] = {1.0, NAN, 0.0, 0.0}, inf[4] = {1e300, 1.0, 1e300, 0.0};
        auto run = [&](const int32_t *idx, const double *uv, int w, int h, int real, const double *lookup) {
            return displace_host_apply(9, 7, idx, uv, w, h, t.data(), real, lookup, c.pos.data(), nullptr, 1.0, 0.0, 0, out.data(), out.data(), nullptr, nullptr, nullptr);
        };
        std::vector<int32_t> range = c.idx;
        range[4] = 9;
        std::vector<double> overflow = c.uv;
        overflow[6] = 1e300;  // 1e300 * 1e300 + 1e300: s is not finite
        if (run(range.data(), c.uv.data(), 2, 2, 1, ok) != 1) std::printf("MISMATCH an index out of range accepted\n"), bad++;
        if (run(c.idx.data(), nullptr, 2, 2, 1, ok) != 1) std::printf("MISMATCH missing uvs accepted\n"), bad++;
        if (run(c.idx.data(), c.uv.data(), 0, 2, 1, ok) != 1) std::printf("MISMATCH a width of 0 accepted\n"), bad++;
        if (run(c.idx.data(), c.uv.data(), 65536, 65536, 1, ok) != 1) std::printf("MISMATCH an image beyond INT32_MAX texels accepted\n"), bad++;
        if (run(c.idx.data(), c.uv.data(), 2, 2, 2, ok) != 1) std::printf("MISMATCH an unknown texel width accepted\n"), bad++;
        if (run(c.idx.data(), c.uv.data(), 2, 2, 1, nan) != 1) std::printf("MISMATCH a NaN lookup parameter accepted\n"), bad++;
        if (run(c.idx.data(), overflow.data(), 2, 2, 1, inf) != 1) std::printf("MISMATCH a lookup coordinate that is not finite accepted\n"), bad++;
        if (run(c.idx.data(), c.uv.data(), 2, 2, 1, ok) != 0) std::printf("MISMATCH the valid description refused: %s\n", displace_host_message()), bad++;
        cases += 8;
    }
    std::printf("displace_host: %d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
