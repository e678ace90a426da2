// subdiv_host.cpp — TEST INFRASTRUCTURE.  take_amd/csrc/tk_subdiv.h built for the host: its topology build as it is, and
// its bodies run in the loop structure of its kernels' launches — blocks of BLOCK threads, one vertex, edge or face per
// thread, the blocks striding when the grid is smaller than the work, the tail block partly idle, a guard element behind
// every output array that must stay untouched — so that tests/test_subdiv_cpu.py can hold what take_hip_subdiv_refine
// computes to tests/subdiv_ref.py bit for bit without a GPU, and tests/test_gpu_subdiv.py the device's output to this.
// With -DSUBDIV_HOST_MAIN a stand-alone program that runs the bodies over cages it makes itself and checks bounds and a
// few exact properties (the sanitizer build of the Makefile).  Never loaded by the product.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tk_subdiv.h"

namespace {
using namespace tk;

// a kernel of tk_subdiv.h as `grid` blocks of BLOCK threads run it over n entries (grid <= 0: the launch's own)
template <class F> void launch(int64_t n, int grid, F &&body) {
    if (grid <= 0) grid = (int)subdiv::blocks_for(n);
    for (int block = 0; block < grid; block++)
        for (int tid = 0; tid < subdiv::BLOCK; tid++)
            for (int64_t i = (int64_t)block * subdiv::BLOCK + tid; i < n; i += (int64_t)grid * subdiv::BLOCK) body(i);
}
const double GUARD = -7.25e77;
std::string g_message;
}  // namespace

extern "C" {
const char *subdiv_host_message() { return g_message.c_str(); }
// -> 0, or the builder's refusal (1 invalid, 2 unsupported; subdiv_host_message has its words)
int subdiv_host_counts(int64_t n_vertices, int64_t n_faces, const int32_t *indices, int32_t levels, int64_t *nv_out, int64_t *nf_out) {
    subdiv::Topology topo;
    if (int rc = subdiv::build_topology(n_vertices, n_faces, indices, nullptr, levels, false, topo, g_message)) return rc;
    *nv_out = topo.n_vertices, *nf_out = topo.n_faces;
    return 0;
}
// A cage (host arrays; uvs null as there) refined `levels` times, as the library's refine launches it -> the refined
// indices, uvs (unless null), positions and normals (unless null).  grid <= 0: every launch's own grid.
// -> 0; 1, 2: the builder's refusal; 256: a write behind an output array
int subdiv_host_refine(int64_t n_vertices, int64_t n_faces, const int32_t *indices, const double *uvs, int32_t levels, const double *cage, int grid, int32_t *indices_out,
                       double *uvs_out, double *out_p, double *out_n) {
    subdiv::Topology topo;
    if (int rc = subdiv::build_topology(n_vertices, n_faces, indices, uvs, levels, true, topo, g_message)) return rc;
    std::vector<double> in(cage, cage + 3 * n_vertices), out;
    int bad = 0;
    for (const subdiv::Level &lv : topo.levels) {
        const subdiv::LevelView t = lv.view();
        out.assign(3 * (size_t)(lv.n_vertices + lv.n_edges) + 1, GUARD);
        launch(t.n_vertices, grid, [&](int64_t v) { subdiv::even_vertex(t, in.data(), v, out.data()); });
        launch(t.n_edges, grid, [&](int64_t e) { subdiv::odd_vertex(t, in.data(), e, out.data()); });
        if (out.back() != GUARD) bad = 256;
        out.pop_back();
        in.swap(out);
    }
    std::memcpy(out_p, in.data(), sizeof(double) * in.size());
    std::memcpy(indices_out, topo.indices.data(), sizeof(int32_t) * topo.indices.size());
    if (uvs_out) std::memcpy(uvs_out, topo.uvs.data(), sizeof(double) * topo.uvs.size());
    if (out_n) {
        std::vector<double> fn(3 * (size_t)topo.n_faces + 1, GUARD), n(3 * (size_t)topo.n_vertices + 1, GUARD);
        launch(topo.n_faces, grid, [&](int64_t f) { subdiv::face_normal(topo.indices.data(), in.data(), f, fn.data()); });
        launch(topo.n_vertices, grid, [&](int64_t v) { subdiv::vertex_normal(topo.face_start.data(), topo.faces.data(), fn.data(), v, n.data()); });
        if (fn.back() != GUARD || n.back() != GUARD) bad = 256;
        // the variant without the face-normal array gives the same bits
        std::vector<double> again(3 * (size_t)topo.n_vertices + 1, GUARD);
        launch(topo.n_vertices, grid, [&](int64_t v) { subdiv::vertex_normal_recomputed(topo.face_start.data(), topo.faces.data(), topo.indices.data(), in.data(), v, again.data()); });
        if (again.back() != GUARD) bad = 256;
        if (!bad && std::memcmp(again.data(), n.data(), sizeof(double) * 3 * (size_t)topo.n_vertices)) bad = 512;
        std::memcpy(out_n, n.data(), sizeof(double) * 3 * (size_t)topo.n_vertices);
    }
    return bad;
}
}

#ifdef SUBDIV_HOST_MAIN
namespace {
struct Cage {  // every array sized exactly: a read behind one is the sanitizer's to find
    std::vector<double> pos;
    std::vector<int32_t> idx;
    int64_t nv() const { return (int64_t)pos.size() / 3; }
    int64_t nf() const { return (int64_t)idx.size() / 3; }
};
Cage strip(int nv, int unused) {
    Cage c;
    for (int i = 0; i < nv; i++) c.pos.insert(c.pos.end(), {0.125 * (i / 2), 0.5 * (i % 2), 0.03125 * ((i * 7) % 5)});
    for (int k = 0; k + 2 < nv; k++) c.idx.insert(c.idx.end(), {k % 2 ? k + 1 : k, k % 2 ? k : k + 1, k + 2});
    for (int i = 0; i < unused; i++) c.pos.insert(c.pos.end(), {9.0, 9.0, 9.0});
    return c;
}
Cage fan(int n, bool closed) {
    Cage c;
    c.pos = {0.0, 0.0, 1.0};
    for (int k = 0; k < n; k++) c.pos.insert(c.pos.end(), {std::cos(0.1 * k), std::sin(0.1 * k), 0.0});
    for (int k = 0; k < (closed ? n : n - 1); k++) c.idx.insert(c.idx.end(), {0, 1 + k, 1 + (k + 1) % n});
    return c;
}
Cage octahedron() {
    Cage c;
    c.pos = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    c.idx = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    return c;
}
}  // namespace

int main() {
    int bad = 0, cases = 0;
    const Cage cages[] = {octahedron(), strip(3, 0), strip(9, 1), strip(23, 0), strip(33, 0), fan(7, false), fan(200, true)};
    for (const Cage &c : cages)
        for (int levels = 1; levels <= 4; levels++)
            for (int grid : {0, 1, 2, 3}) {
                int64_t nv = 0, nf = 0;
                int rc = subdiv_host_counts(c.nv(), c.nf(), c.idx.data(), levels, &nv, &nf);
                if (!rc && nv > 20000) continue;
                std::vector<int32_t> idx(3 * (size_t)nf);
                std::vector<double> p(3 * (size_t)nv), n(3 * (size_t)nv);
                for (int with_normals = 0; with_normals < 2 && !rc; with_normals++) {
                    rc = subdiv_host_refine(c.nv(), c.nf(), c.idx.data(), nullptr, levels, c.pos.data(), grid, idx.data(), nullptr, p.data(), with_normals ? n.data() : nullptr);
                    for (double x : p)
                        if (!rc && !std::isfinite(x)) rc = 2048;
                    for (int32_t i : idx)
                        if (!rc && (i < 0 || i >= nv)) rc = 4096;
                    if (!rc && with_normals)  // unit length or exactly zero
                        for (int64_t v = 0; v < nv; v++) {
                            const double l = std::sqrt(n[3 * v] * n[3 * v] + n[3 * v + 1] * n[3 * v + 1] + n[3 * v + 2] * n[3 * v + 2]);
                            if (l != 0 && std::fabs(l - 1) > 1e-15) rc = 8192;
                        }
                }
                if (rc) std::printf("MISMATCH cage of %lld vertices, %d levels, grid %d: %d %s\n", (long long)c.nv(), levels, grid, rc, subdiv_host_message()), bad++;
                cases++;
            }
    {  // what the builder refuses
        int64_t nv, nf;
        Cage c = strip(9, 0);
        const int32_t bowtie[] = {0, 1, 2, 2, 3, 4}, three[] = {0, 1, 2, 1, 0, 3, 0, 1, 4}, twice[] = {0, 1, 1}, range[] = {0, 1, 5};
        if (subdiv_host_counts(5, 2, bowtie, 1, &nv, &nf) != 1) std::printf("MISMATCH bow-tie accepted\n"), bad++;
        if (subdiv_host_counts(5, 3, three, 1, &nv, &nf) != 1) std::printf("MISMATCH an edge of three faces accepted\n"), bad++;
        if (subdiv_host_counts(5, 1, twice, 1, &nv, &nf) != 1) std::printf("MISMATCH a repeated index accepted\n"), bad++;
        if (subdiv_host_counts(5, 1, range, 1, &nv, &nf) != 1) std::printf("MISMATCH an index out of range accepted\n"), bad++;
        if (subdiv_host_counts(c.nv(), c.nf(), c.idx.data(), 0, &nv, &nf) != 1 || subdiv_host_counts(c.nv(), c.nf(), c.idx.data(), 7, &nv, &nf) != 1)
            std::printf("MISMATCH levels outside 1..6 accepted\n"), bad++;
        cases += 5;
    }
    std::printf("subdiv_host: %d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
