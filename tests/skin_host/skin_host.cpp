// skin_host.cpp — TEST INFRASTRUCTURE.  The bodies of take_amd/csrc/tk_skin.h built for the host and run in the loop
// structure of its kernels' launches — blocks of BLOCK threads, one joint or vertex per thread, the blocks striding when
// the grid is smaller than the work, the tail block partly idle, a guard element behind every output array that must stay
// untouched — so that tests/test_skin_cpu.py can hold what take_hip_rig_pose computes to tests/skin_ref.py bit for
// bit without a GPU, and tests/test_gpu_skin.py the device's output to this.  With -DSKIN_HOST_MAIN a stand-alone program
// that runs the bodies over rigs it makes itself and checks bounds and a few exact properties (the sanitizer build of
// the Makefile).  Never loaded by the product.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tk_skin.h"

namespace {
using namespace tk;

// a kernel of tk_skin.h as `grid` blocks of BLOCK threads run it over n entries (grid <= 0: the launch's own)
template <class F> void launch(int64_t n, int grid, F &&body) {
    if (grid <= 0) grid = (int)skin::blocks_for(n);
    for (int block = 0; block < grid; block++)
        for (int tid = 0; tid < skin::BLOCK; tid++)
            for (int64_t i = (int64_t)block * skin::BLOCK + tid; i < n; i += (int64_t)grid * skin::BLOCK) body(i);
}
const double GUARD = -7.25e77;
}  // namespace

extern "C" {
// the joint count up to which the pose kernel keeps the palette in LDS
int skin_host_lds_max_joints() { return skin::LDS_MAX_JOINTS; }
// TakeRigDesc's arrays and a pose, all in host memory (null as there) -> out_p, and out_n unless null (n_vertices x 3
// each).  grid <= 0: the launch's own grid.  -> 0, or 256 = a write behind an output array
int skin_host_pose(int64_t n_vertices, int32_t n_joints, int32_t K, int32_t T, const double *rest_p, const double *rest_n, const int32_t *joints, const double *weights,
                   const double *inverse_bind, const double *target_p, const double *target_n, const double *joint_xforms, const double *target_weights, int grid,
                   double *out_p, double *out_n) {
    std::vector<double> palette(12 * (size_t)n_joints + 1, GUARD), p(3 * (size_t)n_vertices + 1, GUARD), n(3 * (size_t)n_vertices + 1, GUARD);
    launch(n_joints, grid, [&](int64_t j) { skin::palette_entry(joint_xforms, inverse_bind, palette.data(), j); });
    const skin::RigView r{n_vertices, n_joints, K, T, rest_p, rest_n, joints, weights, target_p, target_n};
    launch(n_vertices, grid, [&](int64_t v) { skin::pose_vertex(r, palette.data(), target_weights, v, p.data(), out_n ? n.data() : nullptr); });
    const int bad = (palette.back() != GUARD || p.back() != GUARD || n.back() != GUARD) ? 256 : 0;
    std::memcpy(out_p, p.data(), sizeof(double) * 3 * (size_t)n_vertices);
    if (out_n) std::memcpy(out_n, n.data(), sizeof(double) * 3 * (size_t)n_vertices);
    return bad;
}
// the smallest vertex with a joint index outside [0, n_joints), -1: none (k_skin_check_joints)
int64_t skin_host_check_joints(const int32_t *joints, int32_t K, int32_t n_joints, int64_t n_vertices, int grid) {
    unsigned long long bad = ~0ull;
    launch(n_vertices, grid, [&](int64_t v) {
        if (skin::bad_joint(joints, K, n_joints, v) && (unsigned long long)v < bad) bad = (unsigned long long)v;
    });
    return bad == ~0ull ? -1 : (int64_t)bad;
}
}

#ifdef SKIN_HOST_MAIN
namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
double draw() {  // (xorshift64*: any fixed sequence will do)
    g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}
struct Made {  // every array sized exactly: a read behind one is the sanitizer's to find
    std::vector<double> rest_p, rest_n, weights, bind, tp, tn, X, tw;
    std::vector<int32_t> joints;
    Made(int64_t nv, int nj, int K, int T, bool identity) {
        for (int64_t i = 0; i < 3 * nv; i++) rest_p.push_back(2 * draw() - 1), rest_n.push_back(i % 3 == 2 ? 1.0 : 0.0);
        for (int64_t i = 0; i < nv * K; i++) joints.push_back((int32_t)(draw() * nj) % nj), weights.push_back(i % K == 0 ? 0.5 : (i % K < 3 ? 0.25 : 0.0));
        if (K == 1) weights.assign((size_t)nv, 1.0);
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < 12; i++) {
                const double one = i % 5 == 0 ? 1.0 : 0.0;
                X.push_back(identity ? one : one + 0.5 * draw()), bind.push_back(identity ? one : one + 0.25 * draw());
            }
        for (int64_t i = 0; i < 3 * nv * T; i++) tp.push_back(0.1 * draw()), tn.push_back(0.1 * draw());
        for (int t = 0; t < T; t++) tw.push_back(identity ? 0.0 : draw());
    }
};
}  // namespace

int main() {
    int bad = 0, cases = 0;
    const int64_t counts[] = {1, 63, 64, 65, 257, 1301};
    const int joint_counts[] = {0, 1, 2, skin::LDS_MAX_JOINTS, skin::LDS_MAX_JOINTS + 1};
    for (int64_t nv : counts)
        for (int nj : joint_counts)
            for (int K : {1, 4, 8})
                for (int T : {0, 1, 3})
                    for (int grid : {0, 1, 2, 3}) {
                        if (grid && nv != 1301) continue;  // (1-3 blocks that stride over the 1301)
                        if (nj == 0 && K != 1) continue;
                        for (int identity = 0; identity < 2; identity++) {
                            Made m(nv, nj, nj ? K : 0, T, identity != 0);
                            std::vector<double> p(3 * (size_t)nv), n(3 * (size_t)nv);
                            for (int with_normals = 0; with_normals < 2; with_normals++) {
                                int rc = skin_host_pose(nv, nj, nj ? K : 0, T, m.rest_p.data(), with_normals ? m.rest_n.data() : nullptr, nj ? m.joints.data() : nullptr,
                                                        nj ? m.weights.data() : nullptr, nj && !identity ? m.bind.data() : nullptr, T ? m.tp.data() : nullptr,
                                                        T && with_normals ? m.tn.data() : nullptr, nj ? m.X.data() : nullptr, T ? m.tw.data() : nullptr, grid, p.data(),
                                                        with_normals ? n.data() : nullptr);
                                // identity joints, binary-fraction weights that sum to 1, zero target weights: the rest pose bit for bit
                                if (!rc && identity && std::memcmp(p.data(), m.rest_p.data(), sizeof(double) * p.size())) rc = 512;
                                if (!rc && identity && with_normals && std::memcmp(n.data(), m.rest_n.data(), sizeof(double) * n.size())) rc = 1024;
                                for (double x : p)
                                    if (!rc && !std::isfinite(x)) rc = 2048;
                                if (rc) std::printf("MISMATCH nv %lld nj %d K %d T %d grid %d identity %d normals %d: %d\n", (long long)nv, nj, K, T, grid, identity, with_normals, rc);
                                bad += rc ? 1 : 0, cases++;
                            }
                        }
                    }
    {  // the joint-range check: the smallest bad vertex, whatever the grid
        Made m(1301, 4, 4, 0, false);
        m.joints[4 * 700 + 2] = 4, m.joints[4 * 300 + 1] = -1, m.joints[4 * 1300 + 3] = 99;
        for (int grid : {0, 1, 2, 3}) {
            const int64_t got = skin_host_check_joints(m.joints.data(), 4, 4, 1301, grid);
            if (got != 300) std::printf("MISMATCH joint check, grid %d: %lld\n", grid, (long long)got), bad++;
            cases++;
        }
        m.joints[4 * 700 + 2] = m.joints[4 * 300 + 1] = m.joints[4 * 1300 + 3] = 0;
        if (skin_host_check_joints(m.joints.data(), 4, 4, 1301, 0) != -1) std::printf("MISMATCH joint check of a good rig\n"), bad++;
        cases++;
    }
    std::printf("skin_host: %d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
