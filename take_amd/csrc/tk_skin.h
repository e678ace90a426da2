// tk_skin.h — linear-blend skinning over a joint palette plus morph targets: what take_hip_rig_pose*, and
// take_hip_scene_pose_meshes in front of the mesh update, compute on the device (include/take_hip.h; specification:
// DESIGN.md §4q).  The bodies below are TK_HD and written once: the kernels at the end of this file run them on the
// device, tests/skin_host runs them in the kernels' loop structure on the host.  Launched from tk_skin.hip.
//
// Arithmetic: everything is double; every + - * / is one operation in the order written (-ffp-contract=off); the square
// root of a normal's length is the only library call, correctly rounded on both sides.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "tk_common.h"

namespace tk {
namespace skin {

// What the kernels read of a rig (TakeRigDesc's arrays in device memory; on the host, the test's arrays).
struct RigView {
    int64_t n_vertices;
    int32_t n_joints, n_influences, n_targets;  // K = n_influences: 1..8 with joints, else 0
    const double *rest_p, *rest_n;               // n_vertices x 3; rest_n null: the rig poses no normals
    const int32_t *joints;                       // n_vertices x K
    const double *weights;                       // n_vertices x K
    const double *target_p, *target_n;           // T x n_vertices x 3 deltas, target-major; target_n may be null
};

// Entry j of the palette: J = X_j · B_j as 3x4 affine matrices (row-major, 12 doubles each), the translation column's
// + X[r][3] added last; B == null (no inverse bind matrices): J = X_j copied, not multiplied.
TK_HD void palette_entry(const double *X, const double *B, double *J, int64_t j) {
    const double *x = X + 12 * j;
    double *o = J + 12 * j;
    if (!B) {
        for (int i = 0; i < 12; i++) o[i] = x[i];
        return;
    }
    const double *b = B + 12 * j;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            double s = (x[4 * r + 0] * b[0 + c] + x[4 * r + 1] * b[4 + c]) + x[4 * r + 2] * b[8 + c];
            if (c == 3) s = s + x[4 * r + 3];
            o[4 * r + c] = s;
        }
}

// Vertex v of the rig under `palette` (n_joints x 12) and the target weights tw (T) -> out_p[3 v ..], and out_n[3 v ..]
// when out_n is not null (the rig then has rest normals).
//  1. morph: p = rest, then p = p + w_t * dp_t for t = 0 .. T-1 in order; n likewise with the targets' normal deltas
//     when the rig has them; no target is skipped for a zero weight
//  2. blend (n_joints > 0): M = weight_0 * J[joint_0], then M = M + weight_k * J[joint_k], k = 1 .. K-1, on all 12
//     entries; no influence is skipped, weights are taken as they are
//  3. p'_r = ((M[r][0] p.x + M[r][1] p.y) + M[r][2] p.z) + M[r][3]
//  4. n' = C n with C the cofactor matrix of M's 3x3 part A, indices mod 3:
//         C[i][j] = A[i+1][j+1] * A[i+2][j+2] - A[i+1][j+2] * A[i+2][j+1]
//     (the inverse transpose times det, without a division: right under non-uniform scale and under mirroring),
//     n'_r = (C[r][0] n.x + C[r][1] n.y) + C[r][2] n.z, negated when det = (A00 C00 + A01 C01) + A02 C02 < 0
//  a morph-only rig (n_joints == 0): p' = p, n' = n
//  5. len = sqrt((n'.x n'.x + n'.y n'.y) + n'.z n'.z); n' / len per component when len > 0 and finite, else n' as it is
TK_HD void pose_vertex(const RigView &r, const double *palette, const double *tw, int64_t v, double *out_p, double *out_n) {
    const bool normals = out_n != nullptr;
    double p[3], n[3] = {0, 0, 0};
    for (int a = 0; a < 3; a++) p[a] = r.rest_p[3 * v + a];
    if (normals)
        for (int a = 0; a < 3; a++) n[a] = r.rest_n[3 * v + a];
    for (int t = 0; t < r.n_targets; t++) {
        const double w = tw[t];
        const int64_t at = 3 * ((int64_t)t * r.n_vertices + v);
        for (int a = 0; a < 3; a++) p[a] = p[a] + w * r.target_p[at + a];
        if (normals && r.target_n)
            for (int a = 0; a < 3; a++) n[a] = n[a] + w * r.target_n[at + a];
    }
    if (r.n_joints > 0) {
        const int K = r.n_influences;
        const int32_t *jv = r.joints + (int64_t)K * v;
        const double *wv = r.weights + (int64_t)K * v;
        double M[12];
        {
            const double w = wv[0];
            const int64_t at = 12 * (int64_t)jv[0];
            for (int i = 0; i < 12; i++) M[i] = w * palette[at + i];
        }
        for (int k = 1; k < K; k++) {
            const double w = wv[k];
            const int64_t at = 12 * (int64_t)jv[k];
            for (int i = 0; i < 12; i++) M[i] = M[i] + w * palette[at + i];
        }
        double q[3];
        for (int i = 0; i < 3; i++) q[i] = ((M[4 * i + 0] * p[0] + M[4 * i + 1] * p[1]) + M[4 * i + 2] * p[2]) + M[4 * i + 3];
        for (int a = 0; a < 3; a++) p[a] = q[a];
        if (normals) {
            double Cf[9];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) {
                    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
                    Cf[3 * i + j] = M[4 * i1 + j1] * M[4 * i2 + j2] - M[4 * i1 + j2] * M[4 * i2 + j1];
                }
            const double det = (M[0] * Cf[0] + M[1] * Cf[1]) + M[2] * Cf[2];
            for (int i = 0; i < 3; i++) q[i] = (Cf[3 * i + 0] * n[0] + Cf[3 * i + 1] * n[1]) + Cf[3 * i + 2] * n[2];
            for (int a = 0; a < 3; a++) n[a] = det < 0 ? -q[a] : q[a];
        }
    }
    for (int a = 0; a < 3; a++) out_p[3 * v + a] = p[a];
    if (normals) {
        const double len = tk_sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        if (len > 0 && len <= 1.7976931348623157e308)  // (finite: neither inf nor NaN)
            for (int a = 0; a < 3; a++) n[a] = n[a] / len;
        for (int a = 0; a < 3; a++) out_n[3 * v + a] = n[a];
    }
}

// vertex v of a rig whose arrays are in device memory: has it a joint index outside [0, n_joints)?
TK_HD bool bad_joint(const int32_t *joints, int32_t K, int32_t n_joints, int64_t v) {
    bool bad = false;
    for (int k = 0; k < K; k++) bad = bad || joints[(int64_t)K * v + k] < 0 || joints[(int64_t)K * v + k] >= n_joints;
    return bad;
}

constexpr int BLOCK = 256;
constexpr int64_t MAX_BLOCKS = 1 << 16;  // a launch's grid: beyond BLOCK * MAX_BLOCKS entries the blocks stride
inline int64_t blocks_for(int64_t n) {
    const int64_t b = (n + BLOCK - 1) / BLOCK;
    return b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b);
}
// A palette of at most this many joints is copied into LDS by every block before its vertices are posed (12 KiB, which
// leaves a CU's 160 KiB room for every block its waves allow); a larger one is gathered from global memory.
constexpr int32_t LDS_MAX_JOINTS = 128;

#if defined(__HIPCC__)
// one lane per joint
__global__ __launch_bounds__(BLOCK) void k_skin_palette(const double *__restrict__ X, const double *__restrict__ B, double *__restrict__ J, int64_t n_joints) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < n_joints; j += (int64_t)gridDim.x * BLOCK) palette_entry(X, B, J, j);
}
// One lane per vertex, consecutive lanes consecutive vertices: a wave reads 1536 contiguous bytes of each of rest
// positions, rest normals and every target's deltas, K * 256 of joints and K * 512 of weights, and writes 1536 per output —
// every byte of every line used.  The palette is the only gather: 96-byte records by joint, from LDS (STAGED: the
// block's copy, filled by all its threads) or from global memory.
template <bool STAGED> __global__ __launch_bounds__(BLOCK) void k_skin_pose(RigView r, const double *__restrict__ palette, const double *__restrict__ tw, double *out_p, double *out_n) {
    if constexpr (STAGED) {
        __shared__ double staged[12 * LDS_MAX_JOINTS];
        for (int i = threadIdx.x; i < 12 * r.n_joints; i += BLOCK) staged[i] = palette[i];
        __syncthreads();
        for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < r.n_vertices; v += (int64_t)gridDim.x * BLOCK) pose_vertex(r, staged, tw, v, out_p, out_n);
    } else {
        for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < r.n_vertices; v += (int64_t)gridDim.x * BLOCK) pose_vertex(r, palette, tw, v, out_p, out_n);
    }
}
// *bad (all ones before): the smallest vertex with a joint index out of range
__global__ __launch_bounds__(BLOCK) void k_skin_check_joints(const int32_t *__restrict__ joints, int32_t K, int32_t n_joints, int64_t n_vertices, unsigned long long *bad) {
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < n_vertices; v += (int64_t)gridDim.x * BLOCK)
        if (bad_joint(joints, K, n_joints, v)) atomicMin(bad, (unsigned long long)v);
}
#endif  // __HIPCC__

}  // namespace skin
}  // namespace tk
