// tk_features.h — first-hit feature buffers (take_hip_render_features*): albedo, shading normal, depth, coverage and
// the ids of the camera ray's hit, the auxiliary images a denoiser or compositor asks a path tracer for.
//
//   k_features          per pixel, the batch's samples in sample order (the walk of k_accumulate): the hit the closest-hit
//                       launch left in the path record -> make_isect -> eval_texture -> per-pixel sums; the ids of
//                       sample 0 go straight to the caller's planes
//   k_features_resolve  divide by spp, vertical flip (as k_resolve)
//
// The pass is the camera + closest-hit launch of a render's round 0 followed by k_features: no sort, no shade round,
// no shadow rays.  Nothing here is reached by a render.
#pragma once

#include "tk_kernels.h"

namespace tk {

// which planes the caller wants (a NULL pointer in TakeFeatureBuffers = not wanted: nothing is read or written for it)
enum FeatureBit : uint32_t { F_ALBEDO = 1, F_NORMAL = 2, F_DEPTH = 4, F_ALPHA = 8, F_SHAPE = 16, F_MATERIAL = 32 };
// per-pixel sums, one plane of npix values per word (a wave reads and writes whole lines of each plane)
enum FeatureWord { FW_ALBEDO = 0, FW_NORMAL = 3, FW_DEPTH = 6, FW_ALPHA = 7, FEATURE_WORDS = 8 };

template <class R> struct FeatureOut {  // TakeFeatureBuffers for records of precision R, in device memory
    R *albedo, *normal, *depth, *alpha;
    int32_t *shape_id, *material_id;
    uint32_t want() const {
        return (albedo ? F_ALBEDO : 0u) | (normal ? F_NORMAL : 0u) | (depth ? F_DEPTH : 0u) | (alpha ? F_ALPHA : 0u) |
               (shape_id ? F_SHAPE : 0u) | (material_id ? F_MATERIAL : 0u);
    }
};

// local pixel p (render-loop order: local row 0 = the bottom row of this rank's rows) -> its place in the output
__device__ __forceinline__ int64_t feature_out_index(int32_t p, int32_t width, int32_t n_local_rows) {
    const int lr = p / width, x = p % width;
    return (int64_t)(n_local_rows - 1 - lr) * width + x;
}

// ids: written only by the batch that holds sample 0 (`first_batch`).  A sample that misses adds nothing.
template <class R>
__global__ void __launch_bounds__(BLOCK)
k_features(DeviceScene<R> sc, PathState<R> st, R *acc, FeatureOut<R> out, int32_t width, int32_t n_local_rows, int32_t spb,
           int first_batch, uint32_t want) {
    const int32_t npix = width * n_local_rows;
    // the Isect is needed for the normal, the uv of the albedo and the (placement-resolved) material
    const bool isect = (want & (F_ALBEDO | F_NORMAL)) != 0 || (first_batch && (want & F_MATERIAL));
    for (int32_t p = blockIdx.x * BLOCK + threadIdx.x; p < npix; p += gridDim.x * BLOCK) {
        Vec3<R> alb{R(0), R(0), R(0)}, nrm{R(0), R(0), R(0)};
        R depth = R(0), alpha = R(0);
        if (want & F_ALBEDO) alb = {acc[(int64_t)(FW_ALBEDO + 0) * npix + p], acc[(int64_t)(FW_ALBEDO + 1) * npix + p], acc[(int64_t)(FW_ALBEDO + 2) * npix + p]};
        if (want & F_NORMAL) nrm = {acc[(int64_t)(FW_NORMAL + 0) * npix + p], acc[(int64_t)(FW_NORMAL + 1) * npix + p], acc[(int64_t)(FW_NORMAL + 2) * npix + p]};
        if (want & F_DEPTH) depth = acc[(int64_t)FW_DEPTH * npix + p];
        if (want & F_ALPHA) alpha = acc[(int64_t)FW_ALPHA * npix + p];
        for (int s = 0; s < spb; s++) {
            const int64_t slot = (int64_t)s * npix + p;
            const int32_t prim = st.I_(S_HIT, slot);
            const bool ids = first_batch && s == 0 && (want & (F_SHAPE | F_MATERIAL));
            int32_t shape = -1, material = -1;
            if (prim >= 0) {
                const R t = st.R_(S_HT, slot);
                const int32_t inst = sc.inst_shade ? st.I_(S_INST, slot) : -1;
                if (isect) {
                    const Vec3<R> ro{st.R_(S_OX, slot), st.R_(S_OY, slot), st.R_(S_OZ, slot)};
                    const Vec3<R> rd{st.R_(S_DX, slot), st.R_(S_DY, slot), st.R_(S_DZ, slot)};
                    Isect<R> v{};
                    make_isect(sc, ro, rd, prim, t, st.R_(S_HU, slot), st.R_(S_HV, slot), v, inst);
                    material = v.material;
                    nrm = nrm + v.sn;
                    if (want & F_ALBEDO) alb = alb + eval_texture(sc, sc.materials[v.material], v.uv);
                }
                depth = depth + t;
                alpha = alpha + R(1);
                if (ids && (want & F_SHAPE)) {  // the trace hooks' numbering (HookIo): a placement's faces follow the shapes
                    shape = sc.prims[prim].shape_id;
                    if (inst >= 0) shape += sc.inst_shade[inst].shape_base;
                }
            }
            if (ids) {
                const int64_t o = feature_out_index(p, width, n_local_rows);
                if (want & F_SHAPE) out.shape_id[o] = shape;
                if (want & F_MATERIAL) out.material_id[o] = material;
            }
        }
        if (want & F_ALBEDO) acc[(int64_t)(FW_ALBEDO + 0) * npix + p] = alb.x, acc[(int64_t)(FW_ALBEDO + 1) * npix + p] = alb.y, acc[(int64_t)(FW_ALBEDO + 2) * npix + p] = alb.z;
        if (want & F_NORMAL) acc[(int64_t)(FW_NORMAL + 0) * npix + p] = nrm.x, acc[(int64_t)(FW_NORMAL + 1) * npix + p] = nrm.y, acc[(int64_t)(FW_NORMAL + 2) * npix + p] = nrm.z;
        if (want & F_DEPTH) acc[(int64_t)FW_DEPTH * npix + p] = depth;
        if (want & F_ALPHA) acc[(int64_t)FW_ALPHA * npix + p] = alpha;
    }
}

// sum / spp into the caller's planes, local rows in increasing image row (src/render.cpp:78, as k_resolve)
template <class R>
__global__ void __launch_bounds__(BLOCK)
k_features_resolve(const R *__restrict__ acc, FeatureOut<R> out, int32_t width, int32_t n_local_rows, int32_t spp) {
    const int32_t npix = width * n_local_rows;
    const R n = R(spp);
    for (int32_t p = blockIdx.x * BLOCK + threadIdx.x; p < npix; p += gridDim.x * BLOCK) {
        const int64_t o = feature_out_index(p, width, n_local_rows);
        if (out.albedo)
            for (int c = 0; c < 3; c++) out.albedo[3 * o + c] = acc[(int64_t)(FW_ALBEDO + c) * npix + p] / n;
        if (out.normal)
            for (int c = 0; c < 3; c++) out.normal[3 * o + c] = acc[(int64_t)(FW_NORMAL + c) * npix + p] / n;
        if (out.depth) out.depth[o] = acc[(int64_t)FW_DEPTH * npix + p] / n;
        if (out.alpha) out.alpha[o] = acc[(int64_t)FW_ALPHA * npix + p] / n;
    }
}

}  // namespace tk
