// tk_rays.h — caller-supplied rays as a first-ray source of the wavefront path tracer, and its inverse: the scene's own
// camera rays handed to the caller (take_hip_render_rays*, take_hip_camera_rays*; contract: include/take_hip.h,
// specification: DESIGN.md §4n).  gfx950, wave64.
//
//   ray_to_path       a ray record (TakeRayF / TakeRayD) -> the initial path record of a slot: what generate_path_as
//                     writes, with origin and direction taken from the record instead of the camera
//   path_to_ray       the inverse: the path record generate_path has just written -> a ray record
//   k_generate_rays   one batch of caller rays -> path records + the identity extend queue (in front of the unchanged
//                     round loop, as k_generate, k_generate_lens and k_generate_list are)
//   k_export_rays     the path records of one batch -> ray records
//
// The two functions are TK_HD and written once, as tk_lens.h: the kernels run them on the device, tests/rays_host runs
// the same text on the host.  Of a ray record org and dir are read; tmin and tmax are not (PathIo keeps one tmin for
// all rays of a launch — the ray epsilon — and a camera ray's first segment is unbounded: so is a caller's).
#pragma once
#include <cstdint>

#include "tk_integrate.h"

namespace tk {

constexpr int32_t RAYS_NORMALIZE = 1;  // TAKE_RAYS_NORMALIZE

// the layout of TakeRayF (32 B) / TakeRayD (64 B)
template <class R> struct RayRec {
    R org[3], tmin, dir[3], tmax;
};

// The initial record of path `slot` for a caller's ray: generate_path_as with the ray given.  normalise: the direction
// goes through camera_dir's own normalize first (TAKE_RAYS_NORMALIZE); else it is taken as it is and has to be of unit
// length already — the shade rounds take cosines against it.
template <class R> TK_HD void ray_to_path(const RayRec<R> &ray, bool normalise, const PathState<R> &st, int64_t slot) {
    Vec3<R> d{ray.dir[0], ray.dir[1], ray.dir[2]};
    if (normalise) d = normalize(d);
    st.R_(S_OX, slot) = ray.org[0];
    st.R_(S_OY, slot) = ray.org[1];
    st.R_(S_OZ, slot) = ray.org[2];
    st.R_(S_DX, slot) = d.x;
    st.R_(S_DY, slot) = d.y;
    st.R_(S_DZ, slot) = d.z;
    st.R_(S_TX, slot) = R(1);
    st.R_(S_TY, slot) = R(1);
    st.R_(S_TZ, slot) = R(1);
    st.R_(S_LX, slot) = R(0);
    st.R_(S_LY, slot) = R(0);
    st.R_(S_LZ, slot) = R(0);
    st.I_(S_CTR, slot) = (int32_t)CAMERA_DRAWS;  // (counters 0 and 1 of the stream: left to the caller's own jitter)
    st.I_(S_FLAGS, slot) = 0;
    st.I_(S_OCC, slot) = -1;
    st.I_(S_CONV, slot) = 0;
}

// The ray of the path record generate_path has just written for `slot`, as the trace hooks take it: tmin = the ray
// epsilon the render would trace it with, tmax = +inf.
template <class R> TK_HD RayRec<R> path_to_ray(const PathState<R> &st, int64_t slot, R tmin) {
    return RayRec<R>{{st.R_(S_OX, slot), st.R_(S_OY, slot), st.R_(S_OZ, slot)}, tmin,
                     {st.R_(S_DX, slot), st.R_(S_DY, slot), st.R_(S_DZ, slot)}, Const<R>::inf()};
}

}  // namespace tk

#if defined(__HIPCC__)
#include "tk_kernels.h"

namespace tk {

// One ray record per lane as 16-byte vectors: two loads in f32, four in f64, instead of eight scalar ones (a request
// each per lane).  Inline asm as the shade kernels' record loads: written as C++ loads the compiler narrows them to
// the six words that are read.  p: 16-byte aligned (checked by the entry points).
template <class R> struct RayWords {
    union {
        uint4 q[sizeof(RayRec<R>) / 16];
        RayRec<R> r;
    };
    __device__ __forceinline__ RayWords() {}
};
__device__ __forceinline__ RayRec<float> load_ray(const RayRec<float> *p) {
    RayWords<float> w;
    asm volatile(
        "global_load_dwordx4 %0, %2, off\n\t"
        "global_load_dwordx4 %1, %2, off offset:16\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(w.q[0]), "=&v"(w.q[1])
        : "v"(p)
        : "memory");
    return w.r;
}
__device__ __forceinline__ RayRec<double> load_ray(const RayRec<double> *p) {
    RayWords<double> w;
    asm volatile(
        "global_load_dwordx4 %0, %4, off\n\t"
        "global_load_dwordx4 %1, %4, off offset:16\n\t"
        "global_load_dwordx4 %2, %4, off offset:32\n\t"
        "global_load_dwordx4 %3, %4, off offset:48\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(w.q[0]), "=&v"(w.q[1]), "=&v"(w.q[2]), "=&v"(w.q[3])
        : "v"(p)
        : "memory");
    return w.r;
}
template <class R> __device__ __forceinline__ void store_ray(RayRec<R> *p, const RayRec<R> &ray) {
    RayWords<R> w;
    w.r = ray;
    uint4 *out = (uint4 *)p;
#pragma unroll
    for (int c = 0; c < (int)(sizeof(RayRec<R>) / 16); c++) out[c] = w.q[c];
}

// The paths of one batch from the caller's rays: slot = s * n + i is sample s of the batch for ray (= texel) i.  It
// reads ray i of set `set0 + s` — set0: the batch's first sample counted from the call's first_sample, or < 0: one set
// serves every sample — and writes the slot's initial record and the identity extend queue.  inv_n = 1.0 / n
// (divmod_u31); n_slots = the batch's samples * n < 2^31.
template <class R>
__global__ void __launch_bounds__(BLOCK)
k_generate_rays(const RayRec<R> *__restrict__ rays, int64_t n, double inv_n, int64_t set0, int normalise, PathState<R> st, int32_t *queue, int64_t n_slots) {
    for (int64_t slot = (int64_t)blockIdx.x * BLOCK + threadIdx.x; slot < n_slots; slot += (int64_t)gridDim.x * BLOCK) {
        uint32_t s, i;
        divmod_u31((uint32_t)slot, (uint32_t)n, inv_n, s, i);
        const int64_t at = set0 < 0 ? (int64_t)i : (set0 + (int64_t)s) * n + (int64_t)i;
        ray_to_path(load_ray(rays + at), normalise != 0, st, slot);
        queue[slot] = (int32_t)slot;
    }
}

// The path records k_generate / k_generate_lens have just written for the n_slots slots of one batch -> ray records;
// out: the record of the batch's slot 0 (the host adds the batch's offset: the sets are sample-major, as the slots are)
template <class R>
__global__ void __launch_bounds__(BLOCK)
k_export_rays(PathState<R> st, RayRec<R> *out, int64_t n_slots, R tmin) {
    for (int64_t slot = (int64_t)blockIdx.x * BLOCK + threadIdx.x; slot < n_slots; slot += (int64_t)gridDim.x * BLOCK)
        store_ray(out + slot, path_to_ray(st, slot, tmin));
}

}  // namespace tk
#endif
