// tk_host.h — host plumbing shared by the library's units, tk_api.hip, tk_scene_update.hip, tk_create.hip and
// tk_group.hip (the C entry points that render and that change a scene, scene creation, groups), tk_build.hip (the device LBVH build), tk_render.hip (rendering, trace hooks),
// tk_mesh.hip (mesh ingest), tk_denoise.hip (the image-space denoiser), tk_display.hip (the display transform),
// tk_bloom.hip (its bloom and the image workspace), tk_envmap.hip (a new environment map for a resident scene),
// tk_shading_update.hip (its new materials and light intensities) and tk_skin.hip (rigs: skinning and morph targets): the error string, fault injection, pinned uploads, the owning device buffer, the staged planes of the host twins, the
// dispatch on a precision, the check of a plane's size and precision.  (The scene handle all but tk_mesh.hip and
// tk_display.hip share is tk_scene_handle.h.)
// Everything here has external linkage (inline, in a named namespace): the units share ONE error string (what
// take_hip_last_error returns) and ONE TAKE_HIP_FAIL_ALLOC counter.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "take_hip.h"

namespace tk_host {

inline thread_local std::string g_error;
inline int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(TAKE_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));             \
    } while (0)

// Fault injection for the allocation-failure tests (tests/test_gpu_robustness.py): TAKE_HIP_FAIL_ALLOC=<k> makes the
// k-th device allocation after the variable was (re)set fail with hipErrorOutOfMemory.  A real out-of-memory cannot
// be provoked reliably from a test: the driver over-commits, a 300 GB request on a 288 GB device succeeded.
// (allocations happen on several host threads at once — one per shard of a scene group — hence the lock)
inline bool inject_alloc_failure() {
    static std::mutex mu;
    static std::string seen;
    static long calls = 0;
    const char *e = std::getenv("TAKE_HIP_FAIL_ALLOC");
    std::lock_guard<std::mutex> lock(mu);
    if (!e || !*e) {
        seen.clear();
        return false;
    }
    if (seen != e) seen = e, calls = 0;
    return ++calls == std::atol(e);
}

// Host -> device copies of the caller's large arrays (mesh positions, shape arrays) for the device-side scene build
// (SURVEY.md §8(f)2): the pages are pinned IN PLACE (hipHostRegister) so that the DMA engine reads the caller's memory
// directly — no bounce through the runtime's staging buffers — and the copies of all arrays are in flight together;
// the registrations are dropped once the stream has drained.  Arrays below 4 MiB, and memory that cannot be
// registered, take the ordinary pageable path.  TAKE_HIP_PINNED_UPLOAD=0 turns the registration off (A/B runs).
struct PinnedUploads {
    hipStream_t stream = nullptr;
    std::vector<void *> regs;
    size_t pinned_bytes = 0, plain_bytes = 0;
    bool enabled = !(std::getenv("TAKE_HIP_PINNED_UPLOAD") && std::atoi(std::getenv("TAKE_HIP_PINNED_UPLOAD")) == 0);
    hipError_t copy(void *dst, const void *src, size_t bytes) {
        if (bytes == 0) return hipSuccess;
        if (enabled && bytes >= ((size_t)4 << 20)) {
            if (hipHostRegister(const_cast<void *>(src), bytes, hipHostRegisterDefault) == hipSuccess) {
                regs.push_back(const_cast<void *>(src));
                pinned_bytes += bytes;
            } else {
                (void)hipGetLastError();  // (already registered, read-only mapping, ...): pageable copy
                plain_bytes += bytes;
            }
        } else {
            plain_bytes += bytes;
        }
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
    }
    hipError_t finish() {
        const hipError_t e = hipStreamSynchronize(stream);
        for (void *p : regs) (void)hipHostUnregister(p);
        regs.clear();
        return e;
    }
    ~PinnedUploads() { (void)finish(); }
};

// A device array that owns its allocation: freed when it goes out of scope or is moved over, handed on with detach().
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p, n = o.n;
            o.p = nullptr, o.n = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count) {
        release();  // p = nullptr, n = 0: the state a failed allocation leaves behind
        if (count == 0) return hipSuccess;
        const hipError_t e = inject_alloc_failure() ? hipErrorOutOfMemory : hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();  // the error is reported through the return value, not left sticky
            return e;
        }
        n = count;
        return hipSuccess;
    }
    hipError_t upload(const std::vector<T> &v) {
        hipError_t e = alloc(v.size());
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    // the allocation, no longer owned (it goes into a caller's TakeMesh)
    T *detach() {
        T *q = p;
        p = nullptr, n = 0;
        return q;
    }
    size_t bytes() const { return n * sizeof(T); }
};

// The per-pixel planes of a host twin (take_hip_denoise, take_hip_render_features, ...), staged in device memory for
// the call's _device twin.  A plane: where it is uploaded from and where it is downloaded to, either null = not that
// way; both null = absent (an optional plane the caller left out): never allocated, its device pointer is null.
struct HostPlane {
    const void *from;
    void *to;
    size_t bytes_per_pixel;
};
inline HostPlane plane_in(const void *from, size_t bytes_per_pixel) { return {from, nullptr, bytes_per_pixel}; }
inline HostPlane plane_out(void *to, size_t bytes_per_pixel) { return {nullptr, to, bytes_per_pixel}; }
// an input the device call changes in place, then copied out: without the input there is no plane, whatever `to` is
inline HostPlane plane_inout(const void *from, void *to, size_t bytes_per_pixel) { return {from, from ? to : nullptr, bytes_per_pixel}; }
template <int N> struct StagedPlanes {
    HostPlane plane[N];
    DevBuf<char> dev[N];
    // the present planes for npix pixels, in the order of `plane` (npix = 0: none); nomem: the TAKE_E_NOMEM message
    int alloc(size_t npix, const char *nomem) {
        for (int k = 0; k < N; k++)
            if ((plane[k].from || plane[k].to) && dev[k].alloc(npix * plane[k].bytes_per_pixel) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
        return TAKE_OK;
    }
    int upload() {
        for (int k = 0; k < N; k++)
            if (plane[k].from && dev[k].p) HIP_TRY(hipMemcpy(dev[k].p, plane[k].from, dev[k].bytes(), hipMemcpyHostToDevice));
        return TAKE_OK;
    }
    int download() {
        for (int k = 0; k < N; k++)
            if (plane[k].to && dev[k].p) HIP_TRY(hipMemcpy(plane[k].to, dev[k].p, dev[k].bytes(), hipMemcpyDeviceToHost));
        return TAKE_OK;
    }
    void *operator[](int k) const { return dev[k].p; }
};

// f(R{}) with R = float or double: the Real of a TAKE_PRECISION_F32 / _F64 value (checked by the caller)
template <class F> auto with_real(int32_t precision, F &&f) { return precision == TAKE_PRECISION_F64 ? f(double{}) : f(float{}); }

// what every scene-free image-space call (tk_denoise.hip, tk_display.hip) refuses of its planes' size and precision
inline int check_image(int32_t precision, int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return fail(TAKE_E_INVALID, "width and height must be positive");
    if (precision != TAKE_PRECISION_F32 && precision != TAKE_PRECISION_F64) return fail(TAKE_E_INVALID, "unknown precision");
    return TAKE_OK;
}

// A rig seen from another unit (tk_subdiv.hip poses the rig a cage is bound with; defined in tk_skin.hip): what a pose
// call refuses without a device, `who` in front of the message; the rig's device and vertex count.
int rig_check_pose(const TakeRig *rig, const TakeRigPose *pose, const std::string &who);
void rig_shape(const TakeRig *rig, int *device, int64_t *n_vertices);

// A subdivision handle seen from another unit (tk_displace.hip displaces the surface a cage is refined to; defined in
// tk_subdiv.hip, the only unit that compiles the kernels of tk_subdiv.h): the handle's device and vertex counts;
// one binding's cage — host or device positions, or a rig that is posed first — refined into the handle's own buffers on
// the default stream, as take_hip_scene_subdivide_meshes refines it (out_n null: no normals) -> where the results are;
// and the two normal launches over any mesh in device memory — face normals into face_n (n_faces x 3), then every
// vertex's normal over its row of faces into out_n — on `stream`, without waiting; `between`, unless null, is recorded
// between the two.
void subdiv_shape(const TakeSubdiv *subdiv, int *device, int64_t *cage_vertices, int64_t *n_vertices);
int subdiv_refine_own(TakeSubdiv *subdiv, const double *cage_positions, bool on_device, TakeRig *rig, const TakeRigPose *pose, bool normals, const double **d_positions,
                      const double **d_normals);
void subdiv_launch_normals(const int32_t *indices, const int32_t *face_start, const int32_t *faces, const double *positions, int64_t n_faces, int64_t n_vertices,
                           double *face_n, double *out_n, hipStream_t stream, hipEvent_t between);

inline int check_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(TAKE_E_NO_GPU, "no HIP device visible: libtake_hip has no CPU path");
    return n;
}

}  // namespace tk_host
