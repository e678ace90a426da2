// tk_group.hip — scene groups (take_hip_group_*): one scene per GPU, prepared and built once and replicated peer to
// peer; every shard renders its strips on its own device and the rows are assembled on the first.  The one kernel
// here is the row scatter.  Rendering itself is tk_render.hip, reached through tk_scene_handle.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "take_hip.h"
#include "tk_scene_handle.h"

using namespace tk;
using namespace tk_host;

struct TakeSceneGroup {
    std::vector<TakeScene *> scenes;        // one per shard, each on its device
    std::vector<DevBuf<char>> staging;      // on the first device: shard k's compact rows (k > 0), copied peer to peer
    std::vector<DevBuf<int32_t>> d_rows;    // on the first device: image row of each compact row of shard k
    std::vector<int> n_rows;
    DevBuf<char> d_full;                    // on the first device: the assembled image (take_hip_group_render)
    int width = 0, height = 0;
    bool f64 = false;
    ~TakeSceneGroup() {
        // the group's buffers are freed here, in the guard's scope: freed as members, they would go after the guard
        // (they exist only once the first shard does)
        if (!scenes.empty()) {
            DeviceGuard guard(scenes[0]->device);
            staging.clear(), d_rows.clear(), d_full = DevBuf<char>();
        }
        for (TakeScene *ts : scenes) take_hip_scene_destroy(ts);
    }
};

namespace {
// A replica of `src` on `device`: every device array is copied peer to peer (xGMI between the GPUs of a node), the
// small host tables by value — the scene is prepared and its tree built ONCE per group, whichever builder made it.
template <class T> int peer_copy(DevBuf<T> &dst, int dst_dev, const DevBuf<T> &src, int src_dev) {
    if (dst.alloc(src.n) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for a scene replica");
    if (src.n && hipMemcpyPeer(dst.p, dst_dev, src.p, src_dev, src.bytes()) != hipSuccess)
        return fail(TAKE_E_DEVICE, "hipMemcpyPeer of a scene array failed");
    return TAKE_OK;
}
template <class R> int replicate_t(const SceneT<R> &a, int a_dev, SceneT<R> &b, int b_dev, int b_cus) {
    int rc = TAKE_OK;
    SceneT<R>::for_each_array([&](auto &dst, const auto &src) { if (!rc) rc = peer_copy(dst, b_dev, src, a_dev); }, b, a);
    if (rc) return rc;
    b.host = a.host;  // (the camera, counts and small tables: upload_scene dropped the large vectors)
    b.dev = a.dev;    // the plain values; then the pointers of this device
    b.bind();
    // the persistent trace grid of THIS device: blocks per CU are a property of the kernels (the same code object on
    // every device), the CU count is the replica device's own
    b.built_on_device = a.built_on_device, b.trace = a.trace, b.trace_state.blocks_per_cu = a.trace_state.blocks_per_cu;
    const hipError_t e = alloc_trace_state(b, b_cus);
    if (e == hipErrorOutOfMemory) return fail(TAKE_E_NOMEM, "out of device memory for a scene replica");
    HIP_TRY(e);
    return TAKE_OK;
}
// -> a new scene handle on `device` (made current for the call), equal to `src`
int replicate_scene(const TakeScene *src, int device, TakeScene **out) {
    *out = nullptr;
    DeviceGuard guard(device);  // (declared before the replica: a failed one is freed with its device current)
    std::unique_ptr<TakeScene> ts(new (std::nothrow) TakeScene());
    if (!ts) return fail(TAKE_E_NOMEM, "out of host memory");
    ts->precision = src->precision, ts->device = device, ts->num_cus = src->num_cus, ts->instrumentation = 0;
    ts->n_placements = src->n_placements;
    ts->lens = src->lens, ts->lens_focus = src->lens_focus, ts->look_distance = src->look_distance, ts->camera = src->camera;  // (the camera records are copied with the sides)
    if (!guard.ok) return fail(TAKE_E_DEVICE, "cannot make the replica's device current");
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ts->num_cus = cus;
    (void)hipGetLastError();
    // every side of src (a) into the same side of the replica (b: for_each_side's `more`), in take_hip_scene_create's order
    const int rc = for_each_side(src, [&](const auto &a, auto &b) { return replicate_t(a, src->device, b, device, ts->num_cus); }, ts.get());
    if (rc) return rc;
    const hipError_t e = on_primary(ts.get(), [](auto &, auto &work) { return work.create(); });  // the replica's own workspace
    if (e == hipErrorOutOfMemory) return fail(TAKE_E_NOMEM, "out of device memory for a scene replica");
    HIP_TRY(e);
    *out = ts.release();
    return TAKE_OK;
}

constexpr int BLOCK = 256;  // threads per block of k_place_rows
// compact rows of one shard -> their rows of the full image
template <class R>
__global__ void __launch_bounds__(BLOCK) k_place_rows(const R *__restrict__ src, const int32_t *__restrict__ rows, int n_rows,
                                                      int row_words, R *dst) {
    const int64_t total = (int64_t)n_rows * row_words;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLOCK) {
        const int r = (int)(i / row_words), c = (int)(i % row_words);
        dst[(int64_t)rows[r] * row_words + c] = src[i];
    }
}

int group_render(TakeSceneGroup *g, const TakeRenderOpts &opts, void *d_out) {
    const int n = (int)g->scenes.size();
    const size_t esz = g->f64 ? 8 : 4;
    const int row_words = g->width * 3;
    // every shard renders its strips on its own device, from its own host thread
    std::vector<int> rc(n, TAKE_OK);
    std::vector<std::string> err(n);
    std::vector<std::thread> pool;
    for (int k = 0; k < n; k++)
        pool.emplace_back([&, k] {
            TakeScene *ts = g->scenes[k];
            TakeRenderOpts o = opts;
            o.strip_first = k, o.strip_stride = n;
            if (g->n_rows[k] == 0) return;
            DeviceGuard guard(ts->device);
            if (!guard.ok) {
                rc[k] = TAKE_E_DEVICE, err[k] = "cannot make the shard's device current";
                return;
            }
            const void *rows = nullptr;
            int r = render_scene_to_out(ts, o, (int64_t)g->n_rows[k] * g->width, rows);
            if (!r && k > 0) {  // the one exchange: this shard's rows to the first device
                const hipError_t e = hipMemcpyPeer(g->staging[k].p, g->scenes[0]->device, rows, ts->device, (size_t)g->n_rows[k] * row_words * esz);
                if (e != hipSuccess) r = TAKE_E_DEVICE, g_error = std::string("hipMemcpyPeer: ") + hipGetErrorString(e);
            }
            rc[k] = r;
            if (r) err[k] = g_error;  // g_error is thread-local: hand the message to the caller's thread
        });
    for (auto &t : pool) t.join();
    for (int k = 0; k < n; k++)
        if (rc[k]) return fail(rc[k], "shard " + std::to_string(k) + ": " + err[k]);
    // assemble on the first device
    DeviceGuard guard(g->scenes[0]->device);
    if (!guard.ok) return fail(TAKE_E_DEVICE, "cannot make the first device current");
    on_primary(g->scenes[0], [&](auto &, auto &work0) {
        using R = std::remove_pointer_t<decltype(work0.out.p)>;
        for (int k = 0; k < n; k++) {
            if (g->n_rows[k] == 0) continue;
            const R *src = k == 0 ? work0.out.p : (const R *)g->staging[k].p;
            const int64_t total = (int64_t)g->n_rows[k] * row_words;
            const dim3 grid((unsigned)std::min<int64_t>((total + BLOCK - 1) / BLOCK, 4096));
            hipLaunchKernelGGL((k_place_rows<R>), grid, dim3(BLOCK), 0, nullptr, src, g->d_rows[k].p, g->n_rows[k], row_words, (R *)d_out);
        }
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return TAKE_OK;
}
}  // namespace

extern "C" {

int take_hip_group_create(const TakeSceneDesc *desc, const TakeBuildOpts *opts, int32_t n_gpus, const int32_t *devices,
                          TakeSceneGroup **out) {
    if (!desc || !out) return fail(TAKE_E_INVALID, "null argument");
    *out = nullptr;
    const int nd = check_device();
    if (nd < 0) return nd;
    if (n_gpus <= 0 || n_gpus > 64) return fail(TAKE_E_INVALID, "n_gpus must be in 1..64");
    for (int k = 0; k < n_gpus; k++) {
        const int dev = devices ? devices[k] : k;
        if (dev < 0 || dev >= nd) return fail(TAKE_E_INVALID, "device " + std::to_string(dev) + " of shard " + std::to_string(k) + " is not visible (" + std::to_string(nd) + " devices)");
    }
    std::unique_ptr<TakeSceneGroup> g(new (std::nothrow) TakeSceneGroup());
    if (!g) return fail(TAKE_E_NOMEM, "out of host memory");
    int prev = 0;
    (void)hipGetDevice(&prev);
    int rc = TAKE_OK;
    for (int k = 0; k < n_gpus && !rc; k++) {
        const int dev = devices ? devices[k] : k;
        if (hipSetDevice(dev) != hipSuccess) {
            rc = fail(TAKE_E_DEVICE, "hipSetDevice failed");
            break;
        }
        TakeScene *ts = nullptr;
        // the first shard prepares and builds the scene; the others are peer-to-peer copies of its device arrays
        rc = k == 0 ? take_hip_scene_create(desc, opts, &ts) : replicate_scene(g->scenes[0], dev, &ts);
        if (!rc) g->scenes.push_back(ts);
    }
    if (!rc) {
        for (TakeScene *x : g->scenes) {  // shards that share a device share its free memory
            int share = 0;
            for (TakeScene *y : g->scenes) share += y->device == x->device;
            x->mem_share = share;
        }
        TakeScene *t0 = g->scenes[0];
        g->f64 = t0->f64(), g->width = t0->width(), g->height = t0->height();
        const size_t esz = g->f64 ? 8 : 4;
        g->staging.resize(n_gpus), g->d_rows.resize(n_gpus), g->n_rows.assign(n_gpus, 0);
        if (hipSetDevice(t0->device) != hipSuccess) rc = fail(TAKE_E_DEVICE, "hipSetDevice failed");
        for (int k = 0; k < n_gpus && !rc; k++) {
            std::vector<int32_t> rows((size_t)g->height);
            const int nr = rows_of(g->height, k, n_gpus, rows.data());
            rows.resize(nr);
            g->n_rows[k] = nr;
            if (nr == 0) continue;
            if (g->d_rows[k].upload(rows) != hipSuccess || (k > 0 && g->staging[k].alloc((size_t)nr * g->width * 3 * esz) != hipSuccess))
                rc = fail(TAKE_E_NOMEM, "out of device memory for the strip staging buffers");
            if (!rc && k > 0 && g->scenes[k]->device != t0->device) {
                // direct peer access if the fabric offers it (hipMemcpyPeer works either way)
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, t0->device, g->scenes[k]->device) == hipSuccess && can)
                    (void)hipDeviceEnablePeerAccess(g->scenes[k]->device, 0);
                (void)hipGetLastError();
            }
        }
    }
    (void)hipSetDevice(prev);
    if (rc) return rc;
    *out = g.release();
    return TAKE_OK;
}

int take_hip_group_destroy(TakeSceneGroup *g) {
    delete g;
    return TAKE_OK;
}
int take_hip_group_size(const TakeSceneGroup *g) { return g ? (int)g->scenes.size() : fail(TAKE_E_INVALID, "null group"); }

int take_hip_group_render_device(TakeSceneGroup *g, const TakeRenderOpts *opts, void *d_rgb_out) {
    if (!g || !opts || !d_rgb_out) return fail(TAKE_E_INVALID, "null argument");
    return group_render(g, *opts, d_rgb_out);
}

int take_hip_group_render(TakeSceneGroup *g, const TakeRenderOpts *opts, void *rgb_out_host) {
    if (!g || !opts || !rgb_out_host) return fail(TAKE_E_INVALID, "null argument");
    const size_t bytes = (size_t)g->width * g->height * 3 * (g->f64 ? 8 : 4);
    DeviceGuard guard(g->scenes[0]->device);
    if (!guard.ok) return fail(TAKE_E_DEVICE, "cannot make the first device current");
    if (!g->d_full.p && g->d_full.alloc(bytes) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the assembled image");
    const int rc = group_render(g, *opts, g->d_full.p);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(rgb_out_host, g->d_full.p, bytes, hipMemcpyDeviceToHost));
    return TAKE_OK;
}

int take_hip_group_get_counters(const TakeSceneGroup *g, int32_t k, TakeCounters *out) {
    if (!g || !out || k < 0 || k >= (int)g->scenes.size()) return fail(TAKE_E_INVALID, "bad argument");
    *out = g->scenes[k]->counters;
    return TAKE_OK;
}

}  // extern "C"
