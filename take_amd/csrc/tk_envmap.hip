// tk_envmap.hip — a new environment map for a resident scene (include/take_hip.h: take_hip_scene_set_envmap*; DESIGN.md
// §4o), the test hook that reads a side's map back (take_hip_debug_env_tables*), and the only unit that compiles the
// kernels of tk_envmap.h.  The build: the image in device memory, ONE pass that converts it for every resident side and
// leaves the rows' prefix sums in scratch (k_env_weigh_scan), the marginal CDF on the host from the h downloaded row
// sums, then per side the conditional CDF (k_env_conditional) and both guide tables (k_env_guides) — all into buffers of
// a stage per side, which commit() swaps in only when every side has succeeded.  Everything runs on the default stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "take_hip.h"
#include "tk_scene_handle.h"
#include "tk_envmap.h"

using namespace tk;
using namespace tk_host;

namespace {

// what the call refuses without looking at a scene or a device
int check_envmap_args(const TakeScene *ts, const TakeEnvImage *im, const double *scale3) {
    if (!ts || !im || !im->data) return fail(TAKE_E_INVALID, "null argument");
    if (im->width <= 0 || im->height <= 0) return fail(TAKE_E_INVALID, "width and height must be positive");
    if (im->real != TAKE_PRECISION_F32 && im->real != TAKE_PRECISION_F64) return fail(TAKE_E_INVALID, "unknown real: the texels are TAKE_PRECISION_F32 or TAKE_PRECISION_F64");
    if (im->flags & ~TAKE_MESH_DEVICE_ARRAYS) return fail(TAKE_E_INVALID, "unknown flag bits");
    if (scale3 && !(std::isfinite(scale3[0]) && std::isfinite(scale3[1]) && std::isfinite(scale3[2]))) return fail(TAKE_E_INVALID, "the scale must be finite");
    return TAKE_OK;
}

// TAKE_HIP_VERBOSE=1: every kernel of the build between two events, printed to stderr once the build has completed
struct KernelClock {
    bool on = std::getenv("TAKE_HIP_VERBOSE") != nullptr;
    EventPool events;
    std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> spans;
    template <class F> void run(const std::string &name, F &&launch) {
        hipEvent_t a = on ? events.get() : nullptr, b = on ? events.get() : nullptr;
        if (a && b) (void)hipEventRecord(a, nullptr);
        launch();
        if (a && b) (void)hipEventRecord(b, nullptr), spans.push_back({name, {a, b}});
    }
    void report() {  // (after the device has been waited for)
        for (const auto &s : spans) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, s.second.first, s.second.second) == hipSuccess) std::fprintf(stderr, "[take_hip] set_envmap: %-28s %8.3f ms\n", s.first.c_str(), ms);
        }
    }
};

// what the sides of a scene share: the map's size, its guide sizes, the prefix sums and row sums in double (device),
// the marginal CDF in double (host)
struct EnvShared {
    int w = 0, h = 0, gm = 1, gc = 1;
    DevBuf<double> prefix, row_sum;
    std::vector<double> marginal;
};

// One side's new map, built aside.  moved: the dimensions changed — texels is the side's whole new texel array and
// images its new table; else texels is the image alone, copied over the old one by commit().
template <class R> struct EnvStage {
    int image = -1;
    bool moved = false, new_lights = false;
    DevBuf<R> texels;
    R *image_texels = nullptr;  // where the image's texels go, in `texels`
    std::vector<ImageInfo> host_images;
    DevBuf<ImageInfo> images;
    DevBuf<R> marginal, conditional;
    DevBuf<int32_t> guide_m, guide_c;
    std::vector<LightRec<R>> host_lights;
    DevBuf<LightRec<R>> lights;
    EnvMap<R> env{};

    // the texel array (with the other images' texels copied), the image table, the record, the light records
    int prepare(const SceneT<R> &sc, const EnvShared &s, const double *scale3) {
        const char *nomem = "out of device memory for the environment map's texels";
        env = sc.host.env;
        for (size_t i = 0; i < sc.host.images.size(); i++)
            if (sc.host.images[i].offset == env.texel0) image = (int)i;
        if (image < 0) return fail(TAKE_E_INVALID, "unsupported: the scene does not know which image its environment map is");
        const ImageInfo old = sc.host.images[image];
        const int64_t n_old = (int64_t)old.width * old.height, n_new = (int64_t)s.w * s.h;
        moved = old.width != s.w || old.height != s.h;
        if (moved) {
            host_images = sc.host.images;
            host_images[image].width = s.w, host_images[image].height = s.h;
            for (size_t i = (size_t)image + 1; i < host_images.size(); i++) host_images[i].offset += n_new - n_old;
            const size_t before = 3 * (size_t)old.offset, after = sc.texels.n - 3 * (size_t)(old.offset + n_old);
            if (texels.alloc(before + 3 * (size_t)n_new + after) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
            if (before) HIP_TRY(hipMemcpy(texels.p, sc.texels.p, before * sizeof(R), hipMemcpyDeviceToDevice));
            if (after) HIP_TRY(hipMemcpy(texels.p + before + 3 * (size_t)n_new, sc.texels.p + before + 3 * (size_t)n_old, after * sizeof(R), hipMemcpyDeviceToDevice));
            if (images.upload(host_images) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
            image_texels = texels.p + before;
        } else {
            if (texels.alloc(3 * (size_t)n_new) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
            image_texels = texels.p;
        }
        env.width = s.w, env.height = s.h, env.n_guide_m = s.gm, env.n_guide_c = s.gc;
        if (scale3) {
            host_lights = sc.host.lights;
            for (int a = 0; a < 3; a++) env.scale[a] = R(scale3[a]), host_lights[env.light].intensity[a] = R(scale3[a]);
            if (lights.upload(host_lights) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the light records");
            new_lights = true;
        }
        return TAKE_OK;
    }
    // the side's tables from the shared doubles: the marginal rounded and uploaded, the conditional CDF and both guides
    // made on the device, the guides searching this side's own rounded CDFs
    int tables(const EnvShared &s, KernelClock &clock) {
        const char *nomem = "out of device memory for the environment map's tables";
        const std::string real = sizeof(R) == 4 ? "<f32>" : "<f64>";
        const std::vector<R> m(s.marginal.begin(), s.marginal.end());
        if (marginal.upload(m) != hipSuccess || conditional.alloc((size_t)s.h * ((size_t)s.w + 1)) != hipSuccess ||
            guide_m.alloc((size_t)s.gm + 1) != hipSuccess || guide_c.alloc((size_t)s.h * ((size_t)s.gc + 1)) != hipSuccess)
            return fail(TAKE_E_NOMEM, nomem);
        auto grid = [](int64_t lanes, int rows) { return dim3((unsigned)((lanes + em::BLOCK - 1) / em::BLOCK), (unsigned)std::min(rows, em::MAX_GRID_Y)); };
        clock.run("k_env_conditional" + real, [&] {
            hipLaunchKernelGGL((em::k_env_conditional<R>), grid((int64_t)s.w + 1, s.h), dim3(em::BLOCK), 0, nullptr, (const double *)s.prefix.p, (const double *)s.row_sum.p, s.w, s.h, conditional.p);
        });
        clock.run("k_env_guides" + real + " marginal", [&] {
            hipLaunchKernelGGL((em::k_env_guides<R>), grid((int64_t)s.gm + 1, 1), dim3(em::BLOCK), 0, nullptr, (const R *)marginal.p, 1, s.h, s.gm, guide_m.p);
        });
        clock.run("k_env_guides" + real + " conditional", [&] {
            hipLaunchKernelGGL((em::k_env_guides<R>), grid((int64_t)s.gc + 1, s.h), dim3(em::BLOCK), 0, nullptr, (const R *)conditional.p, s.h, s.w, s.gc, guide_c.p);
        });
        HIP_TRY(hipGetLastError());
        return TAKE_OK;
    }
    // allocates nothing: moves, and with unchanged dimensions one device-to-device copy over the old texels, which
    // fails only with a lost device (first, so that nothing else has changed then)
    int commit(SceneT<R> &sc) {
        if (!moved) HIP_TRY(hipMemcpy(sc.texels.p + 3 * (size_t)env.texel0, texels.p, texels.bytes(), hipMemcpyDeviceToDevice));
        if (moved) sc.texels = std::move(texels), sc.images = std::move(images), sc.host.images = std::move(host_images);
        sc.env_marginal = std::move(marginal), sc.env_conditional = std::move(conditional);
        sc.env_guide_m = std::move(guide_m), sc.env_guide_c = std::move(guide_c);
        if (new_lights) sc.lights = std::move(lights), sc.host.lights = std::move(host_lights);
        // (the host's copies of creation's tables would be stale: nothing reads them once a scene is resident)
        sc.host.env_marginal = {}, sc.host.env_conditional = {}, sc.host.env_guide_m = {}, sc.host.env_guide_c = {};
        sc.host.env = env, sc.dev.env = env;
        sc.bind();
        return TAKE_OK;
    }
};

int set_envmap(TakeScene *ts, const TakeEnvImage *im, const double *scale3, void *stream) {
    if (int rc = check_envmap_args(ts, im, scale3)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    if (on_primary(ts, [](const auto &sc, const auto &) { return sc.host.env.light < 0; })) return fail(TAKE_E_INVALID, "no environment map: the scene has no environment-map light");
    // (the build runs on the default stream, as scene_create's does: first whatever `stream` still has to write into the texels)
    if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    try {
        KernelClock clock;
        EnvShared s;
        s.w = im->width, s.h = im->height;
        env_guide_sizes(s.w, s.h, s.gm, s.gc);
        struct { EnvStage<double> d; EnvStage<float> f; } stages;  // (sides named as the scene's: for_each_side pairs them)
        if (int rc = for_each_side(ts, [&](const auto &sc, auto &stage) { return stage.prepare(sc, s, scale3); }, &stages)) return rc;

        // the image in device memory, the row weights from the host's sin
        const char *nomem = "out of device memory for the environment map's build";
        const size_t n_in = 3 * (size_t)s.w * (size_t)s.h, in_bytes = n_in * (im->real == TAKE_PRECISION_F64 ? 8 : 4);
        DevBuf<char> staged;
        const void *d_in = im->data;
        if (!(im->flags & TAKE_MESH_DEVICE_ARRAYS)) {
            if (staged.alloc(in_bytes) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
            PinnedUploads up;
            if (up.copy(staged.p, im->data, in_bytes) != hipSuccess || up.finish() != hipSuccess) return fail(TAKE_E_DEVICE, "environment map upload failed");
            d_in = staged.p;
        }
        const double PI_D = 3.14159265358979323846;
        std::vector<double> wy((size_t)s.h);
        for (int y = 0; y < s.h; y++) wy[y] = std::sin(PI_D * (y + 0.5) / s.h);
        DevBuf<double> d_wy;
        if (d_wy.upload(wy) != hipSuccess || s.prefix.alloc((size_t)s.w * (size_t)s.h) != hipSuccess || s.row_sum.alloc((size_t)s.h) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);

        // convert for every side, weigh, scan the rows
        float *tex_f = has_side(ts, TAKE_PRECISION_F32) ? stages.f.image_texels : nullptr;
        double *tex_d = has_side(ts, TAKE_PRECISION_F64) ? stages.d.image_texels : nullptr;
        const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)s.h + em::ROWS - 1) / em::ROWS, 1 << 20);
        clock.run("k_env_weigh_scan", [&] {
            with_real(im->real, [&](auto tag) {
                using T = decltype(tag);
                hipLaunchKernelGGL((em::k_env_weigh_scan<T>), dim3(blocks), dim3(em::BLOCK), 0, nullptr, (const T *)d_in, s.w, s.h, (const double *)d_wy.p, tex_f, tex_d, s.prefix.p, s.row_sum.p);
                return 0;
            });
        });
        HIP_TRY(hipGetLastError());

        // the marginal CDF: h serial adds in row order, on the host from the downloaded row sums
        std::vector<double> row_sum((size_t)s.h);
        HIP_TRY(hipMemcpy(row_sum.data(), s.row_sum.p, s.row_sum.bytes(), hipMemcpyDeviceToHost));
        s.marginal.assign((size_t)s.h + 1, 0.0);
        if (!em::marginal_cdf(row_sum.data(), s.h, s.marginal.data())) return fail(TAKE_E_INVALID, "environment map: no positive luminance");

        if (int rc = for_each_side(ts, [&](const auto &, auto &stage) { return stage.tables(s, clock); }, &stages)) return rc;
        HIP_TRY(hipDeviceSynchronize());
        if (clock.on) clock.report();
        ts->acc_samples = 0, ts->acc_restart_needed = true;
        return for_each_side(ts, [](auto &sc, auto &stage) { return stage.commit(sc); }, &stages);
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while building the environment map");
    }
}

template <class R> int debug_env_tables_info(const SceneT<R> &sc, TakeDebugEnvTablesInfo &o) {
    const EnvMap<R> &e = sc.dev.env;
    if (e.light < 0) return fail(TAKE_E_INVALID, "no environment map: the scene has no environment-map light");
    o = TakeDebugEnvTablesInfo{};
    o.width = e.width, o.height = e.height, o.n_guide_m = e.n_guide_m, o.n_guide_c = e.n_guide_c;
    o.real_bytes = (int32_t)sizeof(R), o.n_images = (int32_t)sc.images.n, o.texel0 = e.texel0;
    LightRec<R> rec;
    HIP_TRY(hipMemcpy(&rec, sc.dev.lights + e.light, sizeof rec, hipMemcpyDeviceToHost));
    for (int a = 0; a < 3; a++) o.scale[a] = (double)e.scale[a], o.intensity[a] = (double)rec.intensity[a];
    return TAKE_OK;
}
template <class R> int debug_env_tables_copy(const SceneT<R> &sc, void *marginal, void *conditional, int32_t *guide_m, int32_t *guide_c, void *texels, void *images) {
    const EnvMap<R> &e = sc.dev.env;
    if (e.light < 0) return fail(TAKE_E_INVALID, "no environment map: the scene has no environment-map light");
    const size_t w = (size_t)e.width, h = (size_t)e.height;
    HIP_TRY(hipMemcpy(marginal, e.marginal, (h + 1) * sizeof(R), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(conditional, e.conditional, h * (w + 1) * sizeof(R), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(guide_m, e.guide_m, ((size_t)e.n_guide_m + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(guide_c, e.guide_c, h * ((size_t)e.n_guide_c + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(texels, sc.dev.texels + 3 * (size_t)e.texel0, 3 * w * h * sizeof(R), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(images, sc.dev.images, sc.images.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}

}  // namespace

extern "C" {

int take_hip_scene_set_envmap(TakeScene *ts, const TakeEnvImage *image, const double *scale3) { return set_envmap(ts, image, scale3, nullptr); }
int take_hip_scene_set_envmap_device(TakeScene *ts, const TakeEnvImage *image, const double *scale3, void *stream) { return set_envmap(ts, image, scale3, stream); }

// ------------------------------------------------------------------------------------------------ test hook: the resident map
int take_hip_debug_env_tables_info(const TakeScene *ts, int32_t side, TakeDebugEnvTablesInfo *info) {
    if (!ts || !info) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    if (!has_side(ts, side)) return fail(TAKE_E_INVALID, "the scene has no such side");
    TAKE_ON_DEVICE(ts);
    HIP_TRY(hipDeviceSynchronize());
    return on_side(ts, side, [&](const auto &sc) { return debug_env_tables_info(sc, *info); });
}
int take_hip_debug_env_tables(const TakeScene *ts, int32_t side, void *marginal, void *conditional, int32_t *guide_m, int32_t *guide_c, void *texels, void *images) {
    if (!ts || !marginal || !conditional || !guide_m || !guide_c || !texels || !images) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    if (!has_side(ts, side)) return fail(TAKE_E_INVALID, "the scene has no such side");
    TAKE_ON_DEVICE(ts);
    HIP_TRY(hipDeviceSynchronize());
    return on_side(ts, side, [&](const auto &sc) { return debug_env_tables_copy(sc, marginal, conditional, guide_m, guide_c, texels, images); });
}

}  // extern "C"
