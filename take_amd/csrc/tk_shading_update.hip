// tk_shading_update.hip — new materials and new light intensities for a resident scene (include/take_hip.h:
// take_hip_scene_set_materials, take_hip_scene_set_light_intensities*), the test hook that reads a side's
// shading tables back (take_hip_debug_shading_tables*), and the only unit that compiles the kernels of
// tk_shading_update.h.  Everything that can fail — validation, allocations, uploads, the power kernel — happens on a
// stage per side; commit() swaps the buffers in only when every side has succeeded, and then launches the in-place retag
// of the primitive and placement records.  Everything runs on the default stream.
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
#include "tk_shading_update.h"

using namespace tk;
using namespace tk_host;

namespace {

const char *const RANGE_MESSAGE = "the range [first, first + count) lies outside the table";

// what the calls refuse of a range without looking at a scene or a device
int check_range_args(const void *ts, const void *values, int32_t first, int32_t count) {
    if (!ts || !values) return fail(TAKE_E_INVALID, "null argument");
    if (count <= 0) return fail(TAKE_E_INVALID, "count must be positive");
    if (first < 0 || first > INT32_MAX - count) return fail(TAKE_E_INVALID, RANGE_MESSAGE);
    return TAKE_OK;
}

// ------------------------------------------------------------------------------------------------ materials
// One side's new material table, built aside.  retag: some material of the range changes its effective tag — the
// records' tag bytes follow in commit(); else the table is all that changes.
template <class R> struct MaterialStage {
    std::vector<MaterialRec<R>> host_materials;
    DevBuf<MaterialRec<R>> materials;
    DevBuf<int32_t> tags;
    int n_material_tags = 0, single_tag = 0;
    uint32_t tag_mask = 0;
    bool retag = false;

    int prepare(const SceneT<R> &sc, const TakeMaterial *in, int32_t first, int32_t count, bool burley_lobes) {
        host_materials = sc.host.materials;
        for (int32_t k = 0; k < count; k++) {
            MaterialRec<R> rec{};
            const std::string err = material_record(in[k], first + k, (int)sc.host.images.size(), burley_lobes, rec);
            if (!err.empty()) return fail(TAKE_E_INVALID, err);
            retag = retag || rec.tag != host_materials[first + k].tag;
            host_materials[first + k] = rec;
        }
        material_tags_in_use(host_materials, n_material_tags, tag_mask, single_tag);
        if (materials.upload(host_materials) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the material table");
        if (retag) {
            std::vector<int32_t> t(host_materials.size());
            for (size_t i = 0; i < t.size(); i++) t[i] = host_materials[i].tag;
            if (tags.upload(t) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the material tags");
        }
        return TAKE_OK;
    }
    // allocates nothing: moves, then the retag in place — no render is in flight (every entry point returns after its
    // work has completed) — which fails only with a lost device
    int commit(SceneT<R> &sc) {
        sc.materials = std::move(materials), sc.host.materials = std::move(host_materials);
        sc.host.n_material_tags = n_material_tags, sc.host.tag_mask = tag_mask, sc.host.single_tag = single_tag;
        sc.bind();
        if (!retag) return TAKE_OK;
        const int32_t n_materials = (int32_t)sc.materials.n;
        // TAKE_HIP_VERBOSE=1: both kernels between events, printed to stderr once they have completed
        EventPool events;
        hipEvent_t ev[3] = {};
        if (std::getenv("TAKE_HIP_VERBOSE"))
            for (hipEvent_t &e : ev) e = events.get();
        const bool clocked = ev[0] && ev[1] && ev[2];
        if (clocked) (void)hipEventRecord(ev[0], nullptr);
        if (sc.prims.n)
            hipLaunchKernelGGL((su::k_retag_prims<R>), dim3((unsigned)su::blocks_for((int64_t)sc.prims.n)), dim3(su::BLOCK), 0, nullptr, sc.prims.p, (int64_t)sc.prims.n,
                               (const int32_t *)tags.p, n_materials);
        if (clocked) (void)hipEventRecord(ev[1], nullptr);
        if (sc.inst_shade.n)
            hipLaunchKernelGGL((su::k_retag_placements<R>), dim3((unsigned)su::blocks_for((int64_t)sc.inst_shade.n)), dim3(su::BLOCK), 0, nullptr, sc.inst_shade.p,
                               (int64_t)sc.inst_shade.n, (const int32_t *)tags.p, n_materials);
        if (clocked) (void)hipEventRecord(ev[2], nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());  // (the tags go with the stage)
        float ms[2] = {0, 0};
        if (clocked && hipEventElapsedTime(&ms[0], ev[0], ev[1]) == hipSuccess && hipEventElapsedTime(&ms[1], ev[1], ev[2]) == hipSuccess) {
            const char *real = sizeof(R) == 4 ? "<f32>" : "<f64>";
            std::fprintf(stderr, "[take_hip] set_materials: k_retag_prims%s %lld records %8.3f ms\n", real, (long long)sc.prims.n, ms[0]);
            std::fprintf(stderr, "[take_hip] set_materials: k_retag_placements%s %lld records %8.3f ms\n", real, (long long)sc.inst_shade.n, ms[1]);
        }
        return TAKE_OK;
    }
};

int set_materials(TakeScene *ts, const TakeMaterial *in, int32_t first, int32_t count) {
    if (int rc = check_range_args(ts, in, first, count)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    if ((int64_t)first + count > on_primary(ts, [](const auto &sc, const auto &) { return (int64_t)sc.host.materials.size(); })) return fail(TAKE_E_INVALID, RANGE_MESSAGE);
    try {
        HIP_TRY(hipDeviceSynchronize());
        return stage_then_commit<MaterialStage>(ts, [&](const auto &sc, auto &stage) { return stage.prepare(sc, in, first, count, ts->burley_lobes); });
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while building the material table");
    }
}

// ------------------------------------------------------------------------------------------------ light intensities
// One side's lights under the new intensities, built aside: the records (a device-to-device copy of the resident ones,
// the range's intensities written and their powers computed by k_light_power), both power tables from the host's
// serial pass, and — when the range holds the environment-map light — the map's scale.
template <class R> struct LightStage {
    std::vector<LightRec<R>> host_lights;
    std::vector<R> host_pmf, host_cdf;
    DevBuf<LightRec<R>> lights;
    DevBuf<R> power, light_pmf, light_cdf;
    EnvMap<R> env{};

    // d_rgb: 3 * count doubles in device memory; rgb: the same values on the host
    int prepare(const SceneT<R> &sc, const double *d_rgb, const double *rgb, int32_t first, int32_t count) {
        const char *nomem = "out of device memory for the light records";
        const size_t n = sc.lights.n;
        if (lights.alloc(n) != hipSuccess || power.alloc((size_t)count) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
        HIP_TRY(hipMemcpy(lights.p, sc.lights.p, sc.lights.bytes(), hipMemcpyDeviceToDevice));
        hipLaunchKernelGGL((su::k_light_power<R>), dim3((unsigned)su::blocks_for(count)), dim3(su::BLOCK), 0, nullptr, lights.p, first, (int64_t)count, d_rgb, power.p);
        HIP_TRY(hipGetLastError());
        std::vector<R> range_power((size_t)count);
        HIP_TRY(hipMemcpy(range_power.data(), power.p, power.bytes(), hipMemcpyDeviceToHost));
        // the host's copies, and the serial pass over ALL powers: the range's from the device, the others' as creation made them
        host_lights = sc.host.lights;
        env = sc.host.env;
        for (int32_t k = 0; k < count; k++)
            for (int a = 0; a < 3; a++) host_lights[first + k].intensity[a] = R(rgb[3 * (size_t)k + a]);
        if (env.light >= first && env.light < first + count)
            for (int a = 0; a < 3; a++) env.scale[a] = host_lights[env.light].intensity[a];
        host_pmf.resize(n);
        for (size_t i = 0; i < n; i++) host_pmf[i] = ((int64_t)i >= first && (int64_t)i < (int64_t)first + count) ? range_power[i - first] : su::light_power(host_lights[i]);
        su::light_tables_from_powers<R>(host_pmf, host_cdf);
        if (light_pmf.upload(host_pmf) != hipSuccess || light_cdf.upload(host_cdf) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the light power tables");
        return TAKE_OK;
    }
    int commit(SceneT<R> &sc) {  // moves only: always TAKE_OK
        sc.lights = std::move(lights), sc.light_pmf = std::move(light_pmf), sc.light_cdf = std::move(light_cdf);
        sc.host.lights = std::move(host_lights), sc.host.light_pmf = std::move(host_pmf), sc.host.light_cdf = std::move(host_cdf);
        for (int a = 0; a < 3; a++) sc.host.env.scale[a] = env.scale[a], sc.dev.env.scale[a] = env.scale[a];
        sc.bind();
        return TAKE_OK;
    }
};

int set_light_intensities(TakeScene *ts, const double *values, bool on_device, int32_t first, int32_t count, void *stream) {
    if (int rc = check_range_args(ts, values, first, count)) return rc;
    if (!on_device)
        for (int64_t i = 0; i < 3 * (int64_t)count; i++)
            if (!std::isfinite(values[i])) return fail(TAKE_E_INVALID, "light " + std::to_string(first + i / 3) + ": the intensity must be finite");
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    if ((int64_t)first + count > on_primary(ts, [](const auto &sc, const auto &) { return (int64_t)sc.host.lights.size(); })) return fail(TAKE_E_INVALID, RANGE_MESSAGE);
    // (the update runs on the default stream: first whatever `stream` still has to write into the values)
    if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    try {
        HIP_TRY(hipDeviceSynchronize());
        const size_t n = 3 * (size_t)count;
        DevBuf<double> staged;
        std::vector<double> host_copy;
        const double *d_rgb = values, *rgb = values;
        if (on_device) {  // the host's records and the serial pass need the values too
            host_copy.resize(n);
            HIP_TRY(hipMemcpy(host_copy.data(), values, n * sizeof(double), hipMemcpyDeviceToHost));
            rgb = host_copy.data();
        } else {
            if (staged.alloc(n) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the intensities");
            HIP_TRY(hipMemcpy(staged.p, values, n * sizeof(double), hipMemcpyHostToDevice));
            d_rgb = staged.p;
        }
        return stage_then_commit<LightStage>(ts, [&](const auto &sc, auto &stage) { return stage.prepare(sc, d_rgb, rgb, first, count); });
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while building the light tables");
    }
}

// ------------------------------------------------------------------------------------------------ test hook
template <class R> int debug_shading_info(const SceneT<R> &sc, TakeDebugShadingTablesInfo &o) {
    o = TakeDebugShadingTablesInfo{};
    o.n_materials = (int32_t)sc.materials.n, o.n_lights = (int32_t)sc.lights.n, o.n_instances = (int64_t)sc.inst_shade.n;
    o.real_bytes = (int32_t)sizeof(R);
    o.material_bytes = (int32_t)sizeof(MaterialRec<R>), o.light_bytes = (int32_t)sizeof(LightRec<R>), o.inst_shade_bytes = (int32_t)sizeof(InstShade<R>);
    o.tag_mask = sc.host.tag_mask, o.n_material_tags = sc.host.n_material_tags, o.single_tag = sc.host.single_tag;
    o.n_pmf = (int32_t)sc.light_pmf.n, o.n_cdf = (int32_t)sc.light_cdf.n;
    return TAKE_OK;
}
template <class R> int debug_shading_copy(const SceneT<R> &sc, void *materials, void *lights, void *pmf, void *cdf, void *inst_shade) {
    if (sc.materials.n) HIP_TRY(hipMemcpy(materials, sc.dev.materials, sc.materials.bytes(), hipMemcpyDeviceToHost));
    if (sc.lights.n) HIP_TRY(hipMemcpy(lights, sc.dev.lights, sc.lights.bytes(), hipMemcpyDeviceToHost));
    if (sc.light_pmf.n) HIP_TRY(hipMemcpy(pmf, sc.dev.light_pmf, sc.light_pmf.bytes(), hipMemcpyDeviceToHost));
    if (sc.light_cdf.n) HIP_TRY(hipMemcpy(cdf, sc.dev.light_cdf, sc.light_cdf.bytes(), hipMemcpyDeviceToHost));
    if (sc.inst_shade.n) HIP_TRY(hipMemcpy(inst_shade, sc.dev.inst_shade, sc.inst_shade.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}

}  // namespace

extern "C" {

int take_hip_scene_set_materials(TakeScene *ts, const TakeMaterial *materials, int32_t first, int32_t count) { return set_materials(ts, materials, first, count); }
int take_hip_scene_set_light_intensities(TakeScene *ts, const double *rgb, int32_t first, int32_t count) { return set_light_intensities(ts, rgb, false, first, count, nullptr); }
int take_hip_scene_set_light_intensities_device(TakeScene *ts, const double *d_rgb, int32_t first, int32_t count, void *stream) {
    return set_light_intensities(ts, d_rgb, true, first, count, stream);
}

int take_hip_debug_shading_tables_info(const TakeScene *ts, int32_t side, TakeDebugShadingTablesInfo *info) {
    if (!ts || !info) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    if (!has_side(ts, side)) return fail(TAKE_E_INVALID, "the scene has no such side");
    TAKE_ON_DEVICE(ts);
    return on_side(ts, side, [&](const auto &sc) { return debug_shading_info(sc, *info); });
}
int take_hip_debug_shading_tables(const TakeScene *ts, int32_t side, void *materials, void *lights, void *light_pmf, void *light_cdf, void *inst_shade) {
    if (!ts || !materials || !lights || !light_pmf || !light_cdf || !inst_shade) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    if (!has_side(ts, side)) return fail(TAKE_E_INVALID, "the scene has no such side");
    TAKE_ON_DEVICE(ts);
    HIP_TRY(hipDeviceSynchronize());
    return on_side(ts, side, [&](const auto &sc) { return debug_shading_copy(sc, materials, lights, light_pmf, light_cdf, inst_shade); });
}

}  // extern "C"
