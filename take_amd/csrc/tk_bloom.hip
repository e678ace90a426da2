// tk_bloom.hip — the C entry points of bloom and of the image workspace (include/take_hip.h: take_hip_image_workspace_*,
// take_hip_bloom_layer*, take_hip_tonemap_bloom*) and the only unit that compiles the kernels of tk_bloom.h.  Scene-free,
// as tk_display.hip, whose options, checks, histogram and auto-exposure it shares (tk_display_host.h).  The workspace
// is one device allocation: the histogram's block rows, then the pyramid's levels, each D_k turned into U_k in place.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "take_hip.h"
#include "tk_host.h"
#include "tk_display_host.h"
#include "tk_bloom.h"

using namespace tk;
using namespace tk_host;
using namespace tk_display;

// grows on demand, never shrinks; what it holds is scratch, so that growing keeps nothing
struct TakeImageWorkspace {
    int device = -1;
    DevBuf<char> buf;
    int reserve(size_t bytes) {
        if (bytes <= buf.n) return TAKE_OK;
        if (buf.alloc(bytes) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the image workspace");
        return TAKE_OK;
    }
};

namespace {
// TakeBloomOpts with the defaults filled in
struct BloomOpts {
    double threshold = 1.0, knee = 0.5, intensity = 0.25;
    int levels = 0;  // 0: all
};
int resolve_bloom(const TakeBloomOpts *o, BloomOpts &r) {
    r = BloomOpts{};
    if (!o) return TAKE_OK;
    if (!std::isfinite(o->threshold) || !std::isfinite(o->knee) || !std::isfinite(o->intensity)) return fail(TAKE_E_INVALID, "the bloom options must be finite");
    if (o->reserved != 0) return fail(TAKE_E_INVALID, "reserved must be 0");
    if (o->levels > TAKE_BLOOM_MAX_LEVELS) return fail(TAKE_E_INVALID, "levels must be at most TAKE_BLOOM_MAX_LEVELS");
    if (o->threshold >= 0) r.threshold = o->threshold;
    if (o->knee >= 0) r.knee = o->knee;
    if (o->intensity >= 0) r.intensity = o->intensity;
    if (o->levels > 0) r.levels = o->levels;
    if (r.knee > r.threshold) return fail(TAKE_E_INVALID, "knee must be at most the threshold");
    return TAKE_OK;
}

int check_layer_args(const void *rgb, int32_t precision, int32_t width, int32_t height, double exposure, const TakeBloomOpts *opts, const void *out, BloomOpts &b) {
    if (!rgb || !out) return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_image(precision, width, height)) return rc;
    if (!(exposure > 0) || !std::isfinite(exposure)) return fail(TAKE_E_INVALID, "the exposure must be positive and finite");
    if (int rc = resolve_bloom(opts, b)) return rc;
    const size_t bytes = 3 * real_bytes(precision) * (size_t)width * height;
    const char *a = (const char *)rgb, *o = (const char *)out;
    if (a != o && a < o + bytes && o < a + bytes) return fail(TAKE_E_INVALID, "the layer output must not partly overlap the input");
    return TAKE_OK;
}

constexpr size_t ALIGN = 256;
size_t aligned(size_t bytes) { return (bytes + ALIGN - 1) / ALIGN * ALIGN; }

// `ws` or, without one, a workspace of this call alone; then the workspace's two parts for this image
struct Workspace {
    TakeImageWorkspace temporary, *ws;
    uint32_t *slab = nullptr;
    char *pyramid = nullptr;
    explicit Workspace(TakeImageWorkspace *given) : ws(given ? given : &temporary) {}
    int prepare(const bl::Pyramid &pyr, int32_t precision, int64_t npix, bool histogram) {
        int device = 0;
        HIP_TRY(hipGetDevice(&device));
        if (ws == &temporary) ws->device = device;
        if (ws->device != device) return fail(TAKE_E_INVALID, "the image workspace belongs to another device");
        const size_t slab_bytes = histogram ? aligned(histogram_slab_words(npix) * sizeof(uint32_t)) : 0;
        if (int rc = ws->reserve(slab_bytes + (size_t)pyr.pixels() * 3 * real_bytes(precision))) return rc;
        slab = histogram ? (uint32_t *)ws->buf.p : nullptr;
        pyramid = ws->buf.p + slab_bytes;
        return TAKE_OK;
    }
};

dim3 row_grid(int w, int h) { return dim3((unsigned)((w + bl::ROW_X - 1) / bl::ROW_X), (unsigned)std::min((h + bl::ROW_Y - 1) / bl::ROW_Y, bl::MAX_GRID_Y)); }

// Steps 1 to 5 on `stream`: the image's bright pass down the pyramid, then the upsamples back -> U_0 at level[0]
template <class R> void launch_pyramid(const bl::Params<R> &P, const R *d_rgb, int width, int height, const bl::Pyramid &pyr, R *const *level, hipStream_t s) {
    const dim3 block(bl::TILE, bl::TILE);
    auto tiles = [](int w, int h) { return dim3((unsigned)((w + bl::TILE - 1) / bl::TILE), (unsigned)std::min((h + bl::TILE - 1) / bl::TILE, bl::MAX_GRID_Y)); };
    hipLaunchKernelGGL((bl::k_bloom_down<R, true>), tiles(pyr.w[0], pyr.h[0]), block, 0, s, P, d_rgb, width, height, level[0], pyr.w[0], pyr.h[0]);
    for (int k = 1; k < pyr.n; k++)
        hipLaunchKernelGGL((bl::k_bloom_down<R, false>), tiles(pyr.w[k], pyr.h[k]), block, 0, s, P, (const R *)level[k - 1], pyr.w[k - 1], pyr.h[k - 1], level[k], pyr.w[k], pyr.h[k]);
    for (int k = pyr.n - 2; k >= 0; k--)
        hipLaunchKernelGGL((bl::k_bloom_up<R, false>), row_grid(pyr.w[k], pyr.h[k]), dim3(bl::ROW_X, bl::ROW_Y), 0, s, (const R *)level[k], (const R *)level[k + 1], pyr.w[k + 1], pyr.h[k + 1], level[k],
                           pyr.w[k], pyr.h[k], R(0));
}

template <class R> bl::Params<R> bloom_params(double exposure, const BloomOpts &b, const bl::Pyramid &pyr) {
    return bl::Params<R>{(R)exposure, (R)b.threshold, (R)b.knee, (R)(b.intensity / (double)pyr.n)};
}
template <class R> void level_pointers(char *pyramid, const bl::Pyramid &pyr, R **level) {
    R *p = (R *)pyramid;
    for (int k = 0; k < pyr.n; k++) level[k] = p, p += (size_t)pyr.w[k] * pyr.h[k] * 3;
}
}  // namespace

extern "C" {

int take_hip_image_workspace_create(TakeImageWorkspace **out) {
    if (!out) return fail(TAKE_E_INVALID, "null argument");
    *out = nullptr;
    const int nd = check_device();
    if (nd < 0) return nd;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    TakeImageWorkspace *ws = new TakeImageWorkspace;
    ws->device = device;
    *out = ws;
    return TAKE_OK;
}

void take_hip_image_workspace_destroy(TakeImageWorkspace *ws) { delete ws; }

int take_hip_bloom_layer_device(const void *d_rgb, int32_t precision, int32_t width, int32_t height, double exposure, const TakeBloomOpts *opts,
                                void *d_layer_out, TakeImageWorkspace *ws, void *stream) {
    BloomOpts b;
    if (int rc = check_layer_args(d_rgb, precision, width, height, exposure, opts, d_layer_out, b)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    hipStream_t s = (hipStream_t)stream;
    const bl::Pyramid pyr = bl::pyramid_of(width, height, b.levels);
    Workspace work(ws);
    if (int rc = work.prepare(pyr, precision, (int64_t)width * height, false)) return rc;
    with_real(precision, [&](auto tag) {
        using R = decltype(tag);
        const bl::Params<R> P = bloom_params<R>(exposure, b, pyr);
        R *level[bl::MAX_LEVELS];
        level_pointers(work.pyramid, pyr, level);
        launch_pyramid(P, (const R *)d_rgb, width, height, pyr, level, s);
        hipLaunchKernelGGL((bl::k_bloom_up<R, true>), row_grid(width, height), dim3(bl::ROW_X, bl::ROW_Y), 0, s, (const R *)nullptr, (const R *)level[0], pyr.w[0], pyr.h[0], (R *)d_layer_out, width,
                           height, P.gain);
        return 0;
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));  // (before a temporary workspace is freed)
    return TAKE_OK;
}

int take_hip_bloom_layer(const void *rgb, int32_t precision, int32_t width, int32_t height, double exposure, const TakeBloomOpts *opts, void *layer_out) {
    BloomOpts b;
    if (int rc = check_layer_args(rgb, precision, width, height, exposure, opts, layer_out, b)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    // rgb, and the layer written over it
    StagedPlanes<1> st{{plane_inout(rgb, layer_out, 3 * real_bytes(precision))}};
    if (int rc = st.alloc((size_t)width * height, "out of device memory for the image")) return rc;
    if (int rc = st.upload()) return rc;
    if (int rc = take_hip_bloom_layer_device(st[0], precision, width, height, exposure, opts, st[0], nullptr, nullptr)) return rc;
    return st.download();
}

int take_hip_tonemap_bloom_device(const void *d_rgb, int32_t precision, int32_t width, int32_t height, const TakeTonemapOpts *opts, const TakeBloomOpts *bloom,
                                  void *d_out, double *exposure_used, TakeImageWorkspace *ws, void *stream) {
    TonemapOpts o;
    BloomOpts b;
    if (int rc = check_tonemap_args(d_rgb, precision, width, height, opts, d_out, o)) return rc;
    if (int rc = resolve_bloom(bloom, b)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    hipStream_t s = (hipStream_t)stream;
    const bl::Pyramid pyr = bl::pyramid_of(width, height, b.levels);
    Workspace work(ws);
    double E = o.exposure;
    if (int rc = work.prepare(pyr, precision, (int64_t)width * height, !(E > 0))) return rc;
    if (!(E > 0)) {
        int64_t hist[dp::SLOTS];
        if (int rc = histogram_on_device(d_rgb, precision, width, height, hist, s, work.slab)) return rc;
        E = auto_exposure(hist, o.auto_opts);
    }
    with_real(precision, [&](auto tag) {
        using R = decltype(tag);
        const bl::Params<R> P = bloom_params<R>(E, b, pyr);
        const dp::Params<R> T{(R)E, (R)(1.0 / (o.white * o.white)), o.op, o.transfer};
        R *level[bl::MAX_LEVELS];
        level_pointers(work.pyramid, pyr, level);
        launch_pyramid(P, (const R *)d_rgb, width, height, pyr, level, s);
        const dim3 grid = row_grid(width, height), block(bl::ROW_X, bl::ROW_Y);
        if (o.format == TAKE_DISPLAY_RGBA)
            hipLaunchKernelGGL((bl::k_tonemap_bloom<R, true>), grid, block, 0, s, T, P.gain, (const R *)d_rgb, width, height, (const R *)level[0], pyr.w[0], pyr.h[0], d_out);
        else
            hipLaunchKernelGGL((bl::k_tonemap_bloom<R, false>), grid, block, 0, s, T, P.gain, (const R *)d_rgb, width, height, (const R *)level[0], pyr.w[0], pyr.h[0], d_out);
        return 0;
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (exposure_used) *exposure_used = E;
    return TAKE_OK;
}

int take_hip_tonemap_bloom(const void *rgb, int32_t precision, int32_t width, int32_t height, const TakeTonemapOpts *opts, const TakeBloomOpts *bloom, void *out,
                           double *exposure_used) {
    TonemapOpts o;
    BloomOpts b;
    if (int rc = check_tonemap_args(rgb, precision, width, height, opts, out, o)) return rc;
    if (int rc = resolve_bloom(bloom, b)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    const bool rgba = o.format == TAKE_DISPLAY_RGBA;
    const size_t real = real_bytes(precision);
    // REAL: rgb, transformed in place; RGBA: rgb, then the codes
    StagedPlanes<2> st{{rgba ? plane_in(rgb, 3 * real) : plane_inout(rgb, out, 3 * real), plane_out(rgba ? out : nullptr, 4)}};
    if (int rc = st.alloc((size_t)width * height, "out of device memory for the display transform's planes")) return rc;
    if (int rc = st.upload()) return rc;
    if (int rc = take_hip_tonemap_bloom_device(st[0], precision, width, height, opts, bloom, rgba ? st[1] : st[0], exposure_used, nullptr, nullptr)) return rc;
    return st.download();
}

}  // extern "C"
