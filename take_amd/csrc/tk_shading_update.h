// tk_shading_update.h — new materials and new light intensities for a resident scene: what
// take_hip_scene_set_materials and take_hip_scene_set_light_intensities* change on the device (include/take_hip.h;
// specification: DESIGN.md §4p).  The bodies below are TK_HD and written once: the kernels at the end of this file run
// them on the device, tk_host_scene.h's light_power_tables runs light_power on the host (scene creation),
// tests/shading_update_host runs them in the kernels' loop structure.  Launched from tk_shading_update.hip.
//
// Arithmetic: every + - * / is one operation in the order written (-ffp-contract=off) in the side's Real; the square
// root of `length` is the only library call, correctly rounded on both sides.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "take_hip.h"
#include "tk_scene.h"

namespace tk {
namespace su {

// PrimRec::meta with the material tag (bits 8..15) replaced; kind (bits 0..7) and the flags from bit 16 up stay
TK_HD int32_t retag_meta(int32_t meta, int32_t tag) { return (int32_t)(((uint32_t)meta & 0xffff00ffu) | (((uint32_t)tag & 0xffu) << 8)); }

// the tag of material `material` in a table of n_materials tags; a record that names no material of the table (there
// is none after creation's checks) keeps the tag it has
TK_HD int32_t tag_of(const int32_t *tags, int32_t n_materials, int32_t material, int32_t old_tag) {
    return material >= 0 && material < n_materials ? tags[material] : old_tag;
}

// record i of the primitive records: meta's tag from the new table.  Reads meta and material, writes meta — and only
// when it changes.  The pair is 8 bytes at an 8-byte aligned offset in PrimRec<float> (40, 44): one dwordx2 load per
// lane; in PrimRec<double> (76, 80) it is not: two dword loads.
template <class R> TK_HD void retag_prim(PrimRec<R> *prims, int64_t i, const int32_t *tags, int32_t n_materials) {
    PrimRec<R> &p = prims[i];
    int32_t meta, material;
    if constexpr (sizeof(R) == 4) {
        struct alignas(8) Pair { int32_t meta, material; };
        static_assert(offsetof(PrimRec<float>, meta) % 8 == 0 && offsetof(PrimRec<float>, material) == offsetof(PrimRec<float>, meta) + 4,
                      "meta and material: one aligned pair of the f32 record");
        const Pair pair = *reinterpret_cast<const Pair *>(&p.meta);
        meta = pair.meta, material = pair.material;
    } else {
        meta = p.meta, material = p.material;
    }
    const int32_t out = retag_meta(meta, tag_of(tags, n_materials, material, (meta >> 8) & 0xff));
    if (out != meta) p.meta = out;
}
// placement i of a two-level scene: InstShade::tag from its (resolved) material
template <class R> TK_HD void retag_placement(InstShade<R> *inst, int64_t i, const int32_t *tags, int32_t n_materials) {
    const int32_t tag = tag_of(tags, n_materials, inst[i].material, inst[i].tag);
    if (tag != inst[i].tag) inst[i].tag = tag;
}

// The power of a light (the reference's light_power(), src/light.cpp:9-30): luminance(intensity) * area * pi for a
// diffuse area light, 0 for a point light and for the environment map.
template <class R> TK_HD R light_power(const LightRec<R> &l) {
    R p = R(0);
    if (l.kind == 1) {
        R area;
        if (l.is_sphere) {
            area = R(4) * Const<R>::PI * l.v[3] * l.v[3];
        } else {
            const Vec3<R> v0 = {l.v[0], l.v[1], l.v[2]}, v1 = {l.v[3], l.v[4], l.v[5]}, v2 = {l.v[6], l.v[7], l.v[8]};
            area = length(cross(v1 - v0, v2 - v0)) / R(2);
        }
        p = (l.intensity[0] * R(0.212671) + l.intensity[1] * R(0.715160) + l.intensity[2] * R(0.072169)) * area * Const<R>::PI;
    }
    return p;
}
// light first + k of the staged records: its intensity from rgb[3 k ..] (double, rounded to R once), its power -> power[k]
template <class R> TK_HD void set_light_intensity(LightRec<R> *lights, int32_t first, int64_t k, const double *rgb, R *power) {
    LightRec<R> &l = lights[first + k];
    for (int a = 0; a < 3; a++) l.intensity[a] = R(rgb[3 * k + a]);
    power[k] = light_power(l);
}

// pmf (in: the lights' powers, in light order) -> pmf = power / total, cdf = the running sum from 0 (n + 1 entries):
// serial adds in light order in R, which is why this runs on the host for creation and for an update alike.  A total
// of 0 leaves NaN tables, as the reference's recipe does.
template <class R, class V> inline void light_tables_from_powers(V &pmf, V &cdf) {
    R total = R(0);
    for (const R &p : pmf) total += p;
    cdf.assign(1, R(0));
    for (R &p : pmf) {
        p = p / total;
        cdf.push_back(cdf.back() + p);
    }
}

constexpr int BLOCK = 256;
constexpr int64_t MAX_BLOCKS = 1 << 16;  // a launch's grid: beyond BLOCK * MAX_BLOCKS entries the blocks stride
inline int64_t blocks_for(int64_t n) {
    const int64_t b = (n + BLOCK - 1) / BLOCK;
    return b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

#if defined(__HIPCC__)
// One lane per record, in resident (leaf) order; consecutive lanes consecutive records: a wave reads 64 pairs, one per
// 64-byte (f32) / 96-byte (f64) record, and writes at most one dword per record.
template <class R> __global__ __launch_bounds__(BLOCK) void k_retag_prims(PrimRec<R> *prims, int64_t n, const int32_t *tags, int32_t n_materials) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) retag_prim(prims, i, tags, n_materials);
}
template <class R> __global__ __launch_bounds__(BLOCK) void k_retag_placements(InstShade<R> *inst, int64_t n, const int32_t *tags, int32_t n_materials) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) retag_placement(inst, i, tags, n_materials);
}
// one lane per light of the range [first, first + count)
template <class R> __global__ __launch_bounds__(BLOCK) void k_light_power(LightRec<R> *lights, int32_t first, int64_t count, const double *rgb, R *power) {
    for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < count; k += (int64_t)gridDim.x * BLOCK) set_light_intensity(lights, first, k, rgb, power);
}
#endif  // __HIPCC__

}  // namespace su
}  // namespace tk
