// shading_update_host.cpp — TEST INFRASTRUCTURE.  The bodies of take_amd/csrc/tk_shading_update.h built for the host and
// run in the loop structure of its kernels' launches — blocks of BLOCK threads, one record or light per thread, the
// blocks striding when the grid is smaller than the work, the tail block partly idle — so that
// tests/test_shading_update_cpu.py can hold what take_hip_scene_set_materials and take_hip_scene_set_light_intensities
// leave on the device to what scene creation makes on the host (material_table + shape_record's meta + placement_records'
// tag, light_records + light_power_tables of tk_host_scene.h), byte for byte, without a GPU.  With -DSHADING_UPDATE_MAIN
// a stand-alone program that runs the same comparison on scenes it makes itself (the sanitizer build of the Makefile).
// Never loaded by the product.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "tk_host_scene.h"
#include "tk_shading_update.h"

namespace {
using namespace tk;

std::string g_error;

// a kernel of tk_shading_update.h as `grid` blocks of BLOCK threads run it over n entries (grid <= 0: the launch's own)
template <class F> void launch(int64_t n, int grid, F &&body) {
    if (grid <= 0) grid = (int)su::blocks_for(n);
    for (int block = 0; block < grid; block++)
        for (int tid = 0; tid < su::BLOCK; tid++)
            for (int64_t i = (int64_t)block * su::BLOCK + tid; i < n; i += (int64_t)grid * su::BLOCK) body(i);
}

template <class T> bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

enum Part { MATERIALS = 1, PRIMS = 2, PLACEMENTS = 4, TAGS_IN_USE = 8, LIGHTS = 16, PMF = 32, CDF = 64, ENV_SCALE = 128, GUARD = 256 };

// what MaterialStage (tk_shading_update.hip) does to a side, on the host's copy of the scene made from `a`; -> the parts
// that differ from the scene made from `b`, or -1
template <class R> int materials(const TakeSceneDesc &a, const TakeSceneDesc &b, int first, int count, bool burley, int grid, int max_leaf, int64_t *n_records, int *retagged) {
    HostScene<R> ha, hb;
    std::string err = prepare_scene<R>(a, max_leaf, 1, ha, PREP_HOST_BUILD, burley);
    if (err.empty()) err = prepare_scene<R>(b, max_leaf, 1, hb, PREP_HOST_BUILD, burley);
    if (!err.empty() || first < 0 || count <= 0 || (size_t)first + count > ha.materials.size()) return g_error = err.empty() ? "bad range" : err, -1;
    bool retag = false;
    for (int k = 0; k < count; k++) {
        MaterialRec<R> rec{};
        err = material_record(b.materials[first + k], first + k, (int)ha.images.size(), burley, rec);
        if (!err.empty()) return g_error = err, -1;
        retag = retag || rec.tag != ha.materials[first + k].tag;
        ha.materials[first + k] = rec;
    }
    material_tags_in_use(ha.materials, ha.n_material_tags, ha.tag_mask, ha.single_tag);
    std::vector<int32_t> tags(ha.materials.size());
    for (size_t i = 0; i < tags.size(); i++) tags[i] = ha.materials[i].tag;
    const int64_t n = (int64_t)ha.prims.size(), n_inst = (int64_t)ha.inst_shade.size();
    // (a record behind each array that no thread may touch)
    ha.prims.push_back(PrimRec<R>{}), ha.inst_shade.push_back(InstShade<R>{});
    ha.prims.back().meta = 0x7f7f7f7f, ha.prims.back().material = 0, ha.inst_shade.back().tag = 0x7f7f7f7f, ha.inst_shade.back().material = 0;
    if (retag) {
        launch(n, grid, [&](int64_t i) { su::retag_prim(ha.prims.data(), i, tags.data(), (int32_t)tags.size()); });
        launch(n_inst, grid, [&](int64_t i) { su::retag_placement(ha.inst_shade.data(), i, tags.data(), (int32_t)tags.size()); });
    }
    int bad = (ha.prims.back().meta != 0x7f7f7f7f || ha.inst_shade.back().tag != 0x7f7f7f7f) ? GUARD : 0;
    ha.prims.pop_back(), ha.inst_shade.pop_back();
    if (!same(ha.materials, hb.materials)) bad |= MATERIALS;
    if (!same(ha.prims, hb.prims)) bad |= PRIMS;
    if (ha.inst_shade.size() != hb.inst_shade.size()) bad |= PLACEMENTS;
    for (size_t i = 0; i < ha.inst_shade.size() && i < hb.inst_shade.size(); i++) {
        const InstShade<R> &x = ha.inst_shade[i], &y = hb.inst_shade[i];
        if (std::memcmp(x.fwd, y.fwd, sizeof x.fwd) || x.material != y.material || x.tag != y.tag || x.shape_base != y.shape_base) bad |= PLACEMENTS;
    }
    if (ha.tag_mask != hb.tag_mask || ha.n_material_tags != hb.n_material_tags || ha.single_tag != hb.single_tag) bad |= TAGS_IN_USE;
    if (n_records) *n_records = n;
    if (retagged) *retagged = retag ? 1 : 0;
    return bad;
}

// what LightStage does to a side: the staged records, k_light_power over the range, the serial pass
template <class R> int lights(const TakeSceneDesc &a, const TakeSceneDesc &b, int first, int count, int grid) {
    HostScene<R> ha, hb;
    std::string err = prepare_scene<R>(a, 0, 1, ha, PREP_HOST_BUILD, false);
    if (err.empty()) err = prepare_scene<R>(b, 0, 1, hb, PREP_HOST_BUILD, false);
    if (!err.empty() || first < 0 || count <= 0 || (size_t)first + count > ha.lights.size()) return g_error = err.empty() ? "bad range" : err, -1;
    std::vector<double> rgb(3 * (size_t)count);
    for (int k = 0; k < count; k++)
        for (int c = 0; c < 3; c++) rgb[3 * (size_t)k + c] = b.lights[first + k].intensity[c];
    std::vector<LightRec<R>> staged = ha.lights;
    staged.push_back(LightRec<R>{});
    staged.back().kind = 1, staged.back().intensity[0] = R(-77);
    std::vector<R> power((size_t)count + 1, R(-77));
    launch(count, grid, [&](int64_t k) { su::set_light_intensity(staged.data(), first, k, rgb.data(), power.data()); });
    int bad = (staged.back().intensity[0] != R(-77) || power.back() != R(-77)) ? GUARD : 0;
    staged.pop_back();
    std::vector<R> pmf(staged.size()), cdf;
    for (size_t i = 0; i < staged.size(); i++) pmf[i] = ((int)i >= first && (int)i < first + count) ? power[i - first] : su::light_power(ha.lights[i]);
    su::light_tables_from_powers<R>(pmf, cdf);
    EnvMap<R> env = ha.env;
    if (env.light >= first && env.light < first + count)
        for (int c = 0; c < 3; c++) env.scale[c] = staged[env.light].intensity[c];
    if (!same(staged, hb.lights)) bad |= LIGHTS;
    if (!same(pmf, hb.light_pmf)) bad |= PMF;
    if (!same(cdf, hb.light_cdf)) bad |= CDF;
    if (std::memcmp(env.scale, hb.env.scale, sizeof env.scale)) bad |= ENV_SCALE;
    return bad;
}
}  // namespace

extern "C" {
const char *shading_update_last_error() { return g_error.c_str(); }
// a: the description as created, b: the same with materials [first, first + count) replaced.  real: 0 float, 1 double;
// grid <= 0: the launch's own grid.  -> 0 = the updated scene is the scene made from b, else the mismatching parts
// (1 table, 2 records, 4 placements, 8 tags in use, 256 a write outside the arrays), -1 = error.  n_records: the
// primitive records the retag ran over, retagged: whether it ran
int shading_update_materials(const TakeSceneDesc *a, const TakeSceneDesc *b, int first, int count, int burley, int real, int grid, int max_leaf, int64_t *n_records,
                             int *retagged) {
    if (!a || !b) return g_error = "null argument", -1;
    return real ? materials<double>(*a, *b, first, count, burley != 0, grid, max_leaf, n_records, retagged)
                : materials<float>(*a, *b, first, count, burley != 0, grid, max_leaf, n_records, retagged);
}
// a, b: the same with the intensities of lights [first, first + count) replaced -> 0, or 16 records, 32 pmf, 64 cdf,
// 128 the environment map's scale, 256 a write outside the arrays; -1 = error
int shading_update_lights(const TakeSceneDesc *a, const TakeSceneDesc *b, int first, int count, int real, int grid) {
    if (!a || !b) return g_error = "null argument", -1;
    return real ? lights<double>(*a, *b, first, count, grid) : lights<float>(*a, *b, first, count, grid);
}
}

#ifdef SHADING_UPDATE_MAIN
namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
double draw() {  // (xorshift64*: any fixed sequence will do)
    g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}
// n_tris triangles in two meshes (materials 0 and 1; those of the first emissive), n_spheres spheres (material 2, the
// first emissive), a point light at the end; three materials
struct Made {
    std::vector<double> pos[2], nrm[2];
    std::vector<int32_t> idx[2], kind, ref, face, al;
    std::vector<TakeMesh> meshes;
    std::vector<TakeSphere> spheres;
    std::vector<TakeLight> lights;
    std::vector<TakeMaterial> mats;
    TakeSceneDesc d{};
    Made(int n_tris, int n_spheres, bool emissive) {
        const int split[2] = {(n_tris + 1) / 2, n_tris / 2};
        for (int m = 0; m < 2; m++)
            for (int f = 0; f < split[m]; f++) {
                for (int k = 0; k < 9; k++) pos[m].push_back(2.0 * draw() - 1.0), nrm[m].push_back(k % 3 == 2 ? 1.0 : 0.0);
                for (int k = 0; k < 3; k++) idx[m].push_back(3 * f + k);
                if (m == 0 && emissive) lights.push_back(TakeLight{1, (int32_t)kind.size(), {1.0 + draw(), 2.0 * draw(), 0.5}, {0, 0, 0}});
                al.push_back(m == 0 && emissive ? (int32_t)lights.size() - 1 : -1);
                kind.push_back(1), ref.push_back(m), face.push_back(f);
            }
        for (int s = 0; s < n_spheres; s++) {
            spheres.push_back(TakeSphere{{2.0 * draw() - 1.0, 2.0 * draw() - 1.0, 2.0 * draw() - 1.0}, 0.05 + 0.2 * draw(), 2, 0});
            if (s == 0 && emissive) lights.push_back(TakeLight{1, (int32_t)kind.size(), {3.0, 2.0, 1.0}, {0, 0, 0}});
            al.push_back(s == 0 && emissive ? (int32_t)lights.size() - 1 : -1);
            kind.push_back(0), ref.push_back(s), face.push_back(0);
        }
        lights.push_back(TakeLight{0, -1, {5.0, 5.0, 5.0}, {0.0, 2.0, 0.0}});
        for (int m = 0; m < 2; m++) meshes.push_back(TakeMesh{3 * (int64_t)split[m], split[m], pos[m].data(), idx[m].data(), nrm[m].data(), nullptr, m, 0});
        for (int m = 0; m < 3; m++) {
            TakeMaterial mat{};
            mat.tag = TAKE_MAT_DIFFUSE;
            for (int c = 0; c < 3; c++) mat.reflectance.value[c] = 0.2 + 0.2 * m;
            mat.reflectance.uscale = mat.reflectance.vscale = 1.0;
            mats.push_back(mat);
        }
        d.camera = TakeCamera{16, 16, {0, 0, 4}, {0, 0, 0}, {0, 1, 0}, 40.0};
        d.n_meshes = 2, d.meshes = meshes.data(), d.n_spheres = n_spheres, d.spheres = spheres.data();
        d.n_shapes = (int64_t)kind.size(), d.shape_kind = kind.data(), d.shape_ref = ref.data(), d.shape_face = face.data(), d.shape_area_light = al.data();
        d.n_lights = (int32_t)lights.size(), d.lights = lights.data(), d.n_materials = 3, d.materials = mats.data();
    }
};
int report(const char *what, int n, int real, int grid, int rc) {
    if (rc) std::printf("MISMATCH %s, %d records, f%d, grid %d: %d %s\n", what, n, real ? 64 : 32, grid, rc, rc < 0 ? g_error.c_str() : "");
    return rc ? 1 : 0;
}
}  // namespace

int main() {
    int bad = 0, cases = 0;
    const int counts[] = {1, 63, 64, 65, 257, 1300};
    for (int n : counts)
        for (int real = 0; real < 2; real++)
            for (int grid : {0, 2}) {
                if (grid && n != 1300) continue;  // (two blocks that stride over 1300 entries)
                const int tris = n > 2 ? n - 2 : n, spheres = n - tris;
                {
                    Made a(tris, spheres, false);
                    std::vector<TakeMaterial> mats = a.mats;
                    mats[1].tag = TAKE_MAT_MIRROR, mats[2].tag = TAKE_MAT_PLASTIC, mats[2].param[0] = 1.5;
                    TakeSceneDesc b = a.d;
                    b.materials = mats.data();
                    int64_t records = 0;
                    int retagged = 0;
                    int rc = shading_update_materials(&a.d, &b, 1, 2, 0, real, grid, 0, &records, &retagged);
                    if (!rc && (records != n || !retagged)) rc = 512;
                    bad += report("materials", n, real, grid, rc), cases++;
                    mats = a.mats;  // colours only: no retag
                    mats[0].reflectance.value[1] = 0.9;
                    b.materials = mats.data();
                    rc = shading_update_materials(&a.d, &b, 0, 1, 0, real, grid, 0, &records, &retagged);
                    if (!rc && retagged) rc = 512;
                    bad += report("colours", n, real, grid, rc), cases++;
                }
                {
                    Made a(2 * n, 1, true);  // n emissive triangles, an emissive sphere, a point light: n + 2 lights
                    std::vector<TakeLight> lights = a.lights;
                    for (int i = 0; i < n + 2; i++)
                        for (int c = 0; c < 3; c++) lights[i].intensity[c] = 4.0 * draw();
                    TakeSceneDesc b = a.d;
                    b.lights = lights.data();
                    bad += report("lights", n + 2, real, grid, shading_update_lights(&a.d, &b, 0, n + 2, real, grid)), cases++;
                    for (int i = 0; i < n + 2; i++)
                        for (int c = 0; c < 3; c++) lights[i].intensity[c] = (i >= 1 && i < n) ? 0.0 : a.lights[i].intensity[c];
                    if (n > 2) bad += report("a sub-range", n + 2, real, grid, shading_update_lights(&a.d, &b, 1, n - 1, real, grid)), cases++;
                    for (int i = 0; i < n + 2; i++)
                        for (int c = 0; c < 3; c++) lights[i].intensity[c] = 0.0;  // (total power 0: NaN tables on both sides)
                    bad += report("dark", n + 2, real, grid, shading_update_lights(&a.d, &b, 0, n + 2, real, grid)), cases++;
                }
            }
    std::printf("shading_update_host: %d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
