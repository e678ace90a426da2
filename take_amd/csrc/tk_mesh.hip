// tk_mesh.hip — mesh ingest of the C ABI of include/take_hip.h: PLY, Mitsuba serialized and Wavefront OBJ files decoded
// into device-array meshes (tk_ply.h, tk_obj.h), and compute_normals on device or host arrays (tk_normals.h).  The
// plumbing it shares with the other units (tk_api.hip, tk_scene_update.hip, tk_create.hip, tk_group.hip, tk_build.hip, tk_render.hip) is tk_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <clocale>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <locale.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <rocprim/rocprim.hpp>

#include "take_hip.h"
#include "tk_host.h"
#include "tk_ply.h"
#include "tk_obj.h"
#include "tk_normals.h"

using namespace tk;
using namespace tk_host;

namespace {

// ---- PLY -> device mesh arrays (tk_ply.h) --------------------------------------------------------------------------
void fill_layout(const ply::Layout &L, TakePlyLayout *o) {
    std::memset(o, 0, sizeof(*o));
    o->n_vertices = L.n_vertices, o->n_faces = L.n_faces;
    o->vertex_offset = L.vertex_off, o->face_offset = L.face_off;
    o->vertex_stride = L.vertex_stride, o->face_stride = L.face_stride;
    o->has_normals = L.nrm_type != ply::T_NONE, o->has_uvs = L.uv_type != ply::T_NONE;
    o->position_is_f64 = L.pos_type == ply::T_F64, o->index_bytes = ply::type_size(L.index_type);
    o->header_bytes = L.header_bytes;
}

// a file, memory-mapped read-only (the body is read once: by the copy to the device, or by the inflater)
struct MappedFile {
    void *p = nullptr;
    size_t n = 0;
    std::string err;
    explicit MappedFile(const char *path) {
        const int fd = open(path, O_RDONLY);
        if (fd < 0) {
            err = std::string("cannot open ") + path;
            return;
        }
        struct stat sb;
        if (fstat(fd, &sb) != 0 || sb.st_size <= 0) {
            close(fd);
            err = std::string("cannot read ") + path;
            return;
        }
        void *q = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (q == MAP_FAILED) {
            err = std::string("cannot map ") + path;
            return;
        }
        (void)madvise(q, (size_t)sb.st_size, MADV_SEQUENTIAL);
        p = q, n = (size_t)sb.st_size;
    }
    ~MappedFile() {
        if (p) munmap(p, n);
    }
    MappedFile(const MappedFile &) = delete;
    MappedFile &operator=(const MappedFile &) = delete;
};

// the *_file entry points: `path` mapped read-only, then the entry point on bytes in memory, `decode(bytes, n)`
template <class F> int from_file(const char *path, TakeMesh *out, const F &decode) {
    if (!path || !out) return fail(TAKE_E_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    MappedFile mf(path);
    if (!mf.p) return fail(TAKE_E_INVALID, mf.err);
    return decode(mf.p, mf.n);
}

void free_mesh_arrays(TakeMesh *m) {
    if (m->positions) (void)hipFree(const_cast<double *>(m->positions));
    if (m->indices) (void)hipFree(const_cast<int32_t *>(m->indices));
    if (m->normals) (void)hipFree(const_cast<double *>(m->normals));
    if (m->uvs) (void)hipFree(const_cast<double *>(m->uvs));
    std::memset(m, 0, sizeof(*m));
}

// to_world / inv_to_world as the decode kernels take them (null: the identity)
ply::Mat4 mat4_or_identity(const double *m) {
    ply::Mat4 M{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    if (m) std::memcpy(M.m, m, sizeof(M.m));
    return M;
}

// the four arrays of a decoded mesh, owned until they go into the caller's TakeMesh
struct MeshArrays {
    DevBuf<double> pos, nrm, uv;
    DevBuf<int32_t> idx;
    // (in this order: TAKE_HIP_FAIL_ALLOC counts the allocations)
    bool alloc(int64_t nv, int64_t nf, bool normals, bool uvs) {
        return pos.alloc(3 * (size_t)nv) == hipSuccess && idx.alloc(3 * (size_t)nf) == hipSuccess &&
               (!normals || nrm.alloc(3 * (size_t)nv) == hipSuccess) && (!uvs || uv.alloc(2 * (size_t)nv) == hipSuccess);
    }
    void hand_to(TakeMesh *out, int64_t nv, int64_t nf, int32_t material_id) {
        TakeMesh m{};
        m.n_vertices = nv, m.n_faces = nf, m.material_id = material_id, m.flags = TAKE_MESH_DEVICE_ARRAYS;
        m.positions = pos.detach(), m.indices = idx.detach(), m.normals = nrm.detach(), m.uvs = uv.detach();
        *out = m;
    }
};

// body (host) -> HBM, then the two decode kernels (tk_ply.h); D's offsets are relative to `host_body`
int decode_mesh_body(const uint8_t *host_body, const ply::Layout &D, const double *to_world, const double *inv_to_world,
                     int32_t material_id, const char *what, TakeMesh *out) {
    const ply::Mat4 X = mat4_or_identity(to_world), Xi = mat4_or_identity(inv_to_world);
    if (to_world && !inv_to_world && D.nrm_type != ply::T_NONE)
        return fail(TAKE_E_INVALID, "the file has normals: pass inverse(to_world) along with to_world");
    DevBuf<uint8_t> body;
    DevBuf<int32_t> status;
    MeshArrays a;
    if (body.alloc((size_t)std::max<int64_t>(D.end_off, 1)) != hipSuccess || status.alloc(1) != hipSuccess ||
        !a.alloc(D.n_vertices, D.n_faces, D.nrm_type != ply::T_NONE, D.uv_type != ply::T_NONE))
        return fail(TAKE_E_NOMEM, "out of device memory for a " + std::to_string(D.n_faces) + "-face " + what + " mesh");
    {
        PinnedUploads pin;
        hipError_t e = pin.copy(body.p, host_body, (size_t)D.end_off);
        if (e == hipSuccess) e = hipMemsetAsync(status.p, 0, sizeof(int32_t), pin.stream);
        constexpr int BLK = 256;
        if (e == hipSuccess && D.n_vertices > 0)
            hipLaunchKernelGGL(ply::k_ply_vertices, dim3((unsigned)((D.n_vertices + BLK - 1) / BLK)), dim3(BLK), 0, pin.stream, body.p, D, X, Xi,
                               a.pos.p, a.nrm.p, a.uv.p);
        if (e == hipSuccess && D.n_faces > 0)
            hipLaunchKernelGGL(ply::k_ply_faces, dim3((unsigned)((D.n_faces + BLK - 1) / BLK)), dim3(BLK), 0, pin.stream, body.p, D, a.idx.p, status.p);
        if (e == hipSuccess) e = hipGetLastError();
        int32_t st = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&st, status.p, sizeof(st), hipMemcpyDeviceToHost, pin.stream);
        if (e == hipSuccess) e = pin.finish();
        if (e != hipSuccess) return fail(TAKE_E_DEVICE, std::string(what) + " decode: " + hipGetErrorString(e));
        if (st & 1) return fail(TAKE_E_INVALID, std::string("a face of the ") + what + " file is not a triangle (the reference reads three indices per face)");
        if (st & 2) return fail(TAKE_E_INVALID, std::string("a face of the ") + what + " file indexes past its vertex array");
    }
    a.hand_to(out, D.n_vertices, D.n_faces, material_id);
    return TAKE_OK;
}

// ---- Mitsuba serialized meshes (src/parse/parse_serialized.cpp:174-256): inflate on the host, decode on the device --
struct Inflater {
    z_stream z{};
    bool open = false;
    const uint8_t *src;
    size_t left;
    Inflater(const uint8_t *p, size_t n) : src(p), left(n) {
        open = inflateInit2(&z, 15) == Z_OK;  // (windowBits 15: parse_serialized.cpp:47)
    }
    ~Inflater() {
        if (open) inflateEnd(&z);
    }
    // exactly `size` inflated bytes into dst, or what is wrong (the messages of ZStream::read, parse_serialized.cpp:60-104)
    const char *read(void *dst, size_t size) {
        uint8_t *out = (uint8_t *)dst;
        while (size > 0) {
            if (z.avail_in == 0) {
                const size_t take = std::min<size_t>(left, (size_t)1 << 30);
                if (take == 0) return "read less data than expected";
                z.next_in = const_cast<uint8_t *>(src), z.avail_in = (uInt)take;
                src += take, left -= take;
            }
            const size_t want = std::min<size_t>(size, (size_t)1 << 30);
            z.next_out = out, z.avail_out = (uInt)want;
            const int rv = inflate(&z, Z_NO_FLUSH);
            if (rv == Z_STREAM_ERROR) return "inflate(): stream error";
            if (rv == Z_NEED_DICT) return "inflate(): need dictionary";
            if (rv == Z_DATA_ERROR) return "inflate(): data error";
            if (rv == Z_MEM_ERROR) return "inflate(): memory error";
            const size_t got = want - z.avail_out;
            out += got, size -= got;
            if (size > 0 && rv == Z_STREAM_END) return "inflate(): attempting to read past the end of the stream";
            if (got == 0 && rv == Z_BUF_ERROR && left == 0 && z.avail_in == 0) return "read less data than expected";
        }
        return nullptr;
    }
};

// ---- Wavefront OBJ (src/parse/parse_obj.cpp:118-203): the whole file decoded on the device (tk_obj.h) -------------
// the three scan phases of tk_obj.h; `up` leaves the total in bsum[nb] (bsum: nb + 1 elements)
inline int64_t scan_tiles(int64_t n) { return (n + obj::SCAN_TILE - 1) / obj::SCAN_TILE; }
template <class T, class F> void scan_up(const F &f, int64_t n, T *bsum, hipStream_t st) {
    const int64_t nb = scan_tiles(n);
    if (nb > 0) hipLaunchKernelGGL((obj::k_scan_reduce<T, F>), dim3((unsigned)nb), dim3(obj::SCAN_BLK), 0, st, f, n, bsum);
    hipLaunchKernelGGL((obj::k_scan_blocks<T>), dim3(1), dim3(obj::SCAN_BLK), 0, st, bsum, nb);
}
template <class T, class F> void scan_down(const F &f, int64_t n, const T *bsum, hipStream_t st) {
    const int64_t nb = scan_tiles(n);
    if (nb > 0) hipLaunchKernelGGL((obj::k_scan_down<T, F>), dim3((unsigned)nb), dim3(obj::SCAN_BLK), 0, st, f, n, bsum);
}
inline dim3 grid_for(int64_t n, int blk) { return dim3((unsigned)std::max<int64_t>((n + blk - 1) / blk, 1)); }

// the numbers the device left to the host: strtod in the "C" locale, what `ss >> Real` computes.  -> the file offset
// of the first one out of the range of a double (the reference's stream fails on those), or -1
int64_t convert_fixups(const uint8_t *file, const std::vector<obj::Fix> &fx, std::vector<double> &val) {
    val.resize(fx.size());
    static locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    std::atomic<int64_t> bad{INT64_MAX};
    auto work = [&](size_t lo, size_t hi) {
        std::string tok;
        for (size_t k = lo; k < hi; k++) {
            tok.assign((const char *)file + fx[k].off, fx[k].len);
            errno = 0;
            val[k] = strtod_l(tok.c_str(), nullptr, c_locale);
            if (errno == ERANGE) {
                int64_t cur = bad.load();
                while ((int64_t)fx[k].off < cur && !bad.compare_exchange_weak(cur, (int64_t)fx[k].off)) {
                }
            }
        }
    };
    const size_t nt = fx.size() < 65536 ? 1 : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nt; t++) pool.emplace_back(work, fx.size() * t / nt, fx.size() * (t + 1) / nt);
    work(0, fx.size() / nt);
    for (auto &t : pool) t.join();
    return bad.load() == INT64_MAX ? -1 : bad.load();
}

std::string obj_message(uint32_t code, int64_t line) {
    const std::string at = "OBJ line " + std::to_string(line + 1) + ": ";
    switch (code) {
    case obj::S_UNSUPPORTED:
        return "unsupported " + at + "a token the reference's parser would not read (std::stoi throws, or a number is missing "
               "or not in the grammar [+-]?(d+(.d*)?|.d+)([eE][+-]?d+)?): keep the host parser";
    case obj::S_FEW: return at + "a face with fewer than 3 corners";
    case obj::S_V0: return at + "a vertex index 0";
    case obj::S_RANGE: return at + "an index outside its pool as it stands at that line";
    default: return at + "The object file contains n-gon (n>4) that we do not support.";
    }
}

int decode_obj(const uint8_t *file, size_t n_bytes, const double *to_world, const double *inv_to_world, int32_t material_id,
               TakeMesh *out) {
    if (n_bytes >= ((size_t)1 << 31) - 1) return fail(TAKE_E_INVALID, "unsupported OBJ file: 2 GiB or larger");
    const int64_t n = (int64_t)n_bytes;
    const ply::Mat4 X = mat4_or_identity(to_world), Xi = mat4_or_identity(inv_to_world);
    DevBuf<uint8_t> body, type;
    DevBuf<int32_t> nl, bsum_i, owner, minseq, slot, rank;
    DevBuf<obj::Cnt> pre, bsum_c;
    DevBuf<double> raw, fixval;
    DevBuf<obj::Corner> corners;
    DevBuf<obj::Face> faces;
    DevBuf<obj::Fix> fix;
    DevBuf<unsigned int> nfix, counts;
    DevBuf<unsigned long long> status;
    auto nomem = [&]() { return fail(TAKE_E_NOMEM, "out of device memory for an OBJ mesh of " + std::to_string(n) + " bytes"); };
    auto dev = [&](hipError_t e) { return fail(TAKE_E_DEVICE, std::string("OBJ decode: ") + hipGetErrorString(e)); };
    constexpr int BLK = 256;
    PinnedUploads pin;
    const hipStream_t st = pin.stream;
    hipError_t e = hipSuccess;
    // 1. the file -> HBM; '\n' positions
    if (body.alloc((size_t)std::max<int64_t>(n, 1)) != hipSuccess || bsum_i.alloc(scan_tiles(std::max(n, (int64_t)1)) + 1) != hipSuccess ||
        status.alloc(1) != hipSuccess || nfix.alloc(1) != hipSuccess || counts.alloc(2) != hipSuccess)
        return nomem();
    e = pin.copy(body.p, file, (size_t)n);
    if (e == hipSuccess) e = hipMemsetAsync(status.p, 0xFF, sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(nfix.p, 0, sizeof(unsigned int), st);
    if (e == hipSuccess) e = hipMemsetAsync(counts.p, 0, 2 * sizeof(unsigned int), st);
    if (e != hipSuccess) return dev(e);
    obj::NewlineF nf_{body.p, nullptr};
    scan_up<int32_t>(nf_, n, bsum_i.p, st);
    int32_t nnl = 0;
    e = hipMemcpyAsync(&nnl, bsum_i.p + scan_tiles(n), sizeof(nnl), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return dev(e);
    const int64_t nlines = (int64_t)nnl + 1;
    if (nl.alloc(std::max(nnl, 1)) != hipSuccess || type.alloc(nlines) != hipSuccess || pre.alloc(nlines) != hipSuccess ||
        bsum_c.alloc(scan_tiles(nlines) + 1) != hipSuccess)
        return nomem();
    nf_.nl = nl.p;
    scan_down<int32_t>(nf_, n, bsum_i.p, st);
    // 2. line types; 3. their scan
    hipLaunchKernelGGL(obj::k_obj_classify, grid_for(nlines, BLK), dim3(BLK), 0, st, body.p, n, nl.p, (int64_t)nnl, type.p);
    const obj::LineF lf{type.p, pre.p};
    scan_up<obj::Cnt>(lf, nlines, bsum_c.p, st);
    scan_down<obj::Cnt>(lf, nlines, bsum_c.p, st);
    obj::Cnt T{};
    e = hipMemcpyAsync(&T, bsum_c.p + scan_tiles(nlines), sizeof(T), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return dev(e);
    if (T.c >= (1 << 28)) return fail(TAKE_E_INVALID, "unsupported OBJ file: more than 2^28 face corners");
    if (to_world && !inv_to_world && T.vn > 0)
        return fail(TAKE_E_INVALID, "the file has normals: pass inverse(to_world) along with to_world");
    // 4. numbers, corners, faces
    const int64_t off_vt = 4 * (int64_t)T.v, off_vn = off_vt + 2 * (int64_t)T.vt, n_raw = off_vn + 3 * (int64_t)T.vn;
    if (raw.alloc(std::max<int64_t>(n_raw, 1)) != hipSuccess || fix.alloc(std::max<int64_t>(n_raw, 1)) != hipSuccess ||
        corners.alloc(std::max(T.c, 1)) != hipSuccess || faces.alloc(std::max(T.f, 1)) != hipSuccess)
        return nomem();
    hipLaunchKernelGGL(obj::k_obj_parse, grid_for(nlines, BLK), dim3(BLK), 0, st, body.p, n, nl.p, (int64_t)nnl, type.p, pre.p,
                       raw.p, off_vt, off_vn, corners.p, faces.p, fix.p, nfix.p, status.p);
    unsigned int n_fix = 0;
    e = hipMemcpyAsync(&n_fix, nfix.p, sizeof(n_fix), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return dev(e);
    int64_t host_bad = -1;  // file offset of a number out of the range of a double
    if (n_fix > 0) {
        std::vector<obj::Fix> fx(n_fix);
        std::vector<double> val;
        e = hipMemcpy(fx.data(), fix.p, n_fix * sizeof(obj::Fix), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return dev(e);
        host_bad = convert_fixups(file, fx, val);
        if (fixval.alloc(n_fix) != hipSuccess) return nomem();
        e = hipMemcpy(fixval.p, val.data(), n_fix * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) return dev(e);
        hipLaunchKernelGGL(obj::k_obj_patch, grid_for(n_fix, BLK), dim3(BLK), 0, st, fix.p, fixval.p, (int64_t)n_fix, raw.p);
    }
    // 5. deduplication on the raw triple
    uint32_t cap = 64;
    while (cap < 2 * (uint32_t)T.c) cap <<= 1;
    if (owner.alloc(cap) != hipSuccess || minseq.alloc(cap) != hipSuccess || slot.alloc(std::max(T.c, 1)) != hipSuccess ||
        rank.alloc(std::max(T.c, 1)) != hipSuccess)
        return nomem();
    e = hipMemsetAsync(owner.p, 0xFF, cap * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(minseq.p, 0x7F, cap * sizeof(int32_t), st);
    if (e != hipSuccess) return dev(e);
    if (T.c > 0) hipLaunchKernelGGL(obj::k_obj_insert, grid_for(T.c, BLK), dim3(BLK), 0, st, corners.p, (int64_t)T.c, owner.p, minseq.p, cap - 1, slot.p);
    const obj::FirstF ff{slot.p, minseq.p, rank.p};
    scan_up<int32_t>(ff, T.c, bsum_i.p, st);  // (bsum_i has room: corners < bytes)
    scan_down<int32_t>(ff, T.c, bsum_i.p, st);
    int32_t nvert = 0;
    e = hipMemcpyAsync(&nvert, bsum_i.p + scan_tiles(T.c), sizeof(nvert), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return dev(e);
    // 6. the vertices, the triangles
    const int64_t ntri = (int64_t)T.c - 2 * (int64_t)T.f;
    MeshArrays a;
    if (!a.alloc(nvert, ntri, T.vn != 0, T.vt != 0)) return nomem();
    if (T.c > 0)
        hipLaunchKernelGGL(obj::k_obj_emit, grid_for(T.c, BLK), dim3(BLK), 0, st, corners.p, (int64_t)T.c, faces.p, slot.p, minseq.p,
                           rank.p, raw.p, off_vt, off_vn, X, Xi, a.pos.p, a.nrm.p, a.uv.p, status.p, counts.p);
    if (T.f > 0) hipLaunchKernelGGL(obj::k_obj_indices, grid_for(T.f, BLK), dim3(BLK), 0, st, faces.p, (int64_t)T.f, slot.p, minseq.p, rank.p, a.idx.p);
    e = hipGetLastError();
    unsigned long long stw = 0;
    unsigned int cnt[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&stw, status.p, sizeof(stw), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt, counts.p, sizeof(cnt), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = pin.finish();
    if (e != hipSuccess) return dev(e);
    // the earliest line with a problem decides, as in the reference's loop
    int64_t bad_line = stw == ~0ull ? INT64_MAX : (int64_t)(stw >> 8);
    uint32_t code = (uint32_t)(stw & 0xFF);
    if (host_bad >= 0) {
        const int64_t line = (int64_t)std::count(file, file + host_bad, (uint8_t)'\n');
        if (line < bad_line || (line == bad_line && code >= obj::S_UNSUPPORTED))
            return fail(TAKE_E_INVALID, "unsupported OBJ line " + std::to_string(line + 1) +
                                                 ": a number outside the range of a double (the reference's stream fails on it)");
    }
    if (bad_line != INT64_MAX) return fail(TAKE_E_INVALID, obj_message(code, bad_line));
    // TakeMesh holds one uv / normal per position: all vertices have one, or none has
    if (cnt[0] == 0) a.uv.release();
    if (cnt[1] == 0) a.nrm.release();
    if (cnt[0] != 0 && cnt[0] != (unsigned)nvert)
        return fail(TAKE_E_INVALID, "unsupported OBJ mesh: only some vertices have a texture coordinate (the reference's uvs would "
                                         "not match its positions)");
    if (cnt[1] != 0 && cnt[1] != (unsigned)nvert)
        return fail(TAKE_E_INVALID, "unsupported OBJ mesh: only some vertices have a normal (the reference's normals would not "
                                         "match its positions)");
    a.hand_to(out, nvert, ntri, material_id);
    return TAKE_OK;
}

// ---- compute_normals (src/compute_normals.cpp:12-47) on device arrays (tk_normals.h) -------------------------------
int normals_counts(int64_t nv, int64_t nf) {
    if (nv < 0 || nf < 0) return fail(TAKE_E_INVALID, "compute_normals: negative vertex or face count");
    if (nf > INT32_MAX / 3)
        return fail(TAKE_E_INVALID, "compute_normals: " + std::to_string(nf) + " faces are more than INT32_MAX corners (the kernels "
                                    "index corners with 32-bit integers)");
    if (nv >= INT32_MAX) return fail(TAKE_E_INVALID, "compute_normals: more vertices than 32-bit indices can name");
    return TAKE_OK;
}

// d_out: 3 * nv doubles, every one written.  Synchronous on `st`.
int normals_on_device(const double *d_pos, int64_t nv, const int32_t *d_idx, int64_t nf, double *d_out, hipStream_t st) {
    const int rc = normals_counts(nv, nf);
    if (rc != TAKE_OK) return rc;
    const int64_t nc = 3 * nf;
    const int64_t heavy_cap = std::max<int64_t>(1, std::min<int64_t>(nv, nc / (nrm::HEAVY + 1)));
    DevBuf<double> contrib;
    DevBuf<uint32_t> keys, keys_s, status;
    DevBuf<int32_t> vals, vals_s, begin, end, heavy;
    DevBuf<char> temp;
    if (contrib.alloc(3 * (size_t)nc) != hipSuccess || keys.alloc((size_t)nc) != hipSuccess || keys_s.alloc((size_t)nc) != hipSuccess ||
        vals.alloc((size_t)nc) != hipSuccess || vals_s.alloc((size_t)nc) != hipSuccess || begin.alloc((size_t)nv) != hipSuccess ||
        end.alloc((size_t)nv) != hipSuccess || heavy.alloc((size_t)heavy_cap) != hipSuccess || status.alloc(2) != hipSuccess)
        return fail(TAKE_E_NOMEM, "out of device memory for compute_normals on " + std::to_string(nf) + " faces");
    // the sort keys: vertex indices and the "adds nothing" key nv
    const int end_bit = std::max(1, 32 - __builtin_clz((uint32_t)std::max<int64_t>(nv, 1)));
    size_t temp_bytes = 0;
    if (nc > 0) {
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, keys.p, keys_s.p, vals.p, vals_s.p, (size_t)nc, 0, end_bit, st));
        if (temp.alloc(std::max<size_t>(temp_bytes, 1)) != hipSuccess)
            return fail(TAKE_E_NOMEM, "out of device memory for compute_normals' sort");
    }
    const int B = nrm::BLK;
    HIP_TRY(hipMemsetAsync(status.p, 0, status.bytes(), st));
    if (nv > 0) {
        HIP_TRY(hipMemsetAsync(begin.p, 0, begin.bytes(), st));
        HIP_TRY(hipMemsetAsync(end.p, 0, end.bytes(), st));
    }
    if (nc > 0) {
        hipLaunchKernelGGL(nrm::k_nrm_faces, grid_for(nf, B), dim3(B), 0, st, d_pos, d_idx, nf, nv, contrib.p, keys.p, vals.p, status.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::radix_sort_pairs(temp.p, temp_bytes, keys.p, keys_s.p, vals.p, vals_s.p, (size_t)nc, 0, end_bit, st));
        hipLaunchKernelGGL(nrm::k_nrm_bounds, grid_for(nc, B), dim3(B), 0, st, keys_s.p, nc, (uint32_t)nv, begin.p, end.p, heavy.p, status.p);
    }
    if (nv > 0) {
        hipLaunchKernelGGL(nrm::k_nrm_vertices, grid_for(nv, B), dim3(B), 0, st, contrib.p, vals_s.p, begin.p, end.p, nv, d_out);
        const int64_t heavy_waves = std::min<int64_t>(heavy_cap, 1024);
        if (nc > nrm::HEAVY)
            hipLaunchKernelGGL(nrm::k_nrm_heavy, grid_for(heavy_waves * 64, B), dim3(B), 0, st, contrib.p, vals_s.p, begin.p, end.p,
                               heavy.p, status.p, d_out);
    }
    HIP_TRY(hipGetLastError());
    uint32_t st_h[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(st_h, status.p, sizeof(st_h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (st_h[0] & 1) return fail(TAKE_E_INVALID, "compute_normals: a face indexes outside the vertex array [0, " + std::to_string(nv) + ")");
    return TAKE_OK;
}
}  // namespace

extern "C" {

int take_hip_ply_layout(const void *file_bytes, size_t n_bytes, TakePlyLayout *out) {
    if (!file_bytes || !out) return fail(TAKE_E_INVALID, "null argument");
    ply::Layout L;
    const std::string err = ply::parse_header((const uint8_t *)file_bytes, n_bytes, L);
    if (!err.empty()) return fail(TAKE_E_INVALID, err);
    fill_layout(L, out);
    return TAKE_OK;
}

int take_hip_mesh_from_ply(const void *file_bytes, size_t n_bytes, const double *to_world, const double *inv_to_world,
                           int32_t material_id, TakeMesh *out) {
    if (!file_bytes || !out) return fail(TAKE_E_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    ply::Layout L;
    const std::string err = ply::parse_header((const uint8_t *)file_bytes, n_bytes, L);
    if (!err.empty()) return fail(TAKE_E_INVALID, err);
    const int nd = check_device();
    if (nd < 0) return nd;
    // the body as it lies in the file: one copy, from the first to the last byte the two elements span
    const int64_t lo = std::min(L.vertex_off, L.face_off);
    ply::Layout D = L;  // offsets relative to the copied span
    D.vertex_off -= lo, D.face_off -= lo, D.nrm_base -= lo, D.uv_base -= lo, D.end_off -= lo;
    return decode_mesh_body((const uint8_t *)file_bytes + lo, D, to_world, inv_to_world, material_id, "PLY", out);
}

int take_hip_mesh_from_serialized(const void *file_bytes, size_t n_bytes, int32_t shape_index, const double *to_world,
                                  const double *inv_to_world, int32_t material_id, TakeMesh *out) {
    if (!file_bytes || !out) return fail(TAKE_E_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    const uint8_t *f = (const uint8_t *)file_bytes;
    if (n_bytes < 4) return fail(TAKE_E_INVALID, "not a serialized mesh file: shorter than its header");
    uint16_t version = 0;
    std::memcpy(&version, f + 2, 2);  // (the magic number in front of it is ignored: parse_serialized.cpp:178)
    if (version != 3 && version != 4) return fail(TAKE_E_INVALID, "serialized mesh: unknown format version " + std::to_string(version));
    size_t at = 0;
    if (shape_index > 0) {  // skip_to_idx (parse_serialized.cpp:117-133): the offset table at the end of the file
        uint32_t count = 0;
        std::memcpy(&count, f + n_bytes - 4, 4);
        const size_t esz = version == 4 ? 8 : 4;
        if ((uint64_t)shape_index >= count || n_bytes < 4 + esz * (size_t)count)
            return fail(TAKE_E_INVALID, "serialized mesh: shape index " + std::to_string(shape_index) + " of " + std::to_string(count));
        uint64_t off = 0;
        std::memcpy(&off, f + n_bytes - 4 - esz * ((size_t)count - (size_t)shape_index), esz);
        if (off + 4 > n_bytes) return fail(TAKE_E_INVALID, "serialized mesh: sub-mesh offset past the end of the file");
        at = (size_t)off;
    } else if (shape_index < 0) {
        return fail(TAKE_E_INVALID, "serialized mesh: negative shape index");
    }
    Inflater z(f + at + 4, n_bytes - at - 4);
    if (!z.open) return fail(TAKE_E_DEVICE, "could not initialize zlib");
    uint32_t flags = 0;
    uint64_t nv = 0, nf = 0;
    const char *bad = z.read(&flags, 4);
    if (!bad && version == 4) {  // the mesh's name, NUL-terminated
        char c = 1;
        while (!bad && c != 0) bad = z.read(&c, 1);
    }
    if (!bad) bad = z.read(&nv, 8);
    if (!bad) bad = z.read(&nf, 8);
    if (bad) return fail(TAKE_E_INVALID, std::string("serialized mesh: ") + bad);
    if (nv >= ((uint64_t)1 << 31) || nf >= ((uint64_t)1 << 31) / 3) return fail(TAKE_E_INVALID, "serialized mesh too large for 32-bit vertex indices");
    ply::Layout L;
    ply::serialized_layout(flags, (int64_t)nv, (int64_t)nf, L);
    const int nd = check_device();
    if (nd < 0) return nd;
    // the blocks, inflated once into one host buffer; the kernels read them where the stream put them
    std::unique_ptr<uint8_t[]> body(new (std::nothrow) uint8_t[(size_t)std::max<int64_t>(L.end_off, 1)]);
    if (!body) return fail(TAKE_E_NOMEM, "out of host memory for the inflated mesh");
    bad = z.read(body.get(), (size_t)L.end_off);
    if (bad) return fail(TAKE_E_INVALID, std::string("serialized mesh: ") + bad);
    return decode_mesh_body(body.get(), L, to_world, inv_to_world, material_id, "serialized", out);
}

int take_hip_mesh_from_obj(const void *file_bytes, size_t n_bytes, const double *to_world, const double *inv_to_world,
                           int32_t material_id, TakeMesh *out) {
    if (!file_bytes || !out) return fail(TAKE_E_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    const int nd = check_device();
    if (nd < 0) return nd;
    return decode_obj((const uint8_t *)file_bytes, n_bytes, to_world, inv_to_world, material_id, out);
}

int take_hip_mesh_from_ply_file(const char *path, const double *to_world, const double *inv_to_world, int32_t material_id, TakeMesh *out) {
    return from_file(path, out, [&](const void *p, size_t n) { return take_hip_mesh_from_ply(p, n, to_world, inv_to_world, material_id, out); });
}

int take_hip_mesh_from_serialized_file(const char *path, int32_t shape_index, const double *to_world, const double *inv_to_world,
                                       int32_t material_id, TakeMesh *out) {
    return from_file(path, out, [&](const void *p, size_t n) {
        return take_hip_mesh_from_serialized(p, n, shape_index, to_world, inv_to_world, material_id, out);
    });
}

int take_hip_mesh_from_obj_file(const char *path, const double *to_world, const double *inv_to_world, int32_t material_id, TakeMesh *out) {
    return from_file(path, out, [&](const void *p, size_t n) { return take_hip_mesh_from_obj(p, n, to_world, inv_to_world, material_id, out); });
}

int take_hip_mesh_compute_normals(TakeMesh *mesh) {
    if (!mesh) return fail(TAKE_E_INVALID, "null mesh");
    if (!(mesh->flags & TAKE_MESH_DEVICE_ARRAYS))
        return fail(TAKE_E_INVALID, "compute_normals: not a device-array mesh (host arrays: take_hip_compute_normals)");
    if (mesh->normals) return fail(TAKE_E_INVALID, "compute_normals: the mesh has normals already");
    int rc = normals_counts(mesh->n_vertices, mesh->n_faces);
    if (rc != TAKE_OK) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    DevBuf<double> nrm;
    if (nrm.alloc(3 * (size_t)mesh->n_vertices) != hipSuccess)
        return fail(TAKE_E_NOMEM, "out of device memory for the normals of a " + std::to_string(mesh->n_vertices) + "-vertex mesh");
    rc = normals_on_device(mesh->positions, mesh->n_vertices, mesh->indices, mesh->n_faces, nrm.p, nullptr);
    if (rc != TAKE_OK) return rc;
    mesh->normals = nrm.detach();
    return TAKE_OK;
}

int take_hip_compute_normals(const double *positions, int64_t n_vertices, const int32_t *indices, int64_t n_faces,
                             double *normals_out) {
    int rc = normals_counts(n_vertices, n_faces);
    if (rc != TAKE_OK) return rc;
    if ((n_vertices > 0 && (!positions || !normals_out)) || (n_faces > 0 && !indices)) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    DevBuf<double> pos, out;
    DevBuf<int32_t> idx;
    if (pos.alloc(3 * (size_t)n_vertices) != hipSuccess || out.alloc(3 * (size_t)n_vertices) != hipSuccess ||
        idx.alloc(3 * (size_t)n_faces) != hipSuccess)
        return fail(TAKE_E_NOMEM, "out of device memory for compute_normals on " + std::to_string(n_faces) + " faces");
    PinnedUploads pin;
    HIP_TRY(pin.copy(pos.p, positions, pos.bytes()));
    HIP_TRY(pin.copy(idx.p, indices, idx.bytes()));
    rc = normals_on_device(pos.p, n_vertices, idx.p, n_faces, out.p, pin.stream);
    HIP_TRY(pin.finish());
    if (rc != TAKE_OK) return rc;
    if (out.n) HIP_TRY(hipMemcpy(normals_out, out.p, out.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}

int take_hip_mesh_download(const TakeMesh *m, double *positions, int32_t *indices, double *normals, double *uvs) {
    if (!m) return fail(TAKE_E_INVALID, "null mesh");
    if (!(m->flags & TAKE_MESH_DEVICE_ARRAYS)) return fail(TAKE_E_INVALID, "not a device-array mesh");
    auto down = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        return (dst && src && bytes) ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
    };
    HIP_TRY(down(positions, m->positions, sizeof(double) * 3 * (size_t)m->n_vertices));
    HIP_TRY(down(indices, m->indices, sizeof(int32_t) * 3 * (size_t)m->n_faces));
    HIP_TRY(down(normals, m->normals, sizeof(double) * 3 * (size_t)m->n_vertices));
    HIP_TRY(down(uvs, m->uvs, sizeof(double) * 2 * (size_t)m->n_vertices));
    return TAKE_OK;
}

int take_hip_mesh_release(TakeMesh *m) {
    if (!m) return TAKE_OK;
    if (m->flags & TAKE_MESH_DEVICE_ARRAYS) free_mesh_arrays(m);
    return TAKE_OK;
}

}  // extern "C"
