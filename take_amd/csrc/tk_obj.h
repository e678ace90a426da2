// Wavefront OBJ -> device mesh arrays (take_hip_mesh_from_obj): the third mesh format of the reference's scenes, after
// PLY and serialized (tk_ply.h).
//
// What it replaces: src/parse/parse_obj.cpp:118-203 — a line-at-a-time std::getline / stringstream loop that builds a
// std::regex per face corner and deduplicates corners through a std::map<ObjVertex, size_t>.  Here the host copies the
// file to HBM once and the kernels below do the rest, each one line / one corner / one face per lane:
//
//   1. '\n' positions: a three-phase scan over the bytes (per-tile counts, one scan of the tile sums, per-tile writes).
//   2. Per line: trim() (std::isspace in the "C" locale: ' ' \t \n \v \f \r), the first token -> v / vt / vn / f / other,
//      and for `f` lines the number of corners (3, 4, or anything else = an error line that makes no corners).
//   3. A scan over the line types gives each v / vt / vn line its slot in its pool, each f line its face number, its
//      first corner (= the sequence number of its first get_vertex_id call) and the three pool sizes AT that line
//      (a negative index is relative to the pool as the face line finds it).
//   4. Per line: the numbers (`ss >> Real`: libstdc++ num_get -> strtod, correctly rounded).  Clinger's exact case
//      (at most 15 significant digits, decimal exponent in [-22, 22]) is one IEEE multiply or divide of two exact
//      doubles on the device; any other token of the grammar [+-]?(d+(.d*)?|.d+)([eE][+-]?d+)? is recorded as a
//      (byte offset, length, destination) fix-up that the host converts with strtod and patches in before the pools
//      are read.  The corners: split_face_str (pieces between '/', a trailing empty piece dropped, "" -> 0, std::stoi
//      on the rest: a leading integer, whatever follows it ignored).
//   5. Deduplication on the RAW (v, vt, vn) triple, as the std::map does: an open-addressing table whose slot keeps
//      atomicMin(corner sequence number); a corner is its vertex's first occurrence iff the minimum is itself, and an
//      exclusive scan over those flags numbers the vertices in the reference's order.  Deterministic by construction.
//   6. Per first occurrence: get_vertex_id's index resolution (negative vt resolves to pool + vt - 1: the reference's
//      off-by-one, kept), Vector3{x,y,z} / w, (s, 1 - t), normalize(); then xform_point / xform_normal (tk_ply.h).
//
// Errors carry the line they were found on: a 64-bit status word holds atomicMin(line << 8 | code), so the earliest
// line wins, as it does in the reference's sequential loop.  S_UNSUPPORTED means the reference would call
// std::terminate or read an uninitialised number (the caller keeps its host parser); the others are errors the
// reference raises or undefined behaviour it would run into (index 0, an index outside its pool at its line, fewer
// than 3 corners).
#pragma once
#include <cstdint>

#include "tk_common.h"
#include "tk_ply.h"

namespace tk {
namespace obj {

enum LineType : uint8_t { L_NONE = 0, L_V, L_VT, L_VN, L_F3, L_F4, L_FBAD };

enum Code : uint32_t { S_UNSUPPORTED = 1, S_FEW = 2, S_V0 = 3, S_RANGE = 4, S_NGON = 5 };

// per-line counts, scanned: pool slots, face number, first corner
struct Cnt {
    int32_t v, vt, vn, f, c;
};
TK_HD Cnt operator+(const Cnt &a, const Cnt &b) { return Cnt{a.v + b.v, a.vt + b.vt, a.vn + b.vn, a.f + b.f, a.c + b.c}; }
TK_HD Cnt count_of(uint8_t t) {
    return Cnt{t == L_V, t == L_VT, t == L_VN, t == L_F3 || t == L_F4, t == L_F3 ? 3 : t == L_F4 ? 4 : 0};
}

struct Corner {
    int32_t v, vt, vn, face;  // the raw indices as split_face_str makes them, and the face they belong to
};
struct Face {
    int32_t c0, nc;        // first corner, 3 or 4 corners
    int32_t nv, nvt, nvn;  // pool sizes at the face's line
    int32_t line;
};
// a number the device does not convert: file bytes [off, off + len) -> raw pool double `dest`
struct Fix {
    uint64_t off;
    uint32_t len, dest;
};

TK_HD bool is_space(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
TK_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// ---- tokens and lines: host-callable, so that tests/obj_host can run this text without a GPU ----------------------
TK_HD void trim(const uint8_t *b, int64_t &s, int64_t &e) {
    while (s < e && is_space(b[s])) s++;
    while (e > s && is_space(b[e - 1])) e--;
}

// the next whitespace-delimited token of [p, e) (operator>> of a std::string) -> [ts, te)
TK_HD bool next_token(const uint8_t *b, int64_t &p, int64_t e, int64_t &ts, int64_t &te) {
    while (p < e && is_space(b[p])) p++;
    if (p >= e) return false;
    ts = p;
    while (p < e && !is_space(b[p])) p++;
    te = p;
    return true;
}

// the type of the line [s, e): the first token of the trimmed line; for `f`, how many corners follow (counting stops at 5)
TK_HD uint8_t classify_line(const uint8_t *b, int64_t s, int64_t e) {
    int64_t ts = 0, te = 0;
    trim(b, s, e);
    uint8_t t = L_NONE;
    int64_t p = s;
    if (s < e && b[s] != '#' && next_token(b, p, e, ts, te)) {
        const int64_t len = te - ts;
        if (len == 1 && b[ts] == 'v') t = L_V;
        else if (len == 2 && b[ts] == 'v' && b[ts + 1] == 't') t = L_VT;
        else if (len == 2 && b[ts] == 'v' && b[ts + 1] == 'n') t = L_VN;
        else if (len == 1 && b[ts] == 'f') {
            int k = 0;
            while (k < 5 && next_token(b, p, e, ts, te)) k++;
            t = k == 3 ? L_F3 : k == 4 ? L_F4 : L_FBAD;
        }
    }
    return t;
}

// 10^k for k in [0, 22]: the powers of ten a double holds exactly
TK_HD double pow10_exact(int64_t k) {
    static constexpr double t[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                     1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    return t[k];
}

// `ss >> Real` on one token [p, e): 0 = converted exactly into *out, 1 = in the grammar but the host's strtod converts
// it, -1 = not a number num_get would read whole (the file is unsupported)
TK_HD int parse_real(const uint8_t *b, int64_t p, int64_t e, double *out) {
    bool neg = false;
    if (p < e && (b[p] == '+' || b[p] == '-')) neg = b[p++] == '-';
    uint64_t m = 0;
    int64_t nd = 0, zeros = 0, nint = 0, nfrac = 0;  // significant digits so far, trailing zeros not in m yet
    auto digit = [&](int d) {
        if (nd == 0) {
            if (d) m = (uint64_t)d, nd = 1;
        } else if (d == 0) {
            zeros++;
        } else {
            nd += zeros + 1;
            if (nd <= 15) {
                for (int64_t k = 0; k <= zeros; k++) m *= 10;
                m += (uint64_t)d;
            }
            zeros = 0;
        }
    };
    while (p < e && is_digit(b[p])) digit(b[p++] - '0'), nint++;
    if (p < e && b[p] == '.') {
        p++;
        while (p < e && is_digit(b[p])) digit(b[p++] - '0'), nfrac++;
    }
    if (nint == 0 && nfrac == 0) return -1;
    int64_t ex = 0;
    if (p < e && (b[p] == 'e' || b[p] == 'E')) {
        p++;
        bool eneg = false;
        if (p < e && (b[p] == '+' || b[p] == '-')) eneg = b[p++] == '-';
        if (p >= e || !is_digit(b[p])) return -1;
        while (p < e && is_digit(b[p])) {
            ex = ex * 10 + (b[p++] - '0');
            if (ex > 100000000) ex = 100000000;
        }
        if (eneg) ex = -ex;
    }
    if (p != e) return -1;
    if (nd == 0) {  // every digit zero: a signed zero, whatever the exponent
        *out = neg ? -0.0 : 0.0;
        return 0;
    }
    const int64_t E = ex - nfrac + zeros;
    if (nd > 15 || E < -22 || E > 22) return 1;
    double v = (double)m;
    v = E >= 0 ? v * pow10_exact(E) : v / pow10_exact(-E);
    *out = neg ? -v : v;
    return 0;
}

// std::stoi on a non-empty piece [p, e): a leading [+-]?digits (anything behind it ignored), or false where stoi throws
TK_HD bool stoi_prefix(const uint8_t *b, int64_t p, int64_t e, int32_t &v) {
    bool neg = false;
    if (p < e && (b[p] == '+' || b[p] == '-')) neg = b[p++] == '-';
    if (p >= e || !is_digit(b[p])) return false;
    int64_t a = 0;
    while (p < e && is_digit(b[p])) {
        a = a * 10 + (b[p++] - '0');
        if (a > ((int64_t)1 << 32)) a = (int64_t)1 << 32;
    }
    if (neg) a = -a;
    if (a < INT32_MIN || a > INT32_MAX) return false;
    v = (int32_t)a;
    return true;
}

// split_face_str: the pieces between '/' (std::sregex_token_iterator, -1: every piece in front of a '/', and the piece
// behind the last one only if it is not empty), "" -> 0, std::stoi on the others, padded with zeros to three; pieces
// after the third are converted (and can throw) but not kept
TK_HD bool parse_corner(const uint8_t *b, int64_t s, int64_t e, int32_t key[3]) {
    key[0] = key[1] = key[2] = 0;
    int part = 0;
    int64_t p = s;
    while (true) {
        int64_t q = p;
        while (q < e && b[q] != '/') q++;
        const bool last = q >= e;
        if (last && q == p) break;
        int32_t v = 0;
        if (q > p && !stoi_prefix(b, p, q, v)) return false;
        if (part < 3) key[part] = v;
        part++;
        if (last) break;
        p = q + 1;
    }
    return true;
}

#if defined(__HIPCC__)
// ---- three-phase scan: f.load(i) -> T, f.store(i, exclusive prefix) ----------------------------------------------
constexpr int SCAN_BLK = 256, SCAN_IPT = 16;
constexpr int64_t SCAN_TILE = (int64_t)SCAN_BLK * SCAN_IPT;

template <class T> __device__ T block_scan_excl(T x, T &total) {
    __shared__ T sh[SCAN_BLK];
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (int d = 1; d < SCAN_BLK; d <<= 1) {
        const T y = t >= d ? sh[t - d] : T{};
        __syncthreads();
        if (t >= d) sh[t] = sh[t] + y;
        __syncthreads();
    }
    total = sh[SCAN_BLK - 1];
    const T r = t ? sh[t - 1] : T{};
    __syncthreads();
    return r;
}

template <class T, class F> __global__ void __launch_bounds__(SCAN_BLK) k_scan_reduce(F f, int64_t n, T *bsum) {
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_IPT;
    T s{};
    for (int k = 0; k < SCAN_IPT; k++)
        if (base + k < n) s = s + f.load(base + k);
    T total;
    (void)block_scan_excl(s, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: the tile sums -> their exclusive prefixes in place, the grand total behind them (bsum[nb])
template <class T> __global__ void __launch_bounds__(SCAN_BLK) k_scan_blocks(T *bsum, int64_t nb) {
    T carry{};
    for (int64_t b0 = 0; b0 < nb; b0 += SCAN_BLK) {
        const int64_t i = b0 + threadIdx.x;
        T total;
        const T e = block_scan_excl(i < nb ? bsum[i] : T{}, total);
        if (i < nb) bsum[i] = carry + e;
        carry = carry + total;
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

template <class T, class F> __global__ void __launch_bounds__(SCAN_BLK) k_scan_down(F f, int64_t n, const T *bsum) {
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_IPT;
    T s{};
    for (int k = 0; k < SCAN_IPT; k++)
        if (base + k < n) s = s + f.load(base + k);
    T total;
    T run = bsum[blockIdx.x] + block_scan_excl(s, total);
    for (int k = 0; k < SCAN_IPT; k++) {
        if (base + k >= n) break;
        const T x = f.load(base + k);
        f.store(base + k, run);
        run = run + x;
    }
}

// '\n' positions
struct NewlineF {
    const uint8_t *b;
    int32_t *nl;
    __device__ int32_t load(int64_t i) const { return b[i] == '\n'; }
    __device__ void store(int64_t i, int32_t e) const {
        if (b[i] == '\n') nl[e] = (int32_t)i;
    }
};
// line types -> pool slots / face numbers / first corners
struct LineF {
    const uint8_t *type;
    Cnt *pre;
    __device__ Cnt load(int64_t i) const { return count_of(type[i]); }
    __device__ void store(int64_t i, const Cnt &e) const { pre[i] = e; }
};
// first occurrences -> vertex ids
struct FirstF {
    const int32_t *slot, *minseq;
    int32_t *rank;
    __device__ int32_t load(int64_t c) const { return minseq[slot[c]] == (int32_t)c; }
    __device__ void store(int64_t c, int32_t e) const {
        if (minseq[slot[c]] == (int32_t)c) rank[c] = e;
    }
};

// ---- lines -----------------------------------------------------------------------------------------------------
// line i is [s, e): from behind the previous '\n' to the next one (the last line: to the end of the file)
TK_D void line_bounds(const int32_t *nl, int64_t nnl, int64_t n, int64_t i, int64_t &s, int64_t &e) {
    s = i ? (int64_t)nl[i - 1] + 1 : 0;
    e = i < nnl ? (int64_t)nl[i] : n;
}

TK_D void report(unsigned long long *status, int64_t line, uint32_t code) {
    atomicMin(status, ((unsigned long long)line << 8) | code);
}

__global__ void k_obj_classify(const uint8_t *b, int64_t n, const int32_t *nl, int64_t nnl, uint8_t *type) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nnl) return;
    int64_t s, e;
    line_bounds(nl, nnl, n, i, s, e);
    type[i] = classify_line(b, s, e);
}

// per line: the numbers of v / vt / vn lines into the raw pools (v: x y z w, w = 1 unless given; vt: s t; vn: x y z),
// the corners and the face record of f lines
__global__ void k_obj_parse(const uint8_t *b, int64_t n, const int32_t *nl, int64_t nnl, const uint8_t *type, const Cnt *pre,
                            double *raw, int64_t off_vt, int64_t off_vn, Corner *corners, Face *faces, Fix *fix,
                            unsigned int *nfix, unsigned long long *status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nnl) return;
    const uint8_t t = type[i];
    if (t == L_NONE) return;
    int64_t s, e, ts = 0, te = 0;
    line_bounds(nl, nnl, n, i, s, e);
    trim(b, s, e);
    int64_t p = s;
    (void)next_token(b, p, e, ts, te);  // the keyword
    const Cnt c = pre[i];
    if (t == L_V || t == L_VT || t == L_VN) {
        const int need = t == L_VT ? 2 : 3, take = t == L_V ? 4 : need;
        const int64_t base = t == L_V ? 4 * (int64_t)c.v : t == L_VT ? off_vt + 2 * (int64_t)c.vt : off_vn + 3 * (int64_t)c.vn;
        if (t == L_V) raw[base + 3] = 1.0;
        for (int k = 0; k < take; k++) {
            if (!next_token(b, p, e, ts, te)) {
                if (k < need) report(status, i, S_UNSUPPORTED);  // (the reference would read an uninitialised Real)
                break;
            }
            double v = 0;
            const int r = parse_real(b, ts, te, &v);
            if (r < 0) {
                report(status, i, S_UNSUPPORTED);
                break;
            }
            if (r == 0) {
                raw[base + k] = v;
            } else {
                const unsigned int slot = atomicAdd(nfix, 1u);  // (< the number of raw doubles: one record per dest at most)
                fix[slot] = Fix{(uint64_t)ts, (uint32_t)(te - ts), (uint32_t)(base + k)};
            }
        }
        return;
    }
    // f: stoi runs on the first four tokens before the n-gon check (parse_obj.cpp:142-198)
    int32_t key[4][3];
    int k = 0;
    bool ok = true;
    while (k < 5 && next_token(b, p, e, ts, te)) {
        if (k < 4) ok = parse_corner(b, ts, te, key[k]) && ok;
        k++;
    }
    if (!ok) report(status, i, S_UNSUPPORTED);
    if (t == L_FBAD) {
        report(status, i, k < 3 ? S_FEW : S_NGON);
        return;
    }
    const int nc = t == L_F3 ? 3 : 4;
    for (int j = 0; j < nc; j++) corners[c.c + j] = Corner{key[j][0], key[j][1], key[j][2], c.f};
    faces[c.f] = Face{c.c, nc, c.v, c.vt, c.vn, (int32_t)i};
}

__global__ void k_obj_patch(const Fix *fix, const double *val, int64_t n, double *raw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) raw[fix[i].dest] = val[i];
}

// ---- deduplication ---------------------------------------------------------------------------------------------
TK_D uint32_t hash3(int32_t a, int32_t b, int32_t c) {
    uint64_t h = (uint64_t)(uint32_t)a * 0x9E3779B97F4A7C15ull;
    h ^= (uint64_t)(uint32_t)b * 0xC2B2AE3D27D4EB4Full;
    h ^= (uint64_t)(uint32_t)c * 0x165667B19E3779F9ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return (uint32_t)h;
}

// owner[slot]: the first corner that claimed the slot (its key is the slot's key; -1 = empty), minseq[slot]: the
// smallest corner sequence number with that key.  The table has at least twice as many slots as corners, so a probe
// always ends.
__global__ void k_obj_insert(const Corner *cs, int64_t nc, int32_t *owner, int32_t *minseq, uint32_t mask, int32_t *slot) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const Corner k = cs[c];
    uint32_t h = hash3(k.v, k.vt, k.vn) & mask;
    while (true) {
        int32_t o = __hip_atomic_load(&owner[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (o < 0) {
            o = atomicCAS(&owner[h], -1, (int32_t)c);
            if (o < 0) break;
        }
        const Corner q = cs[o];
        if (q.v == k.v && q.vt == k.vt && q.vn == k.vn) break;
        h = (h + 1) & mask;
    }
    atomicMin(&minseq[h], (int32_t)c);
    slot[c] = (int32_t)h;
}

// ---- emit ------------------------------------------------------------------------------------------------------
// per first occurrence: get_vertex_id (parse_obj.cpp:67-112) with the pools as its face line found them.
// counts[0] / [1]: vertices with a vt / a vn (all or none of them, or the arrays would not match positions)
__global__ void __launch_bounds__(256) k_obj_emit(const Corner *cs, int64_t nc, const Face *faces, const int32_t *slot,
                                                  const int32_t *minseq, const int32_t *rank, const double *raw, int64_t off_vt,
                                                  int64_t off_vn, ply::Mat4 X, ply::Mat4 Xi, double *pos, double *nrm, double *uv,
                                                  unsigned long long *status, unsigned int *counts) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool first = c < nc && minseq[slot[c]] == (int32_t)c;
    int has_t = 0, has_n = 0;
    if (first) {
        const Corner k = cs[c];
        const Face f = faces[k.face];
        const int64_t id = rank[c];
        const int64_t iv = k.v > 0 ? (int64_t)k.v - 1 : (int64_t)f.nv + k.v;
        const int64_t it = k.vt > 0 ? (int64_t)k.vt - 1 : (int64_t)f.nvt + k.vt - 1;  // (sic: parse_obj.cpp:95-96)
        const int64_t in = k.vn > 0 ? (int64_t)k.vn - 1 : (int64_t)f.nvn + k.vn;
        uint32_t code = 0;
        if (k.v == 0) code = S_V0;
        else if (iv < 0 || iv >= f.nv || (k.vt != 0 && (it < 0 || it >= f.nvt)) || (k.vn != 0 && (in < 0 || in >= f.nvn))) code = S_RANGE;
        has_t = k.vt != 0, has_n = k.vn != 0;
        if (code) {
            report(status, f.line, code);
        } else {
            const double *r = raw + 4 * iv;
            const double inv_w = 1.0 / r[3];  // (Vector3 / Real: src/vector.h:194-197)
            ply::xform_point(X, r[0] * inv_w, r[1] * inv_w, r[2] * inv_w, pos + 3 * id);
            if (has_t && uv) {
                const double *q = raw + off_vt + 2 * it;
                uv[2 * id + 0] = q[0], uv[2 * id + 1] = 1.0 - q[1];
            }
            if (has_n && nrm) {
                const double *q = raw + off_vn + 3 * in;
                double u[3];
                ply::normalize3(q[0], q[1], q[2], u);  // (the pool holds normalize(Vector3{x, y, z}))
                ply::xform_normal(Xi, u[0], u[1], u[2], nrm + 3 * id);
            }
        }
    }
    const int bt = __syncthreads_count(has_t), bn = __syncthreads_count(has_n);
    if (threadIdx.x == 0) {
        if (bt) atomicAdd(&counts[0], (unsigned int)bt);
        if (bn) atomicAdd(&counts[1], (unsigned int)bn);
    }
}

// per face: one triangle (v0, v1, v2), a quad a second one (v0, v2, v3)
__global__ void k_obj_indices(const Face *faces, int64_t nf, const int32_t *slot, const int32_t *minseq, const int32_t *rank,
                              int32_t *idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf) return;
    const Face f = faces[i];
    const int64_t t0 = (int64_t)f.c0 - 2 * i;
    int32_t v[4] = {0, 0, 0, 0};
    for (int k = 0; k < f.nc; k++) v[k] = rank[minseq[slot[f.c0 + k]]];
    idx[3 * t0 + 0] = v[0], idx[3 * t0 + 1] = v[1], idx[3 * t0 + 2] = v[2];
    if (f.nc == 4) idx[3 * t0 + 3] = v[0], idx[3 * t0 + 4] = v[2], idx[3 * t0 + 5] = v[3];
}
#endif

}  // namespace obj
}  // namespace tk
