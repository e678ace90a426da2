// tk_record_io.h — a wave moves the path records of its 64 lanes as whole lines.
//
// Row-per-lane access (every lane loads its own 128- or 256-byte record with 16-byte loads) makes each wave instruction
// touch 64 different lines for 16 bytes each: every line is requested 8 (16) times on the way in and written in 8 (16)
// pieces on the way out.  Here P = REC_BYTES / 16 lanes share a record instead: in instruction j, lane l moves 16-byte
// piece l % P of the record that lane RPI * j + l / P owns (RPI = 64 / P records per instruction), so one
// global_load_dwordx4 / global_store_dwordx4 covers 8 whole 128-byte lines.  The pieces are transposed through a
// wave-private LDS stage of REC_STAGE_BYTES, filled CHUNK records at a time; the owner of a record ends with (starts
// from) the same registers q[0..P) the row-per-lane form gives it.
//
// The stage is private to the wave: no block barrier, only the order of the wave's own LDS operations (the hardware
// executes them in issue order) and a wave-level fence the compiler respects.  Lanes that own no record (past the end
// of the queue, or not continuing at the handover round) still move their neighbours' pieces; `owned` (a ballot) says
// which records exist, and nothing is read or written for the others.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace tk {

constexpr int REC_STAGE_BYTES = 4096;  // LDS stage per wave (16 KiB per 256-thread block: five blocks per CU keep 80 KiB)

template <int REC_BYTES> struct RecMove {
    static constexpr int P = REC_BYTES / 16;                  // 16-byte pieces per record = lanes that share one
    static constexpr int RPI = 64 / P;                        // records per wave instruction
    static constexpr int N_INSTR = P;                         // wave instructions per 64 records (as row-per-lane)
    static constexpr int CHUNK = REC_STAGE_BYTES / REC_BYTES;  // records per fill of the stage
    static constexpr int IPC = CHUNK / RPI;                   // wave instructions per fill
    static constexpr int CHUNKS = 64 / CHUNK;
    // instruction j, lane l -> (lane that owns the record, piece)
    static constexpr int rec_of(int j, int lane) { return RPI * j + lane / P; }
    static constexpr int piece_of(int lane) { return lane % P; }
    // LDS image of a fill: record rloc (0..CHUNK) in row rloc, its pieces XOR-swizzled with the record index so that
    // the row-per-lane phase (every lane the same piece of its own record) is conflict-free as a ds_read_b128 and as a
    // ds_write_b128, and the cooperative phase (P consecutive lanes one record) stays so
    static constexpr int swz(int rloc) { return P == 8 ? ((rloc ^ (rloc >> 3)) & 7) : (rloc & (P - 1)); }
    static constexpr int lds_off(int rloc, int piece) { return (rloc * P + (piece ^ swz(rloc))) * 16; }
};

namespace recmove_check {
// lane groups that one LDS cycle serves (MI355X): ds_read_b128 4 x 16 lanes over 64 banks, ds_write_b128 8 x 8
// consecutive lanes over 32 banks
constexpr int read128_group(int lane) {
    const int l = lane & 31, g = (l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28)) ? 0 : 1;
    return (lane >> 5) * 2 + g;
}
constexpr int write128_group(int lane) { return lane >> 3; }
// every piece of every record is moved exactly once
template <int REC_BYTES> constexpr bool covers_once() {
    using M = RecMove<REC_BYTES>;
    int seen[64][M::P] = {};
    for (int j = 0; j < M::N_INSTR; j++)
        for (int lane = 0; lane < 64; lane++) {
            const int r = M::rec_of(j, lane), p = M::piece_of(lane);
            if (r < 0 || r >= 64 || p < 0 || p >= M::P) return false;
            if (r / M::CHUNK != j / M::IPC) return false;  // an instruction stays inside the fill of its records
            seen[r][p]++;
        }
    for (int r = 0; r < 64; r++)
        for (int p = 0; p < M::P; p++)
            if (seen[r][p] != 1) return false;
    return true;
}
// the LDS image of a fill has no two pieces at one address, and stays inside the stage
template <int REC_BYTES> constexpr bool image_is_bijective() {
    using M = RecMove<REC_BYTES>;
    bool used[REC_STAGE_BYTES / 16] = {};
    for (int r = 0; r < M::CHUNK; r++)
        for (int p = 0; p < M::P; p++) {
            const int off = M::lds_off(r, p);
            if (off < 0 || off + 16 > REC_STAGE_BYTES || off % 16) return false;
            if (used[off / 16]) return false;
            used[off / 16] = true;
        }
    return true;
}
// no two active lanes of one lane group on one 16-byte bank column (off[lane] < 0: lane inactive)
constexpr bool conflict_free(const int (&off)[64], bool is_read) {
    const int columns = is_read ? 16 : 8;
    int held[8][16] = {};  // [lane group][column]: 1 + the offset of the lane that has it (equal offsets broadcast)
    for (int lane = 0; lane < 64; lane++) {
        if (off[lane] < 0) continue;
        int &h = held[is_read ? read128_group(lane) : write128_group(lane)][(off[lane] / 16) % columns];
        if (h != 0 && h != off[lane] + 1) return false;
        h = off[lane] + 1;
    }
    return true;
}
template <int REC_BYTES> constexpr bool phases_conflict_free() {
    using M = RecMove<REC_BYTES>;
    for (int c = 0; c < M::CHUNKS; c++) {
        // row-per-lane phase: the lanes of fill c, every one piece p of its own record (read on load, write on store)
        for (int p = 0; p < M::P; p++) {
            int off[64] = {};
            for (int lane = 0; lane < 64; lane++) off[lane] = lane / M::CHUNK == c ? M::lds_off(lane - c * M::CHUNK, p) : -1;
            if (!conflict_free(off, true) || !conflict_free(off, false)) return false;
        }
        // cooperative phase: all lanes, instruction j (write on load, read on store)
        for (int jj = 0; jj < M::IPC; jj++) {
            int off[64] = {};
            for (int lane = 0; lane < 64; lane++)
                off[lane] = M::lds_off(M::rec_of(c * M::IPC + jj, lane) - c * M::CHUNK, M::piece_of(lane));
            if (!conflict_free(off, true) || !conflict_free(off, false)) return false;
        }
    }
    return true;
}
static_assert(covers_once<128>() && covers_once<256>(), "every piece of every record is moved exactly once");
static_assert(image_is_bijective<128>() && image_is_bijective<256>(), "the LDS image has no two pieces at one address");
static_assert(phases_conflict_free<128>() && phases_conflict_free<256>(), "ds_write_b128 and ds_read_b128 phases are conflict-free");
}  // namespace recmove_check

// orders the wave's LDS writes before its following LDS reads (and the reverse) for the compiler; the hardware keeps
// one wave's LDS operations in issue order, so no wait and no barrier instruction is needed
__device__ __forceinline__ void wave_stage_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// 16 bytes as the compiler's own vector type: one ds_read_b128 / global_load_dwordx4 that it neither splits nor narrows
typedef uint32_t rec_piece __attribute__((ext_vector_type(4), may_alias));
__device__ __forceinline__ uint4 piece_to_uint4(rec_piece v) { return make_uint4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ rec_piece piece_of_uint4(const uint4 &v) { return rec_piece{v.x, v.y, v.z, v.w}; }
// the wave's stage inside a block's s_stage[BLOCK / 64][REC_STAGE_BYTES / 16]; wave-uniform, so it lives in SGPRs
__device__ __forceinline__ rec_piece *wave_stage(rec_piece *block_stage) {
    return block_stage + __builtin_amdgcn_readfirstlane(threadIdx.x / 64) * (REC_STAGE_BYTES / 16);
}
// the lane index, computed where it is called: what is derived from it is not kept in registers across the caller's
// work between a load and a store
__device__ __forceinline__ int lane_here() {
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    return lane;
}

// q[0..P) of every lane whose bit in `owned` is set = the record of its `slot`; convergent: every lane of the wave calls.
// AHEAD: the loads of the next fill are issued before this fill is transposed (two fills in flight; 16 more registers)
template <int REC_BYTES, bool AHEAD = true>
__device__ __forceinline__ void record_load_coop(const char *base, int32_t slot, uint64_t owned, rec_piece *stage, uint4 (&q)[REC_BYTES / 16]) {
    using M = RecMove<REC_BYTES>;
    const int lane = lane_here();
    const int piece = M::piece_of(lane);
    rec_piece t[M::N_INSTR];
    auto issue = [&](int c) {  // the loads of fill c
#pragma unroll
        for (int jj = 0; jj < M::IPC; jj++) {
            const int j = c * M::IPC + jj;
            const int r = M::rec_of(j, lane);
            const int32_t s = __shfl(slot, r);
            t[j] = rec_piece{0, 0, 0, 0};
            if ((owned >> r) & 1) t[j] = *reinterpret_cast<const rec_piece *>(base + (int64_t)s * REC_BYTES + 16 * piece);
        }
    };
    if (AHEAD) issue(0);
#pragma unroll
    for (int c = 0; c < M::CHUNKS; c++) {
        if (!AHEAD) issue(c);
        else if (c + 1 < M::CHUNKS) issue(c + 1);  // the next fill's loads run under this one's transpose
#pragma unroll
        for (int jj = 0; jj < M::IPC; jj++) {
            const int j = c * M::IPC + jj;
            stage[M::lds_off(M::rec_of(j, lane) - c * M::CHUNK, piece) / 16] = t[j];
        }
        wave_stage_fence();
        if (lane / M::CHUNK == c) {
#pragma unroll
            for (int p = 0; p < M::P; p++) q[p] = piece_to_uint4(stage[M::lds_off(lane - c * M::CHUNK, p) / 16]);
        }
        wave_stage_fence();
    }
}

// the mirror image: the record of every lane whose bit in `owned` is set is written from its q[0..P); no other record
// is touched
template <int REC_BYTES>
__device__ __forceinline__ void record_store_coop(char *base, int32_t slot, uint64_t owned, rec_piece *stage, const uint4 (&q)[REC_BYTES / 16]) {
    using M = RecMove<REC_BYTES>;
    const int lane = lane_here();
    const int piece = M::piece_of(lane);
#pragma unroll
    for (int c = 0; c < M::CHUNKS; c++) {
        if (lane / M::CHUNK == c && ((owned >> lane) & 1)) {
#pragma unroll
            for (int p = 0; p < M::P; p++) stage[M::lds_off(lane - c * M::CHUNK, p) / 16] = piece_of_uint4(q[p]);
        }
        wave_stage_fence();
#pragma unroll
        for (int jj = 0; jj < M::IPC; jj++) {
            const int r = M::rec_of(c * M::IPC + jj, lane);
            const int32_t s = __shfl(slot, r);
            const rec_piece v = stage[M::lds_off(r - c * M::CHUNK, piece) / 16];
            if ((owned >> r) & 1) *reinterpret_cast<rec_piece *>(base + (int64_t)s * REC_BYTES + 16 * piece) = v;
        }
        wave_stage_fence();
    }
}

}  // namespace tk
