// Micro-benchmark: what does the access SHAPE of the shade kernel's path-record traffic cost?
// A 1 GiB array of 128-byte (f32) or 256-byte (f64) records — four times the Infinity Cache — is visited through a queue
// of ascending slots that keeps a fraction p of the slots, in runs of 100..250 neighbours (the queues of a render,
// DESIGN.md §7).  Every queued record is loaded, the first word of each 16-byte piece is incremented, and the record is
// stored back: the shade kernel's record traffic without its arithmetic.  Three shapes:
//   (a) row-per-lane: every lane loads and stores its own record with 16-byte accesses (k_shade with
//       TAKE_HIP_SHADE_COOP=0)
//   (b) 8 (16) lanes per record, whole lines per wave instruction, transposed through a wave-private LDS stage — the
//       code of take_amd/csrc/tk_record_io.h itself
//   (c) the same accesses, transposed by cross-lane permutes, no LDS
// at 5 and at 8 resident blocks per CU (5 = the f32 Diffuse shade instance).  Prints GB/s of record bytes (read +
// written; the 4-byte queue entries are not counted) and checks every word of the array after each run.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/ubench_records tools/ubench_records.hip && tools/ubench_records
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../take_amd/csrc/tk_record_io.h"

#define CK(x)                                                       \
    do {                                                            \
        hipError_t e_ = (x);                                        \
        if (e_ != hipSuccess) {                                     \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
            return 1;                                               \
        }                                                           \
    } while (0)

constexpr size_t ARRAY_BYTES = (size_t)1 << 30;
constexpr int BLOCK = 256;

// ---- shape (c): the transposition as butterfly exchanges between a bit of the register index and a bit of the lane.
// t[4 * i + d]: dword d of 16-byte register i
template <int K, int M, int N> __device__ __forceinline__ void exchange(uint32_t (&t)[N]) {
    const bool hi = ((threadIdx.x >> M) & 1) != 0;
#pragma unroll
    for (int w = 0; w < N; w++) {
        if ((w / 4) & (1 << K)) continue;
        const int w1 = w + 4 * (1 << K);
        const uint32_t got = __shfl_xor(hi ? t[w] : t[w1], 1 << M);
        t[w] = hi ? got : t[w];
        t[w1] = hi ? t[w1] : got;
    }
}
template <int N> __device__ __forceinline__ void lane_permute(uint32_t (&t)[N], int src) {
#pragma unroll
    for (int w = 0; w < N; w++) t[w] = __shfl(t[w], src);
}
// register j of lane l = piece l % P of record RPI * j + l / P   <->   register p of lane r = piece p of record r
template <int REC, bool TO_ROWS> __device__ __forceinline__ void transpose_permute(uint32_t (&t)[REC / 4]) {
    const int lane = threadIdx.x & 63;
    if constexpr (REC == 128) {
        if constexpr (TO_ROWS) {
            exchange<0, 3>(t), exchange<1, 4>(t), exchange<2, 5>(t);
            exchange<0, 0>(t), exchange<1, 1>(t), exchange<2, 2>(t);
        } else {
            exchange<2, 2>(t), exchange<1, 1>(t), exchange<0, 0>(t);
            exchange<2, 5>(t), exchange<1, 4>(t), exchange<0, 3>(t);
        }
    } else {
        if constexpr (TO_ROWS) {
            exchange<0, 0>(t), exchange<1, 1>(t), exchange<2, 2>(t), exchange<3, 3>(t);
            lane_permute(t, ((lane & 3) << 4) | (lane >> 2));
        } else {
            lane_permute(t, ((lane & 15) << 2) | (lane >> 4));
            exchange<3, 3>(t), exchange<2, 2>(t), exchange<1, 1>(t), exchange<0, 0>(t);
        }
    }
}

template <int REC, int SHAPE>
__global__ void __launch_bounds__(BLOCK) k_touch(char *recs, const int32_t *__restrict__ queue, int32_t n) {
    using M = tk::RecMove<REC>;
    constexpr int P = REC / 16;
    const int32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (blockIdx.x * BLOCK >= n) return;
    const bool own = i < n;
    const int32_t slot = own ? queue[i] : 0;
    const uint64_t owned = __ballot(own);
    const int lane = threadIdx.x & 63;
    if constexpr (SHAPE == 0) {
        if (own) {
            uint4 q[P];
            uint4 *rec = reinterpret_cast<uint4 *>(recs + (int64_t)slot * REC);
#pragma unroll
            for (int p = 0; p < P; p++) q[p] = rec[p];
#pragma unroll
            for (int p = 0; p < P; p++) q[p] = make_uint4(q[p].x + 1, q[p].y, q[p].z, q[p].w);
#pragma unroll
            for (int p = 0; p < P; p++) rec[p] = q[p];
        }
    } else if constexpr (SHAPE == 1) {
        __shared__ tk::rec_piece s_stage[BLOCK / 64][tk::REC_STAGE_BYTES / 16];
        tk::rec_piece *stage = tk::wave_stage(&s_stage[0][0]);
        uint4 q[P];
        tk::record_load_coop<REC>(recs, slot, owned, stage, q);
        if (own) {
#pragma unroll
            for (int p = 0; p < P; p++) q[p] = make_uint4(q[p].x + 1, q[p].y, q[p].z, q[p].w);
        }
        tk::record_store_coop<REC>(recs, slot, owned, stage, q);
    } else {
        const int piece = M::piece_of(lane);
        uint32_t t[4 * P];
#pragma unroll
        for (int j = 0; j < P; j++) {
            const int r = M::rec_of(j, lane);
            const int32_t s = __shfl(slot, r);
            uint4 v = make_uint4(0, 0, 0, 0);
            if ((owned >> r) & 1) v = *reinterpret_cast<const uint4 *>(recs + (int64_t)s * REC + 16 * piece);
            t[4 * j] = v.x, t[4 * j + 1] = v.y, t[4 * j + 2] = v.z, t[4 * j + 3] = v.w;
        }
        transpose_permute<REC, true>(t);
        if (own) {
#pragma unroll
            for (int p = 0; p < P; p++) t[4 * p] += 1;
        }
        transpose_permute<REC, false>(t);
#pragma unroll
        for (int j = 0; j < P; j++) {
            const int r = M::rec_of(j, lane);
            const int32_t s = __shfl(slot, r);
            if ((owned >> r) & 1)
                *reinterpret_cast<uint4 *>(recs + (int64_t)s * REC + 16 * piece) = make_uint4(t[4 * j], t[4 * j + 1], t[4 * j + 2], t[4 * j + 3]);
        }
    }
}

__global__ void k_init(uint32_t *words, size_t n) {
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < n; w += (size_t)gridDim.x * blockDim.x) words[w] = (uint32_t)w * 2654435761u;
}
// every word is what k_init wrote, plus `launches` in the first word of each piece of a queued record
__global__ void k_check(const uint32_t *words, size_t n, const uint8_t *queued, int rec_words, uint32_t launches, unsigned long long *bad) {
    unsigned long long mine = 0;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < n; w += (size_t)gridDim.x * blockDim.x) {
        const uint32_t want = (uint32_t)w * 2654435761u + ((w % 4 == 0 && queued[w / rec_words]) ? launches : 0u);
        mine += words[w] != want;
    }
    if (mine) atomicAdd(bad, mine);
}

struct Queue {
    std::vector<int32_t> slots;
    std::vector<uint8_t> queued;
};
// ascending slots, a fraction p of [0, n_slots) kept in runs of 100..250 neighbours
static Queue make_queue(int64_t n_slots, double p) {
    Queue q;
    q.queued.assign((size_t)n_slots, 0);
    uint32_t s = 12345;
    int64_t at = 0;
    while (at < n_slots) {
        s = s * 1664525u + 1013904223u;
        const int64_t run = 100 + (s >> 8) % 151;
        for (int64_t k = at; k < std::min(at + run, n_slots); k++) q.slots.push_back((int32_t)k), q.queued[(size_t)k] = 1;
        at += run + (p < 1.0 ? (int64_t)(run * (1.0 - p) / p + 0.5) : 0);
    }
    return q;
}

template <int REC, int SHAPE>
static int run(char *d_recs, const Queue &q, const int32_t *d_queue, const uint8_t *d_queued, unsigned long long *d_bad, double p, int blocks_per_cu) {
    const int32_t n = (int32_t)q.slots.size();
    const int grid = (n + BLOCK - 1) / BLOCK;
    // occupancy: pad the block's LDS to 160 KiB / blocks_per_cu with a dynamic allocation nobody touches
    const size_t stat = SHAPE == 1 ? (size_t)(BLOCK / 64) * tk::REC_STAGE_BYTES : 0;
    const size_t dyn = (size_t)160 * 1024 / blocks_per_cu - stat - 64;
    constexpr int LAUNCHES = 6;
    hipEvent_t ev[LAUNCHES + 1];
    for (auto &e : ev) CK(hipEventCreate(&e));
    k_init<<<4096, 256>>>((uint32_t *)d_recs, ARRAY_BYTES / 4);
    CK(hipMemset(d_bad, 0, 8));
    for (int l = 0; l < LAUNCHES; l++) {
        CK(hipEventRecord(ev[l]));
        k_touch<REC, SHAPE><<<grid, BLOCK, dyn>>>(d_recs, d_queue, n);
    }
    CK(hipEventRecord(ev[LAUNCHES]));
    CK(hipGetLastError());
    k_check<<<4096, 256>>>((const uint32_t *)d_recs, ARRAY_BYTES / 4, d_queued, REC / 4, LAUNCHES, d_bad);
    CK(hipDeviceSynchronize());
    unsigned long long bad = 0;
    CK(hipMemcpy(&bad, d_bad, 8, hipMemcpyDeviceToHost));
    std::vector<float> ms;
    for (int l = 1; l < LAUNCHES; l++) {  // the first launch warms up
        float t = 0;
        CK(hipEventElapsedTime(&t, ev[l], ev[l + 1]));
        ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    const double bytes = 2.0 * n * REC;
    printf("rec=%3dB p=%.2f blocks/CU=%d shape=%c : %7.1f GB/s median  (%7.1f best, %7.1f worst; %d records, %s)\n", REC, p, blocks_per_cu,
           "abc"[SHAPE], bytes / ms[ms.size() / 2] * 1e-6, bytes / ms.front() * 1e-6, bytes / ms.back() * 1e-6, n,
           bad ? "WRONG WORDS" : "all words right");
    fflush(stdout);
    for (auto &e : ev) CK(hipEventDestroy(e));
    return bad ? 1 : 0;
}

template <int REC> static int run_size(char *d_recs, unsigned long long *d_bad) {
    const int64_t n_slots = (int64_t)(ARRAY_BYTES / REC);
    for (double p : {1.0, 0.5, 0.25, 0.1}) {
        const Queue q = make_queue(n_slots, p);
        int32_t *d_queue;
        uint8_t *d_queued;
        CK(hipMalloc(&d_queue, q.slots.size() * 4));
        CK(hipMalloc(&d_queued, q.queued.size()));
        CK(hipMemcpy(d_queue, q.slots.data(), q.slots.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(d_queued, q.queued.data(), q.queued.size(), hipMemcpyHostToDevice));
        for (int bpc : {5, 8}) {
            if (run<REC, 0>(d_recs, q, d_queue, d_queued, d_bad, p, bpc)) return 1;
            if (run<REC, 1>(d_recs, q, d_queue, d_queued, d_bad, p, bpc)) return 1;
            if (run<REC, 2>(d_recs, q, d_queue, d_queued, d_bad, p, bpc)) return 1;
        }
        CK(hipFree(d_queue));
        CK(hipFree(d_queued));
        printf("\n");
    }
    return 0;
}

int main() {
    char *d_recs;
    unsigned long long *d_bad;
    CK(hipMalloc(&d_recs, ARRAY_BYTES));
    CK(hipMalloc(&d_bad, 8));
    if (run_size<128>(d_recs, d_bad)) return 1;
    if (run_size<256>(d_recs, d_bad)) return 1;
    return 0;
}
