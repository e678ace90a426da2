// tk_adaptive.h — per-pixel adaptive sampling (include/take_hip.h: take_hip_render_adaptive*; specification:
// DESIGN.md §4g): a pixel stops receiving samples once the relative standard error of its mean is at or below a
// threshold.  The samples themselves are the render's own — a pass puts the slots sample * npix + pixel of the pixels
// still active into the round-0 extend queue, and trace, sort, shade and shadow run on that queue as they are — so a
// pixel that stops at c samples is, bit for bit, that pixel of take_hip_render(spp = c).
// The per-pixel functions below are TK_HD and written once: the kernels at the end of this file run them on the device,
// tests/adaptive_host runs the same text on the host, tests/adaptive_ref.py restates the rule in numpy.  Launched from
// tk_render.hip (the driver shares Frame, launch_round and QueuePoll with the render loop).
//
// Arithmetic: moments and test are double whatever the scene's precision; every + - * / sqrt is one operation in the
// order written (-ffp-contract=off; double / and sqrt are correctly rounded on the device as on the host).
#pragma once
#include <cstdint>

#include "tk_integrate.h"

namespace tk {
namespace ad {

// TakeAdaptiveOpts with the defaults filled in and min_spp clamped to the render's spp (= the maximum per pixel)
struct Rule {
    int32_t spp, min_spp, step_spp;
    double threshold, floor;
};

// ---- the moments: L_s = (r + g) + b of the sample as the image sums take it; m1 += L_s, m2 += L_s * L_s in sample order
TK_HD double sample_value(double r, double g, double b) { return (r + g) + b; }
TK_HD void add_moments(double L, double &m1, double &m2) {
    m1 = m1 + L;
    m2 = m2 + L * L;
}

// ---- the test after a pass, for a pixel with n samples: the relative standard error of the mean.  n == 1 divides by
// zero (inf or NaN: such a pixel never stops on err); a NaN anywhere comes out as NaN.
TK_HD double rel_error(int32_t n, double m1, double m2, double floor) {
    const double dn = (double)n;
    const double mean = m1 / dn;
    double v = m2 / dn - mean * mean;
    v = v > 0.0 ? v : 0.0;
    return tk_sqrt(v / (dn - 1.0)) / (tk_fabs(mean) + floor);
}
// (a NaN err never satisfies <=: the pixel runs to spp)
TK_HD bool stops(const Rule &rule, int32_t n, double err) { return (n >= 2 && err <= rule.threshold) || n == rule.spp; }

// ---- the work list of a pass: entry j < nb * n_active is sample j / n_active of the batch and listed pixel
// j % n_active (sample-major, as the slots of a full batch are; neighbouring listed pixels in neighbouring lanes),
// with the reciprocal of the launch-invariant divisor (divmod_u31)
TK_HD void list_entry(uint32_t j, uint32_t n_active, double inv_n_active, uint32_t &sample, uint32_t &idx) {
    divmod_u31(j, n_active, inv_n_active, sample, idx);
}
// the path slot of (sample of the batch, local pixel): the address of its record, whoever is on the list
TK_HD int64_t slot_of(uint32_t sample, int32_t pixel, int32_t npix) { return (int64_t)sample * npix + pixel; }
// listed pixel idx of `list` (null: the identity — pass 0 is over all pixels)
TK_HD int32_t listed(const int32_t *list, int64_t idx) { return list ? list[idx] : (int32_t)idx; }

// ---- ordered compaction of the kept pixels into the next list, without atomics: the keep flags of 64 consecutive
// list entries are one mask word (k_adaptive_select: a wave's ballot); one block scans the words' bit counts
// (k_compact_scan: thread t owns the run scan_run gives it) into base[word]; entry j goes to base[j / 64] + the kept
// entries below it in its word (k_compact_scatter).  Ascending in, ascending out; the same list in every run.
constexpr int GROUP = 64;
constexpr int SCAN_THREADS = 1024;
TK_HD int64_t groups_of(int64_t n) { return (n + GROUP - 1) / GROUP; }
TK_HD int32_t bits_of(uint64_t mask) { return (int32_t)__builtin_popcountll(mask); }
TK_HD bool kept(uint64_t mask, int lane) { return ((mask >> lane) & 1ull) != 0; }
TK_HD int32_t rank_below(uint64_t mask, int lane) { return bits_of(mask & ((1ull << lane) - 1ull)); }
// the run [lo, hi) of the `total` mask words that thread t of `threads` sums and then numbers
TK_HD void scan_run(int64_t total, int threads, int t, int64_t &lo, int64_t &hi) {
    const int64_t per = (total + threads - 1) / threads;
    lo = (int64_t)t * per < total ? (int64_t)t * per : total;
    hi = lo + per < total ? lo + per : total;
}
TK_HD int32_t run_sum(const uint64_t *mask, int64_t lo, int64_t hi) {
    int32_t s = 0;
    for (int64_t g = lo; g < hi; g++) s += bits_of(mask[g]);
    return s;
}
// base[g] of the run, from the exclusive prefix of the runs before it -> that prefix plus the run's sum
TK_HD int32_t run_number(const uint64_t *mask, int64_t lo, int64_t hi, int32_t prefix, int32_t *base) {
    for (int64_t g = lo; g < hi; g++) {
        base[g] = prefix;
        prefix += bits_of(mask[g]);
    }
    return prefix;
}
// entry j of the list -> its place in the next list (only for a kept entry)
TK_HD int32_t compact_dest(const uint64_t *mask, const int32_t *base, int64_t j) {
    return base[j / GROUP] + rank_below(mask[j / GROUP], (int)(j % GROUP));
}

// The compaction as the three kernels run it, serially (the host build of tests/adaptive_host): keep[j] != 0 keeps
// listed(list, j).  mask, base: groups_of(n) words each; out: n entries -> the length of the next list.
inline int32_t compact_serial(const uint8_t *keep, const int32_t *list, int64_t n, int threads, uint64_t *mask, int32_t *base, int32_t *out) {
    const int64_t n_groups = groups_of(n);
    for (int64_t g = 0; g < n_groups; g++) {  // (a wave's ballot, lanes beyond n voting no)
        uint64_t m = 0;
        for (int l = 0; l < GROUP; l++)
            if (g * GROUP + l < n && keep[g * GROUP + l]) m |= 1ull << l;
        mask[g] = m;
    }
    int32_t prefix = 0;
    for (int t = 0; t < threads; t++) {
        int64_t lo, hi;
        scan_run(n_groups, threads, t, lo, hi);
        prefix = run_number(mask, lo, hi, prefix, base);
    }
    for (int64_t j = 0; j < n; j++)
        if (kept(mask[j / GROUP], (int)(j % GROUP))) out[compact_dest(mask, base, j)] = listed(list, j);
    return prefix;
}

#if defined(__HIPCC__)
// These are streaming kernels, one lane per listed pixel (or per work-list entry); none keeps more than a handful of
// values live.  BLOCK, WAVE and lane_id are tk_kernels.h's, which the one unit that compiles this includes first.

// Round 0 of a pass over the listed pixels: the initial records of samples s0 .. s0 + nb - 1 (rp) of each, and the
// extend queue.  (Pass 0 is a full batch and takes the render's own start_batch.)
template <class R>
__global__ void __launch_bounds__(BLOCK)
k_generate_list(DeviceScene<R> sc, RenderParams<R> rp, PathState<R> st, const int32_t *__restrict__ list, int32_t n_active, double inv_n_active,
                int32_t *queue, int64_t n) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * BLOCK) {
        uint32_t sample, idx;
        list_entry((uint32_t)j, (uint32_t)n_active, inv_n_active, sample, idx);
        const int64_t slot = slot_of(sample, list[idx], rp.npix);
        generate_path_as<R, false>(sc, rp, st, slot);
        queue[j] = (int32_t)slot;
    }
}
// the same for a scene with a lens (CameraRec::lens_radius > 0): the host picks (adaptive_impl)
template <class R>
__global__ void __launch_bounds__(BLOCK)
k_generate_list_lens(DeviceScene<R> sc, RenderParams<R> rp, PathState<R> st, const int32_t *__restrict__ list, int32_t n_active, double inv_n_active,
                     int32_t *queue, int64_t n) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * BLOCK) {
        uint32_t sample, idx;
        list_entry((uint32_t)j, (uint32_t)n_active, inv_n_active, sample, idx);
        const int64_t slot = slot_of(sample, list[idx], rp.npix);
        generate_path_as<R, true>(sc, rp, st, slot);
        queue[j] = (int32_t)slot;
    }
}

// k_accumulate's additions for the listed pixels, plus the moments and the count.  (The record reads are strided by
// PATH_REC Reals between neighbouring pixels, as k_accumulate's are: three words of every record line.)
template <class R>
__global__ void __launch_bounds__(BLOCK)
k_accumulate_stats(PathState<R> st, R *accum, int32_t *count, double *m1, double *m2, const int32_t *__restrict__ list, int32_t n_active,
                   int32_t npix, int32_t nb) {
    for (int32_t j = blockIdx.x * BLOCK + threadIdx.x; j < n_active; j += gridDim.x * BLOCK) {
        const int32_t p = listed(list, j);
        R r = accum[3 * (int64_t)p], g = accum[3 * (int64_t)p + 1], b = accum[3 * (int64_t)p + 2];
        double s1 = m1[p], s2 = m2[p];
        for (int s = 0; s < nb; s++) {
            const int64_t slot = slot_of((uint32_t)s, p, npix);
            const R lr = st.R_(S_LX, slot), lg = st.R_(S_LY, slot), lb = st.R_(S_LZ, slot);
            r = r + lr;
            g = g + lg;
            b = b + lb;
            add_moments(sample_value((double)lr, (double)lg, (double)lb), s1, s2);
        }
        accum[3 * (int64_t)p] = r;
        accum[3 * (int64_t)p + 1] = g;
        accum[3 * (int64_t)p + 2] = b;
        m1[p] = s1, m2[p] = s2;
        count[p] += nb;
    }
}
// ... k_accumulate_mixed's: a sample's channels are the doubles a + (conv ? (double)b : 0) that kernel adds
__global__ void __launch_bounds__(BLOCK)
k_accumulate_stats_mixed(PathState<double> a, PathState<float> b, double *accum, int32_t *count, double *m1, double *m2,
                         const int32_t *__restrict__ list, int32_t n_active, int32_t npix, int32_t nb) {
    for (int32_t j = blockIdx.x * BLOCK + threadIdx.x; j < n_active; j += gridDim.x * BLOCK) {
        const int32_t p = listed(list, j);
        double r = accum[3 * (int64_t)p], g = accum[3 * (int64_t)p + 1], bl = accum[3 * (int64_t)p + 2];
        double s1 = m1[p], s2 = m2[p];
        for (int s = 0; s < nb; s++) {
            const int64_t slot = slot_of((uint32_t)s, p, npix);
            const bool conv = a.I_(S_CONV, slot) != 0;
            const float bx = b.R_(S_LX, slot), by = b.R_(S_LY, slot), bz = b.R_(S_LZ, slot);
            const double lr = a.R_(S_LX, slot) + (conv ? (double)bx : 0.0);
            const double lg = a.R_(S_LY, slot) + (conv ? (double)by : 0.0);
            const double lb = a.R_(S_LZ, slot) + (conv ? (double)bz : 0.0);
            r = r + lr;
            g = g + lg;
            bl = bl + lb;
            add_moments(sample_value(lr, lg, lb), s1, s2);
        }
        accum[3 * (int64_t)p] = r;
        accum[3 * (int64_t)p + 1] = g;
        accum[3 * (int64_t)p + 2] = bl;
        m1[p] = s1, m2[p] = s2;
        count[p] += nb;
    }
}

// The test on every listed pixel; the keep flags of a wave are one mask word.  One lane per entry, the grid covers
// n_active: every lane of a wave reaches the ballot, those beyond the list vote no.
__global__ void __launch_bounds__(BLOCK)
k_adaptive_select(Rule rule, const int32_t *__restrict__ count, const double *__restrict__ m1, const double *__restrict__ m2,
                  const int32_t *__restrict__ list, int32_t n_active, uint64_t *mask) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    bool keep = false;
    if (j < n_active) {
        const int32_t p = listed(list, j);
        const int32_t n = count[p];
        keep = !stops(rule, n, rel_error(n, m1[p], m2[p], rule.floor));
    }
    const uint64_t m = __ballot(keep);
    if (lane_id() == 0 && j < n_active) mask[j / GROUP] = m;
}
// One block: base[word] = kept entries before the word; *n_next = all of them.
__global__ void __launch_bounds__(SCAN_THREADS) k_compact_scan(const uint64_t *__restrict__ mask, int64_t n_groups, int32_t *base, int32_t *n_next) {
    __shared__ int32_t s_sum[SCAN_THREADS];
    int64_t lo, hi;
    scan_run(n_groups, SCAN_THREADS, (int)threadIdx.x, lo, hi);
    const int32_t sum = run_sum(mask, lo, hi);
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {  // Hillis-Steele inclusive scan of the runs' sums
        const int32_t v = (int)threadIdx.x >= off ? s_sum[threadIdx.x - off] : 0;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    (void)run_number(mask, lo, hi, s_sum[threadIdx.x] - sum, base);
    if (threadIdx.x == SCAN_THREADS - 1) *n_next = s_sum[SCAN_THREADS - 1];
}
__global__ void __launch_bounds__(BLOCK)
k_compact_scatter(const int32_t *__restrict__ list, const uint64_t *__restrict__ mask, const int32_t *__restrict__ base, int32_t n_active,
                  int32_t *next) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < n_active; j += (int64_t)gridDim.x * BLOCK)
        if (kept(mask[j / GROUP], (int)(j % GROUP))) next[compact_dest(mask, base, j)] = listed(list, j);
}

// k_resolve with the pixel's own count in place of spp: sum * (1 / count), the local rows flipped into increasing image
// row; the count and moment planes the caller asked for, flipped the same way.
template <class R>
__global__ void __launch_bounds__(BLOCK)
k_resolve_adaptive(const R *__restrict__ accum, const int32_t *__restrict__ count, const double *__restrict__ m1, const double *__restrict__ m2, R *out,
                   int32_t *count_out, double *m1_out, double *m2_out, int32_t width, int32_t n_local_rows) {
    const int32_t npix = width * n_local_rows;
    for (int32_t p = blockIdx.x * BLOCK + threadIdx.x; p < npix; p += gridDim.x * BLOCK) {
        const int lr = p / width, x = p % width;
        const int64_t q = (int64_t)(n_local_rows - 1 - lr) * width + x;
        const int32_t c = count[p];
        const R inv = R(1) / R(c);
        out[3 * q] = accum[3 * (int64_t)p] * inv;
        out[3 * q + 1] = accum[3 * (int64_t)p + 1] * inv;
        out[3 * q + 2] = accum[3 * (int64_t)p + 2] * inv;
        if (count_out) count_out[q] = c;
        if (m1_out) m1_out[q] = m1[p];
        if (m2_out) m2_out[q] = m2[p];
    }
}
#endif  // __HIPCC__

}  // namespace ad
}  // namespace tk
