// adaptive_host.cpp — TEST INFRASTRUCTURE.  The per-pixel functions of take_amd/csrc/tk_adaptive.h built for the host:
// the stopping rule, the moments, the work-list index arithmetic and the ordered compaction run serially in the
// kernels' order, so that tests/test_adaptive_cpu.py can hold the text the device runs to the numpy restatement
// (tests/adaptive_ref.py) without a GPU.  Never loaded by the product.
#include <cstdint>

#include "take_hip.h"
#include "tk_adaptive.h"

extern "C" {
// err[i] and stop[i] of (n[i], m1[i], m2[i]) under (spp, threshold, floor)
void adaptive_host_test(int64_t count, const int32_t *n, const double *m1, const double *m2, int32_t spp, double threshold, double floor, double *err,
                        int32_t *stop) {
    const tk::ad::Rule rule{spp, 0, 0, threshold, floor};
    for (int64_t i = 0; i < count; i++) {
        err[i] = tk::ad::rel_error(n[i], m1[i], m2[i], floor);
        stop[i] = tk::ad::stops(rule, n[i], err[i]) ? 1 : 0;
    }
}
// the moments of the samples rgb[s][3] (already double), added in order to m[0], m[1]
void adaptive_host_moments(int64_t n_samples, const double *rgb, double *m) {
    for (int64_t s = 0; s < n_samples; s++) tk::ad::add_moments(tk::ad::sample_value(rgb[3 * s], rgb[3 * s + 1], rgb[3 * s + 2]), m[0], m[1]);
}
// the ordered compaction (list may be null: the identity); mask, base: (n + 63) / 64 words -> the next list's length
int32_t adaptive_host_compact(const uint8_t *keep, const int32_t *list, int64_t n, int32_t threads, uint64_t *mask, int32_t *base, int32_t *out) {
    return tk::ad::compact_serial(keep, list, n, threads, mask, base, out);
}
// the work list of a pass: slot[j] for j < nb * n_active, as k_generate_list computes it (reciprocal divisor)
void adaptive_host_worklist(const int32_t *list, int32_t n_active, int32_t nb, int32_t npix, int64_t *slot) {
    const double inv = 1.0 / (double)n_active;
    for (int64_t j = 0; j < (int64_t)nb * n_active; j++) {
        uint32_t sample, idx;
        tk::ad::list_entry((uint32_t)j, (uint32_t)n_active, inv, sample, idx);
        slot[j] = tk::ad::slot_of(sample, list[idx], npix);
    }
}
}
