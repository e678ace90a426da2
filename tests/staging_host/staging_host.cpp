// TEST INFRASTRUCTURE: the host logic of StagedPlanes and with_real (take_amd/csrc/tk_host.h) without a device.  The
// HIP calls they make — hipMalloc, hipMemcpy, hipFree — are defined here over the host heap and keep a log, so that a
// sanitizer build sees every byte a plane's copy touches: which planes are present, their byte counts, the order of
// the allocations and copies, what a failed allocation leaves behind.  Prints "ok" and returns 0, or says what
// differs and returns 1.  Not part of the product.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tk_host.h"

namespace {
struct Call {
    char op;  // 'a'lloc, 'u'pload, 'd'ownload, 'f'ree
    size_t bytes;
    const void *dev;
    bool operator==(const Call &o) const { return op == o.op && bytes == o.bytes && dev == o.dev; }
};
std::vector<Call> g_log;
long g_fail_malloc = 0;  // the k-th hipMalloc from now fails (0: none)
int g_failures = 0;

void expect(bool ok, const char *what, int line) {
    if (ok) return;
    std::printf("line %d: %s\n", line, what);
    g_failures++;
}
#define EXPECT(cond) expect((cond), #cond, __LINE__)
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) {
    if (g_fail_malloc > 0 && --g_fail_malloc == 0) return hipErrorOutOfMemory;
    *p = std::malloc(bytes);
    g_log.push_back({'a', bytes, *p});
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    g_log.push_back({'f', 0, p});
    std::free(p);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    g_log.push_back({kind == hipMemcpyHostToDevice ? 'u' : 'd', bytes, kind == hipMemcpyHostToDevice ? dst : src});
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stub"; }
}

using namespace tk_host;

int main() {
    constexpr size_t NPIX = 7;
    // every kind of plane, present and absent; host arrays exactly as large as their planes
    std::vector<char> in3(NPIX * 3, 1), in8(NPIX * 8, 2), inout_from(NPIX * 4, 3), inout_to(NPIX * 4, 0), out12(NPIX * 12, 0), orphan(NPIX * 4, 9);
    {
        g_log.clear();
        StagedPlanes<8> st{{plane_in(in3.data(), 3), plane_in(nullptr, 5), plane_out(out12.data(), 12), plane_out(nullptr, 16), plane_inout(inout_from.data(), inout_to.data(), 4),
                            plane_inout(nullptr, orphan.data(), 4), plane_inout(in8.data(), nullptr, 8), plane_in(nullptr, 0)}};
        EXPECT(st.alloc(NPIX, "no memory") == TAKE_OK);
        // present: 0, 2, 4, 6 — in the order of the table, with the table's bytes per pixel
        const std::vector<Call> allocs{{'a', NPIX * 3, st[0]}, {'a', NPIX * 12, st[2]}, {'a', NPIX * 4, st[4]}, {'a', NPIX * 8, st[6]}};
        EXPECT(g_log == allocs);
        EXPECT(st[0] && st[2] && st[4] && st[6]);
        EXPECT(!st[1] && !st[3] && !st[5] && !st[7]);
        g_log.clear();
        EXPECT(st.upload() == TAKE_OK);
        const std::vector<Call> uploads{{'u', NPIX * 3, st[0]}, {'u', NPIX * 4, st[4]}, {'u', NPIX * 8, st[6]}};
        EXPECT(g_log == uploads);
        EXPECT(std::memcmp(st[0], in3.data(), in3.size()) == 0 && std::memcmp(st[4], inout_from.data(), inout_from.size()) == 0 &&
               std::memcmp(st[6], in8.data(), in8.size()) == 0);
        // "the device call": writes the output plane, changes the in-place one
        std::memset(st[2], 5, NPIX * 12);
        std::memset(st[4], 6, NPIX * 4);
        g_log.clear();
        EXPECT(st.download() == TAKE_OK);
        const std::vector<Call> downloads{{'d', NPIX * 12, st[2]}, {'d', NPIX * 4, st[4]}};
        EXPECT(g_log == downloads);
        EXPECT(out12 == std::vector<char>(NPIX * 12, 5) && inout_to == std::vector<char>(NPIX * 4, 6));
        EXPECT(inout_from == std::vector<char>(NPIX * 4, 3) && orphan == std::vector<char>(NPIX * 4, 9));  // inputs and absent planes: untouched
        g_log.clear();
    }
    EXPECT(g_log.size() == 4);  // every plane freed with its owner
    for (const Call &c : g_log) EXPECT(c.op == 'f');

    // no pixels (an empty strip set): nothing is allocated, copied or written, every device pointer is null
    {
        g_log.clear();
        StagedPlanes<3> st{{plane_in(in3.data(), 3), plane_out(out12.data(), 12), plane_inout(inout_from.data(), inout_to.data(), 4)}};
        EXPECT(st.alloc(0, "no memory") == TAKE_OK && st.upload() == TAKE_OK && st.download() == TAKE_OK);
        EXPECT(!st[0] && !st[1] && !st[2]);
    }
    EXPECT(g_log.empty());

    // the device refuses the second allocation: TAKE_E_NOMEM with the caller's message, the first plane is freed, the third never asked for
    {
        g_log.clear();
        g_fail_malloc = 2;
        StagedPlanes<3> st{{plane_in(in3.data(), 3), plane_out(out12.data(), 12), plane_in(in8.data(), 8)}};
        EXPECT(st.alloc(NPIX, "out of device memory for the planes") == TAKE_E_NOMEM);
        EXPECT(g_error == "out of device memory for the planes");
        EXPECT(g_log.size() == 1 && g_log[0].op == 'a' && g_log[0].bytes == NPIX * 3);
        EXPECT(st[0] && !st[1] && !st[2]);
        g_fail_malloc = 0;
    }
    EXPECT(g_log.size() == 2 && g_log[1].op == 'f' && g_log[1].dev == g_log[0].dev);

    // TAKE_HIP_FAIL_ALLOC counts the allocations of present planes only: the third is plane 4
    {
        g_log.clear();
        setenv("TAKE_HIP_FAIL_ALLOC", "3", 1);
        StagedPlanes<5> st{{plane_in(in3.data(), 3), plane_in(nullptr, 3), plane_out(out12.data(), 12), plane_out(nullptr, 12), plane_in(in8.data(), 8)}};
        EXPECT(st.alloc(NPIX, "injected") == TAKE_E_NOMEM && g_error == "injected");
        EXPECT(g_log.size() == 2 && st[0] && st[2] && !st[4]);
        unsetenv("TAKE_HIP_FAIL_ALLOC");
        EXPECT(!inject_alloc_failure());
    }

    // the precision dispatch: the tag's type is the Real
    EXPECT(with_real(TAKE_PRECISION_F32, [](auto tag) { return sizeof(tag); }) == 4);
    EXPECT(with_real(TAKE_PRECISION_F64, [](auto tag) { return sizeof(tag); }) == 8);
    int called = 0;
    with_real(TAKE_PRECISION_F64, [&](auto tag) { called += (int)sizeof(tag); });  // (a lambda that returns nothing)
    EXPECT(called == 8);

    if (g_failures == 0) std::printf("ok\n");
    return g_failures ? 1 : 0;
}
