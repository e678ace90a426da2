// tk_round.h — directed rounding of a double to float, for boxes that must contain double geometry
// (tk_build_gpu.h::k_prim_boxes<double>).  Written on the bit patterns, so the host build (tests/round_shim) and the
// device give the same answer whatever the rounding and denormal modes of either.
#pragma once

#include "tk_common.h"

namespace tk {

// the neighbours of a float in the order of the reals (x not NaN; -0 and +0 count as one value; the neighbour of the
// largest finite float is the infinity, and the infinities stay)
TK_HD float f_below(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    if (u == 0xff800000u) return x;
    u = x > 0.0f ? u - 1u : (x < 0.0f ? u + 1u : 0x80000001u);
    __builtin_memcpy(&x, &u, 4);
    return x;
}
TK_HD float f_above(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    if (u == 0x7f800000u) return x;
    u = x > 0.0f ? u + 1u : (x < 0.0f ? u - 1u : 0x00000001u);
    __builtin_memcpy(&x, &u, 4);
    return x;
}

// The largest float <= x and the smallest float >= x (x not NaN): the conversion rounds to a float f next to x (to
// nearest by default; any mode gives one of the two floats around x), and where f lies on the wrong side of x its
// neighbour on the other side is the answer.  A float-representable x comes back unchanged; |x| beyond the largest
// float gives that float on the inner side and the infinity on the outer one; a double too small for a float
// denormal gives 0 on the inner side and the smallest denormal on the outer one.
TK_HD float d2f_down(double x) {
    const float f = (float)x;
    return (double)f > x ? f_below(f) : f;
}
TK_HD float d2f_up(double x) {
    const float f = (float)x;
    return (double)f < x ? f_above(f) : f;
}

}  // namespace tk
