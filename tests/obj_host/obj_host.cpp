// obj_host.cpp — TEST INFRASTRUCTURE.  The per-token and per-line functions of take_amd/csrc/tk_obj.h (parse_real,
// stoi_prefix, parse_corner, classify_line: the text k_obj_classify and k_obj_parse run per lane), built for the host and
// run serially over a buffer of tokens or lines, so that tests/test_obj_cpu.py can hold them to the restatement
// (tests/obj_ref.py) and to Python's correctly rounded float() without a GPU.  Never loaded by the product.
#include <cstdint>

#include "tk_obj.h"

extern "C" {
// element i of each call is the bytes [off[i], off[i + 1]) of `buf` (off: n + 1 offsets, ascending)

// parse_real: code[i] = 0 converted on the device (value[i] holds it), 1 left to the host's strtod, -1 not in the grammar;
// value[i] keeps what the caller put there unless the code is 0
void obj_host_parse_real(const uint8_t *buf, const int64_t *off, int64_t n, int32_t *code, double *value) {
    for (int64_t i = 0; i < n; i++) code[i] = tk::obj::parse_real(buf, off[i], off[i + 1], value + i);
}

// stoi_prefix on a non-empty piece: ok[i] = 1 and value[i], or ok[i] = 0 where std::stoi throws
void obj_host_stoi_prefix(const uint8_t *buf, const int64_t *off, int64_t n, int32_t *ok, int32_t *value) {
    for (int64_t i = 0; i < n; i++) {
        int32_t v = 0;
        ok[i] = tk::obj::stoi_prefix(buf, off[i], off[i + 1], v);
        value[i] = v;
    }
}

// parse_corner: ok[i] = 1 and key[3 i .. 3 i + 2] = (v, vt, vn), or ok[i] = 0 where std::stoi throws
void obj_host_parse_corner(const uint8_t *buf, const int64_t *off, int64_t n, int32_t *ok, int32_t *key) {
    for (int64_t i = 0; i < n; i++) ok[i] = tk::obj::parse_corner(buf, off[i], off[i + 1], key + 3 * i);
}

// classify_line on an untrimmed line (without its '\n'): type[i] = a tk::obj::LineType
void obj_host_classify(const uint8_t *buf, const int64_t *off, int64_t n, uint8_t *type) {
    for (int64_t i = 0; i < n; i++) type[i] = tk::obj::classify_line(buf, off[i], off[i + 1]);
}

// the LineType values in the order NONE, V, VT, VN, F3, F4, FBAD
void obj_host_line_types(uint8_t out[7]) {
    const uint8_t t[7] = {tk::obj::L_NONE, tk::obj::L_V, tk::obj::L_VT, tk::obj::L_VN, tk::obj::L_F3, tk::obj::L_F4, tk::obj::L_FBAD};
    for (int k = 0; k < 7; k++) out[k] = t[k];
}
}
