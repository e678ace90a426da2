// normals_shim.cpp — TEST INFRASTRUCTURE.  The per-face and per-vertex arithmetic of take_amd/csrc/tk_normals.h built
// for the host (the C library's asin, as the reference's) and run as the reference's serial loop, so that
// tests/test_normals_cpu.py can hold it to the reference's compute_normals bit for bit without a GPU.  Never loaded
// by the product.
#include <cstdint>

#include "tk_normals.h"

extern "C" {
// -> 0, or -1: an index outside [0, n_vertices) (nothing written)
int normals_shim_compute(const double *positions, int64_t n_vertices, const int32_t *indices, int64_t n_faces, double *out) {
    return tk::nrm::compute_normals_serial(positions, n_vertices, indices, n_faces, out) ? 0 : -1;
}
// the three products n * angle of one face -> 1, or 0: its normal has length 0 and it adds nothing
int normals_shim_face(const double *positions, const int32_t *face, double *out9) {
    tk::nrm::V3 c[3];
    if (!tk::nrm::face_contributions(positions, face[0], face[1], face[2], c)) return 0;
    for (int i = 0; i < 3; i++) out9[3 * i] = c[i].x, out9[3 * i + 1] = c[i].y, out9[3 * i + 2] = c[i].z;
    return 1;
}
}
