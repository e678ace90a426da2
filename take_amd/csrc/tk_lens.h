// tk_lens.h — the thin-lens camera ray (EXTENSION, parity unpinned; specification: DESIGN.md §4k): the per-ray
// arithmetic of a camera with an aperture (CameraRec::lens_radius > 0) focused on the plane perpendicular to the view
// axis at CameraRec::focus along -w.  TK_HD and written once, as tk_motion_pixel.h: generate_path (the _lens kernels)
// runs it on the device, tests/lens_host runs the same text on the host, tests/lens_ref.py restates it in numpy.  Every + - * /
// is one operation of Real in the order written (-ffp-contract=off); cos, sin and sqrt are the library's.
//
// A sample's plane coordinates (sx, sy) are the pinhole camera's (draws 0 and 1 of the path's stream: CAMERA_DRAWS
// stays 2 and the shade rounds start where they always did); the two lens draws come from the same key at the counters
// LENS_COUNTER and LENS_COUNTER + 1, the top of the 32-bit counter space, which no path reaches.  A point of the plane
// of focus is seen by every lens ray of a sample where the sample's pinhole ray sees it.
#pragma once
#include <cstdint>

#include "tk_scene.h"

namespace tk {

constexpr uint32_t LENS_COUNTER = 0xFFFFFFFEu;

// (r1, r2) in [0, 1)^2 -> the unit disc, Shirley-Chiu's concentric map
template <class R> TK_HD void concentric_disc(R r1, R r2, R &x, R &y) {
    const R a = R(2) * r1 - R(1), b = R(2) * r2 - R(1);
    if (a == R(0) && b == R(0)) {
        x = R(0), y = R(0);
        return;
    }
    R r, phi;
    if (tk_fabs(a) > tk_fabs(b)) r = a, phi = (Const<R>::PI / R(4)) * (b / a);
    else r = b, phi = Const<R>::PI / R(2) - (Const<R>::PI / R(4)) * (a / b);
    x = r * tk_cos(phi), y = r * tk_sin(phi);
}

// The lens ray of the sample with plane coordinates (sx, sy) (camera_dir's, each in [-0.5, 0.5)) and random stream `key`
// -> origin o on the lens, unit direction d through the sample's point of the plane of focus.
template <class R> TK_HD void lens_ray(const CameraRec<R> &c, R sx, R sy, uint64_t key, Vec3<R> &o, Vec3<R> &d) {
    const Vec3<R> u{c.u[0], c.u[1], c.u[2]}, v{c.v[0], c.v[1], c.v[2]}, w{c.w[0], c.w[1], c.w[2]};
    const Vec3<R> p = u * (sx * c.viewport_width) + v * (sy * c.viewport_height) - w;  // the pinhole direction before its normalise
    Rng lens{key, LENS_COUNTER};
    const R r1 = random_real<R>(lens);
    const R r2 = random_real<R>(lens);
    R dx, dy;
    concentric_disc(r1, r2, dx, dy);
    const R lx = c.lens_radius * dx, ly = c.lens_radius * dy;
    const Vec3<R> off = u * lx + v * ly;
    o = Vec3<R>{c.lookfrom[0], c.lookfrom[1], c.lookfrom[2]} + off;
    d = normalize(p * c.focus - off);
}

}  // namespace tk
