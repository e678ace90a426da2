"""CPU side of the motion pass that follows moved vertices (take_hip_scene_track_vertices, take_hip_scene_tracking_info:
include/take_hip.h): the two symbols are declared, exported and bound, they are no new ABI version and change no
struct, the refusals that need no device are TAKE_E_INVALID with their messages; and the per-pixel text the device runs
(take_amd/csrc/tk_motion_pixel.h: tracked_pixel) built for the host (tests/motion_host) against the numpy restatement
(tests/motion_ref.py) on synthetic records: hit / miss / sphere, in and out of a placement, u and v on the corners, the
edges and inside, points behind the camera, NaN in every input.

Bars.  f64 and f32 host builds are each bit-identical to the restatement of their own dtype (the same operations in the
same order).  f32 against the f64 restatement of the float-rounded inputs: F32_XY_BAR pixel and F32_REL_BAR relative on
prev_depth, the next power of ten above 8 x the largest difference measured on these records (1.74e-5 pixel: 8 x = 1.4e-4;
1.64e-7 relative: 8 x = 1.3e-6; DESIGN.md par. 4i); the pixel bar has to stay at or below 0.01 pixel, where a bilinear weight
visibly changes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import motion_ref as M
from helpers import HERE
from take_amd import capi
from take_amd import cdefs as D

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_scene_track_vertices", "take_hip_scene_tracking_info")
F32_XY_BAR, F32_REL_BAR = 1e-3, 1e-5
assert F32_XY_BAR <= 0.01


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ------------------------------------------------------------------ the boundary
def test_the_two_symbols_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "take_hip.h")).read(), flags=re.S)
    assert set(D.TRACKING_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.TRACKING_PROTOTYPES[name], name
    assert [len(D.TRACKING_PROTOTYPES[n]) for n in SYMBOLS] == [2, 3]
    assert re.search(r"#define\s+TAKE_TRACK_VERTICES\s+1\b", hdr) and D.TAKE_TRACK_VERTICES == 1
    assert callable(capi.Scene.track_vertices) and callable(capi.Scene.tracking_info)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version


def test_no_existing_struct_changed_its_size():
    """the sizes the earlier CPU tests pin, and those of the records the kernels share (InstTrace, InstShade, PrimRec)"""
    assert (C.sizeof(D.TakeMotionBuffers), C.sizeof(D.TakeTemporalFrame), C.sizeof(D.TakeTemporalOpts)) == (32, 48, 16)
    assert (C.sizeof(D.TakeMeshUpdate), C.sizeof(D.TakeAdaptiveStats)) == (24, 24)
    prog = ('#include <cstdio>\n#include "take_hip.h"\n#include "tk_scene.h"\nint main() { std::printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(tk::PrimRec<float>), '
            "sizeof(tk::PrimRec<double>), sizeof(tk::InstTrace<float>), sizeof(tk::InstTrace<double>), sizeof(tk::InstShade<float>), sizeof(tk::InstShade<double>)); }\n")
    import tempfile

    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.cpp"), os.path.join(td, "t")
        open(src, "w").write(prog)
        subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "take_amd", "csrc"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert [int(x) for x in out] == [64, 96, 80, 128, 64, 96]


def test_refusals_come_before_the_device_is_looked_for(lib):
    """TAKE_E_INVALID with its message, never TAKE_E_NO_GPU, with or without a GPU (`scene` is not a scene: a call that
    went past the argument check would not survive it)"""
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    flags, held = C.c_int32(), C.c_int64()
    for call, msg in ((lambda: lib.take_hip_scene_track_vertices(None, D.TAKE_TRACK_VERTICES), b"null argument"),
                      (lambda: lib.take_hip_scene_track_vertices(None, 0), b"null argument"),
                      (lambda: lib.take_hip_scene_track_vertices(scene, 2), b"unknown flag bits"),
                      (lambda: lib.take_hip_scene_track_vertices(scene, D.TAKE_TRACK_VERTICES | 4), b"unknown flag bits"),
                      (lambda: lib.take_hip_scene_track_vertices(scene, -1), b"unknown flag bits"),
                      (lambda: lib.take_hip_scene_tracking_info(None, C.byref(flags), C.byref(held)), b"null argument")):
        assert call() == D.TAKE_E_INVALID and msg in lib.take_hip_last_error(), msg


def test_the_texts_agree_on_what_is_kept():
    """the header, the kernel's header and the restatement name the same layout and the same message"""
    hdr = open(os.path.join(ROOT, "include", "take_hip.h")).read()
    pix = open(os.path.join(ROOT, "take_amd", "csrc", "tk_motion_pixel.h")).read()
    build = open(os.path.join(ROOT, "take_amd", "csrc", "tk_build.hip")).read()
    assert "constexpr int MARKED_STRIDE = 12;" in pix and "48 bytes per record in f32, 96 in f64" in hdr
    assert "out of device memory for the marked frame's geometry" in hdr and "out of device memory for the marked frame's geometry" in build
    assert (M.MISS, M.POINT, M.TRIANGLE) == (0, 1, 2) and "MOTION_MISS = 0, MOTION_POINT = 1, MOTION_TRIANGLE = 2" in pix


# ------------------------------------------------------------------ the pixel function, host build against the restatement
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "motion_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libmotion_host.so"))
        L.motion_host.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 12
        _HOST = L
    return _HOST


def host_pixels(cam, rec, dtype):
    """what the kernel's text computes on the records rounded to dtype -> prev_xy (n, 2), prev_depth (n,)"""
    n = len(rec["kind"])
    a = {k: np.ascontiguousarray(rec[k].astype(dtype)) for k in ("ro", "rd", "t", "u", "v", "words", "inv")}
    c = np.ascontiguousarray(M.camera_words(cam, dtype))
    kind, placed, fwd = np.ascontiguousarray(rec["kind"], np.int32), np.ascontiguousarray(rec["placed"], np.int32), np.ascontiguousarray(rec["fwd"], np.float64)
    xy, pd = np.full((n, 2), 7, dtype), np.full(n, 7, dtype)
    rc = host_lib().motion_host(int(dtype == np.float64), c.ctypes.data, cam["width"], cam["height"], n, kind.ctypes.data, a["ro"].ctypes.data, a["rd"].ctypes.data,
                                a["t"].ctypes.data, a["u"].ctypes.data, a["v"].ctypes.data, a["words"].ctypes.data, a["inv"].ctypes.data, fwd.ctypes.data,
                                placed.ctypes.data, xy.ctypes.data, pd.ctypes.data)
    assert rc == 0
    return xy, pd


@pytest.fixture(scope="module")
def records():
    return M.synthetic_records()


def test_the_records_cover_the_cases(records):
    _, r = records
    k, p = r["kind"], r["placed"]
    for kind in (M.MISS, M.POINT, M.TRIANGLE):
        assert (k == kind).sum() > 50
    assert ((k == M.TRIANGLE) & p).sum() > 30 and ((k == M.TRIANGLE) & ~p).sum() > 30 and ((k == M.POINT) & p).sum() > 30 and not (p & (k == M.MISS)).any()
    tri = k == M.TRIANGLE
    for u, v in ((0, 0), (1, 0), (0, 1), (0.5, 0.5)):
        assert (tri & (r["u"] == u) & (r["v"] == v)).any(), (u, v)
    assert (tri & (r["u"] > 0) & (r["v"] > 0) & (r["u"] + r["v"] < 1)).sum() > 50
    assert all(np.isnan(r[name]).any() for name in ("words", "u", "fwd", "rd", "t"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_build_is_bit_identical_to_the_restatement_of_its_dtype(records, dtype):
    cam, r = records
    xy, pd = host_pixels(cam, r, dtype)
    want_xy, want_pd = M.tracked_pixels(cam, dtype=dtype, **r)
    assert xy.dtype == want_xy.dtype == dtype
    assert np.array_equal(xy, want_xy, equal_nan=True) and np.array_equal(pd, want_pd, equal_nan=True)
    seen = (xy[:, 0] != -2) & np.isfinite(xy).all(-1)
    assert seen.mean() > 0.5 and (xy[~np.isnan(xy).any(-1) & ~seen] == -2).all(), "unseen points are (-2, -2)"
    assert (pd[r["kind"] == M.MISS] == 0).all() and (pd[xy[:, 0] == -2] == 0).all()


def test_a_point_behind_the_marked_camera_and_nan_are_nowhere_or_nan(records):
    cam, r = records
    xy, pd = host_pixels(cam, r, np.float64)
    e_z = np.where(r["kind"] == M.TRIANGLE, -(r["words"][:, :3] - cam["from"]) @ cam["w"], 1.0)
    behind = (r["kind"] == M.TRIANGLE) & ~r["placed"] & (r["u"] == 0) & (r["v"] == 0) & (e_z < 0)
    assert behind.any() and (xy[behind] == -2).all() and (pd[behind] == 0).all()
    bad = np.isnan(r["words"]).any(-1) & (r["kind"] == M.TRIANGLE)
    assert bad.any() and ((xy[bad] == -2).all(-1) | np.isnan(xy[bad]).any(-1)).all(), "NaN words: nowhere, or not a number — never a pixel"


def test_f32_against_the_f64_restatement_of_the_rounded_inputs(records):
    cam, r = records
    xy, pd = host_pixels(cam, r, np.float32)
    r32 = {k: (v.astype(np.float32).astype(np.float64) if v.dtype == np.float64 and k != "fwd" else v) for k, v in r.items()}
    r32["fwd"] = r["fwd"].astype(np.float32).astype(np.float64)
    cam32 = dict(cam)
    w = M.camera_words(cam, np.float32).astype(np.float64)
    cam32.update(u=w[0:3], v=w[3:6], w=w[6:9], vw=w[12], vh=w[13])
    cam32["from"] = w[9:12]
    want_xy, want_pd = M.tracked_pixels(cam32, dtype=np.float64, **r32)
    ok = np.isfinite(want_xy).all(-1) & (want_xy[:, 0] != -2)
    assert ok.mean() > 0.5 and np.array_equal(xy[:, 0] != -2, want_xy[:, 0] != -2), "the same points are seen"
    d_xy = float(np.abs(xy[ok].astype(np.float64) - want_xy[ok]).max())
    hit = ok & (r["kind"] != M.MISS)
    d_pd = float(np.abs(pd[hit].astype(np.float64) / want_pd[hit] - 1).max())
    print(f"f32 host build against the f64 restatement: prev_xy {d_xy:.3e} pixel (bar {F32_XY_BAR:.0e}), prev_depth {d_pd:.3e} relative (bar {F32_REL_BAR:.0e})")
    assert d_xy <= F32_XY_BAR and d_pd <= F32_REL_BAR


def test_u_goes_with_e1_and_v_with_e2(records):
    """at (u, v) = (1, 0) the point is v0' + e1', at (0, 1) v0' + e2' (tri_test's convention): a swap moves the pixel"""
    cam, r = records
    n = 8
    rec = {k: v[:n].copy() for k, v in r.items()}
    rec["kind"][:] = M.TRIANGLE
    rec["placed"][:] = False
    rec["words"] = np.tile(np.array([0.1, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.4, 0.0]), (n, 1))
    rec["u"][:], rec["v"][:] = 1.0, 0.0
    along_e1, _ = host_pixels(cam, rec, np.float64)
    rec["u"][:], rec["v"][:] = 0.0, 1.0
    along_e2, _ = host_pixels(cam, rec, np.float64)
    rec["u"][:], rec["v"][:] = 0.0, 0.0
    at_v0, _ = host_pixels(cam, rec, np.float64)
    d1, d2 = along_e1 - at_v0, along_e2 - at_v0
    assert (np.abs(d1[:, 0]) > 10 * np.abs(d1[:, 1])).all() and (d1[:, 0] > 1).all(), "e1 = +x moves the pixel to the right"
    assert (np.abs(d2[:, 1]) > 10 * np.abs(d2[:, 0])).all() and (d2[:, 1] < -1).all(), "e2 = +y moves the pixel up (row 0 = top)"
