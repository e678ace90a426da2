"""CPU side of the temporal reprojection and accumulation (take_hip_scene_mark_frame, take_hip_render_motion,
take_hip_temporal_accumulate, take_hip_render_temporal and their _device twins: include/take_hip.h): the symbols are
declared, exported and bound, the defaults are the same in every place, every refusal that needs no device is
TAKE_E_INVALID with its message; the text the device runs (take_amd/csrc/tk_temporal.h) built for the host
(tests/temporal_host) against the numpy restatement (tests/temporal_ref.py); and the properties of the specification
(DESIGN.md par. 4i), on the restatement alone.

Bars, those of tests/test_denoise_var_cpu.py.  Host build against the restatement in f64: 1e-12 * max(1, max|ref|) on
rgb, m1 and m2 — the same operations in the same order — and count equal.  In f32: count equal to the f32 restatement's
(the same float operations), rgb 1e-5 * max(1, max|ref|) against the f64 restatement of the float-rounded inputs on the
pixels where the two restatements give the same count (where they do not, a weight's last float bit moved n_r + 0.5 across
an integer: the two differ by a whole history sample there; those pixels are held to the f32 restatement and counted
against the cap of 0.1 %)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_var_ref as V
import temporal_ref as T
from helpers import HERE
from take_amd import capi
from take_amd import cdefs as D

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_scene_mark_frame", "take_hip_render_motion_device", "take_hip_render_motion", "take_hip_temporal_accumulate_device",
           "take_hip_temporal_accumulate", "take_hip_render_temporal_device", "take_hip_render_temporal")
SIZES = [(1, 1), (7, 1), (1, 7), (37, 23), (130, 70)]
TESTS = [("depth", "shape_id"), ()]
CAP = 1e-3  # share of the pixels whose count may differ between the f32 and the f64 arithmetic


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ------------------------------------------------------------------ the boundary
def test_the_seven_symbols_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "take_hip.h")).read(), flags=re.S)
    assert set(D.TEMPORAL_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.TEMPORAL_PROTOTYPES[name], name
    assert [len(D.TEMPORAL_PROTOTYPES[n]) for n in SYMBOLS] == [1, 4, 3, 10, 9, 8, 7]
    for f in (capi.temporal_accumulate, capi.temporal_accumulate_device, capi.Scene.mark_frame, capi.Scene.render_motion, capi.Scene.render_motion_device,
              capi.Scene.render_temporal, capi.Scene.render_temporal_device):
        assert callable(f)
    for struct in ("TakeMotionBuffers", "TakeTemporalFrame", "TakeTemporalOpts"):
        assert re.search(r"typedef struct " + struct + r"\b", hdr) and hasattr(D, struct), struct
    assert (C.sizeof(D.TakeMotionBuffers), C.sizeof(D.TakeTemporalFrame), C.sizeof(D.TakeTemporalOpts)) == (32, 48, 16)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version


def test_the_defaults_are_the_same_in_every_place():
    hdr = open(os.path.join(ROOT, "include", "take_hip.h")).read()
    assert "samples of history a pixel may carry; <= 0: 64" in hdr and "relative; <= 0: 0.05" in hdr
    assert D.TEMPORAL_DEFAULTS == T.DEFAULTS == {"max_history": 64, "depth_tol": 0.05}
    src = open(os.path.join(ROOT, "take_amd", "csrc", "tk_denoise.hip")).read()
    assert "int max_history = 64;" in src and "double depth_tol = 0.05;" in src
    o = D.temporal_opts()
    assert (o.max_history, o.flags, o.depth_tol) == (0, 0, 0.0)
    # a value <= 0 and a missing one are the default: the restatement, as the library
    cur, hist, pd = T.frames(37, 23)
    xy = T.motion("fraction", 37, 23)
    first = T.accumulate(cur, hist, xy, pd)
    for kw in (dict(max_history=64, depth_tol=0.05), dict(max_history=-1, depth_tol=-1.0)):
        again = T.accumulate(cur, hist, xy, pd, **kw)
        assert all(np.array_equal(first[k], again[k]) for k in first)
    assert not np.array_equal(first["count"], T.accumulate(cur, hist, xy, pd, max_history=3)["count"])
    assert not np.array_equal(first["count"], T.accumulate(cur, hist, xy, pd, depth_tol=1e-4)["count"])


def test_refusals_come_before_the_device_is_looked_for(lib):
    """TAKE_E_INVALID with its message, never TAKE_E_NO_GPU, with or without a GPU.  (`scene` and the planes below are
    not a scene and not device memory: a call that went past the argument check would not survive it.)"""
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    ro = D.TakeRenderOpts()
    ro.spp = 1
    F32 = D.TAKE_PRECISION_F32
    p = buf.value

    def ref(x):
        return None if x is None else C.byref(x)

    def frame(missing=None):
        return D.TakeTemporalFrame(*[None if k == missing else p for k in range(4)], None, None)

    full = frame()

    def dev(cur=full, hist=None, xy=buf, precision=F32, w=2, h=2, opts=None, out=full):
        return lib.take_hip_temporal_accumulate_device(ref(cur), ref(hist), xy, None, precision, w, h, ref(opts), ref(out), None)

    def host(cur=full, hist=None, xy=buf, precision=F32, w=2, h=2, opts=None, out=full):
        return lib.take_hip_temporal_accumulate(ref(cur), ref(hist), xy, None, precision, w, h, ref(opts), ref(out))

    def md(sc=scene, o=ro, b=D.TakeMotionBuffers(p, p, p, p)):
        return lib.take_hip_render_motion_device(sc, ref(o), ref(b), None)

    def mh(sc=scene, o=ro, b=D.TakeMotionBuffers(p, p, p, p)):
        return lib.take_hip_render_motion(sc, ref(o), ref(b))

    def rd(sc=scene, o=ro, a=None, t=None, opts=None, out=buf):
        return lib.take_hip_render_temporal_device(sc, ref(o), ref(a), ref(t), ref(opts), 0, out, None)

    def rh(sc=scene, o=ro, a=None, t=None, opts=None, out=buf):
        return lib.take_hip_render_temporal(sc, ref(o), ref(a), ref(t), ref(opts), 0, out)

    bad_temporal = [(D.TakeTemporalOpts(0, 1, 0.0), b"unknown flag bits"), (D.TakeTemporalOpts(0, -1, 0.0), b"unknown flag bits")]
    bad_temporal += [(D.temporal_opts(depth_tol=v), b"depth_tol must be finite") for v in (float("nan"), float("inf"), -float("inf"))]
    bad_adaptive = (D.adaptive_opts(threshold=float("nan")), b"threshold and floor must be finite")
    bad_denoise = (D.denoise_opts(iterations=9), b"iterations")
    cases = [(lambda: lib.take_hip_scene_mark_frame(None), b"null argument")]
    for f in (dev, host):
        cases += [(lambda f=f: f(cur=None), b"null argument"), (lambda f=f: f(out=None), b"null argument"), (lambda f=f: f(xy=None), b"null argument")]
        cases += [(lambda f=f, k=k: f(cur=frame(k)), b"null argument") for k in range(4)]
        cases += [(lambda f=f, k=k: f(out=frame(k)), b"null argument") for k in range(4)]
        cases += [(lambda f=f, k=k: f(hist=frame(k)), b"incomplete history") for k in range(4)]
        cases += [(lambda f=f: f(w=0), b"width and height"), (lambda f=f: f(h=-3), b"width and height"),
                  (lambda f=f: f(precision=D.TAKE_PRECISION_MIXED), b"unknown precision"), (lambda f=f: f(precision=-1), b"unknown precision")]
        cases += [(lambda f=f, t=t: f(opts=t), msg) for t, msg in bad_temporal]
    for f in (md, mh):
        cases += [(lambda f=f: f(sc=None), b"null argument"), (lambda f=f: f(o=None), b"null argument"), (lambda f=f: f(b=None), b"null argument"),
                  (lambda f=f: f(b=D.TakeMotionBuffers()), b"no motion buffer was asked for")]
    for f in (rd, rh):
        cases += [(lambda f=f: f(sc=None), b"null argument"), (lambda f=f: f(o=None), b"null argument"), (lambda f=f: f(out=None), b"null argument")]
        cases += [(lambda f=f: f(a=bad_adaptive[0]), bad_adaptive[1]), (lambda f=f: f(opts=bad_denoise[0]), bad_denoise[1])]
        cases += [(lambda f=f, t=t: f(t=t), msg) for t, msg in bad_temporal]
        # the refusals of the three parts in that order: the sampler's, the accumulation's, the denoiser's
        cases += [(lambda f=f: f(a=bad_adaptive[0], t=bad_temporal[0][0], opts=bad_denoise[0]), bad_adaptive[1]),
                  (lambda f=f: f(t=bad_temporal[0][0], opts=bad_denoise[0]), bad_temporal[0][1])]
    assert len(cases) == 1 + 2 * 24 + 2 * 4 + 2 * 12
    for call, msg in cases:
        lib.take_hip_scene_build_info(None, None, None)  # (leaves another message behind)
        assert b"null scene" in lib.take_hip_last_error()
        assert call() == D.TAKE_E_INVALID
        assert msg in lib.take_hip_last_error(), (msg, lib.take_hip_last_error())


def test_the_python_binding_checks_its_arrays():
    cur, hist, pd = T.frames(7, 5)
    c, hh = T.cast(cur, np.float32), T.cast(hist, np.float32)
    xy = T.motion("identity", 7, 5).astype(np.float32)
    bad = [dict(cur=dict(c, rgb=c["rgb"].astype(np.float64).astype(np.int32)), hist=hh, prev_xy=xy), dict(cur=dict(c, count=c["count"].astype(np.int64)), hist=hh, prev_xy=xy),
           dict(cur={k: v for k, v in c.items() if k != "m1"}, hist=hh, prev_xy=xy), dict(cur=c, hist=dict(hh, m2=hh["m2"].astype(np.float32)), prev_xy=xy),
           dict(cur=c, hist=dict(hh, rgb=hh["rgb"].astype(np.float64)), prev_xy=xy), dict(cur=c, hist=hh, prev_xy=xy.astype(np.float64)),
           dict(cur=c, hist=hh, prev_xy=xy[..., 0]), dict(cur=c, hist=hh, prev_xy=None), dict(cur=c, hist=hh, prev_xy=xy, prev_depth=pd),
           dict(cur=dict(c, albedo=c["rgb"]), hist=hh, prev_xy=xy), dict(cur=c, hist=hh, prev_xy=xy, opts=D.temporal_opts(), max_history=2),
           dict(cur=dict(c, depth=c["depth"][:, :3]), hist=hh, prev_xy=xy)]
    for kw in bad:
        with pytest.raises(ValueError):
            capi.temporal_accumulate(**kw)
    with pytest.raises(ValueError):
        capi.temporal_accumulate_device({"rgb": 1, "count": 1, "m1": 1, "m2": 1, "normal": 1}, None, 1, None, 2, 2, D.TAKE_PRECISION_F32)


# ------------------------------------------------------------------ host execution of tk_temporal.h
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "temporal_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libtemporal_host.so"))
        L.temporal_host.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p]
        _HOST = L
    return _HOST


def host_accumulate(cur, hist, prev_xy, prev_depth=None, in_place=False, max_history=64, depth_tol=0.05):
    """contiguous planes of one dtype -> what the kernel's text computes: a dict of the output's planes"""
    dtype = cur["rgb"].dtype
    cur = {k: v.copy() for k, v in cur.items()}
    out = cur if in_place else {k: (np.full_like(v, np.nan) if v.dtype.kind == "f" else np.full_like(v, -7)) for k, v in cur.items()}

    def pointers(f):
        return (C.c_void_p * 6)(*[f[k].ctypes.data if f.get(k) is not None else None for k in T.PLANES])

    h, w = cur["count"].shape
    xy = np.ascontiguousarray(prev_xy, dtype)
    pd = None if prev_depth is None else np.ascontiguousarray(prev_depth, dtype)
    rc = host_lib().temporal_host(int(dtype == np.float64), pointers(cur), None if hist is None else pointers(hist), xy.ctypes.data,
                                  None if pd is None else pd.ctypes.data, w, h, max_history, depth_tol, pointers(out))
    assert rc == 0
    return out


CASES = [(size, m, tests, mh) for size in SIZES for m in T.MOTIONS for tests in TESTS for mh in (1, 64)]


def case_id(c):
    (w, h), m, tests, mh = c
    return f"{w}x{h}-{m}-{'tests' if tests else 'plain'}-h{mh}"


def inputs(c, dtype):
    (w, h), m, tests, mh = c
    cur, hist, pd = T.frames(w, h)
    return T.cast(cur, dtype, tests), T.cast(hist, dtype, tests), T.motion(m, w, h).astype(dtype), (pd.astype(dtype) if tests else None), mh


def check(got, ref, bar, label, where=None):
    """rgb, m1 and m2 against the reference's on max(1, max|ref|) (on the pixels of `where`), depth and shape_id equal"""
    for k in ("rgb", "m1", "m2"):
        scale = max(1.0, float(np.abs(ref[k]).max()))
        d = np.abs(got[k].astype(np.float64) - ref[k])
        if where is not None:
            d = d[where]
        d = float(d.max()) if d.size else 0.0
        print(f"{label} {k}: max |difference| {d:.3e}, bar {bar * scale:.3e}")
        assert np.isfinite(got[k]).all() and d <= bar * scale, (label, k, d)
    for k in ("depth", "shape_id"):
        assert (k in got) == (k in ref) and (k not in ref or np.array_equal(got[k], ref[k])), (label, k)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_host_build_against_the_restatement_f64(c):
    cur, hist, xy, pd, mh = inputs(c, np.float64)
    got, ref = host_accumulate(cur, hist, xy, pd, max_history=mh), T.accumulate(cur, hist, xy, pd, max_history=mh)
    assert np.array_equal(got["count"], ref["count"])
    check(got, ref, 1e-12, "f64 " + case_id(c))


def widen(f):
    return None if f is None else {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in f.items()}


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_host_build_against_the_restatement_f32(c):
    cur, hist, xy, pd, mh = inputs(c, np.float32)
    got = host_accumulate(cur, hist, xy, pd, max_history=mh)
    ref32 = T.accumulate(cur, hist, xy, pd, max_history=mh)
    ref64 = T.accumulate(widen(cur), widen(hist), xy.astype(np.float64), None if pd is None else pd.astype(np.float64), max_history=mh)
    assert got["rgb"].dtype == np.float32 and np.array_equal(got["count"], ref32["count"])
    same = ref32["count"] == ref64["count"]
    print(f"{case_id(c)}: {int((~same).sum())} of {same.size} pixels differ in count between the f32 and the f64 restatement")
    assert (~same).sum() <= max(CAP * same.size, 0)
    check(got, ref64, 1e-5, "f32 against f64 " + case_id(c), where=same)
    check(ref32, ref64, 1e-5, "f32 restatement against f64 " + case_id(c), where=same)
    check(got, {k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in ref32.items()}, 1e-5, "f32 against the f32 restatement " + case_id(c))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_build_without_a_history_gives_the_frame_back(size, dtype):
    cur, _, _ = T.frames(*size)
    c = T.cast(cur, dtype)
    xy = T.motion("identity", *size).astype(dtype)
    for out in (host_accumulate(c, None, xy), T.accumulate(c, None, xy)):
        assert all(np.array_equal(out[k], c[k]) for k in c)


def test_host_build_in_place_and_repeated():
    cur, hist, pd = T.frames(37, 23)
    c, h = T.cast(cur, np.float64), T.cast(hist, np.float64)
    xy = T.motion("random", 37, 23)
    a, b, i = host_accumulate(c, h, xy, pd), host_accumulate(c, h, xy, pd), host_accumulate(c, h, xy, pd, in_place=True)
    assert all(np.array_equal(a[k], b[k]) and np.array_equal(a[k], i[k]) for k in a)


def test_the_cases_can_tell_a_wrong_tap_from_a_right_one():
    """the history moved by one pixel, or the id test dropped, moves the result by orders above either bar"""
    cur, hist, pd = T.frames(37, 23)
    a = T.accumulate(cur, hist, T.motion("fraction", 37, 23), pd)
    b = T.accumulate(cur, hist, T.motion("fraction", 37, 23) + (1.0, 0.0), pd)
    c = T.accumulate(T.cast(cur, np.float64, ("depth",)), T.cast(hist, np.float64, ("depth",)), T.motion("fraction", 37, 23), pd)
    for other in (b, c):
        d = float(np.abs(a["rgb"] - other["rgb"]).max())
        print(f"max |difference| of rgb {d:.3e}")
        assert d > 1e-3


# ------------------------------------------------------------------ properties of the specification (the restatement alone)
def constant_variance_frame(rng, shape, c, mean=1.0, sigma=0.25):
    """a frame of c samples per pixel, L_s = mean + sigma * z (grey: r = g = b = L / 3)"""
    L = mean + sigma * rng.standard_normal((c,) + shape)
    m1, m2 = L.sum(0), (L * L).sum(0)
    return {"rgb": np.repeat((m1 / c / 3.0)[..., None], 3, -1), "count": np.full(shape, c, np.int32), "m1": m1, "m2": m2}, L


def test_identity_motion_pools_the_frames_exactly():
    """K frames of c samples under identity motion with every test passing and max_history >= K c: count = K c exactly,
    m1, m2 and rgb the pooled statistics to 1e-12 relative"""
    rng = np.random.default_rng(5)
    shape, c, K = (23, 37), 4, 6
    xy = T.motion("identity", shape[1], shape[0])
    acc, all_L = None, []
    for k in range(K):
        f, L = constant_variance_frame(rng, shape, c)
        f["depth"], f["shape_id"] = np.full(shape, 2.0), np.full(shape, 3, np.int32)
        all_L.append(L)
        acc = T.accumulate(f, acc, xy, f["depth"], max_history=K * c)
    L = np.concatenate(all_L)
    assert (acc["count"] == K * c).all()
    for got, want in ((acc["m1"], L.sum(0)), (acc["m2"], (L * L).sum(0)), (acc["rgb"][..., 0], L.mean(0) / 3.0)):
        d = float(np.abs(got / want - 1).max())
        print(f"pooled: max relative difference {d:.3e}")
        assert d <= 1e-12


def test_an_integer_shift_is_the_shifted_history():
    cur, hist, _ = T.frames(37, 23)
    c, h = T.cast(cur, np.float64, ()), T.cast(hist, np.float64, ())
    out = T.accumulate(c, h, T.motion("integer", 37, 23), max_history=1000)
    H, W = c["count"].shape
    ys, xs = np.mgrid[0:H, 0:W]
    qx, qy = xs + 3, ys - 2
    inside = (qx < W) & (qy >= 0)
    qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
    nh = np.where(inside, h["count"][qyc, qxc], 0)
    assert np.array_equal(out["count"], c["count"] + nh)
    live = nh > 0
    want_m1 = np.where(live, h["m1"][qyc, qxc] + c["m1"], c["m1"])
    assert float(np.abs(out["m1"] - want_m1).max()) <= 1e-12 * float(np.abs(want_m1).max())
    want = (h["rgb"][qyc, qxc] * nh[..., None] + c["rgb"] * c["count"][..., None]) / (nh + c["count"])[..., None]
    assert float(np.abs(out["rgb"] - want)[live].max()) <= 1e-12 * float(np.abs(want).max())
    assert np.array_equal(out["rgb"][~live], c["rgb"][~live]) and np.array_equal(out["m2"][~live], c["m2"][~live])


def test_a_pixel_whose_taps_all_fail_is_the_current_frame_bitwise():
    cur, hist, pd = T.frames(37, 23)
    c, h = T.cast(cur, np.float64), T.cast(hist, np.float64)
    for dtype in (np.float32, np.float64):
        cc, hh = T.cast(cur, dtype), T.cast(hist, dtype)
        # nowhere; off the image; a history without samples; ids that never match; depths that never match
        for hist_k, xy, prev_depth in ((hh, np.full((23, 37, 2), -2.0), pd), (hh, T.motion("identity", 37, 23) + 1000.0, pd),
                                       (dict(hh, count=np.zeros_like(hh["count"])), T.motion("fraction", 37, 23), pd),
                                       (dict(hh, shape_id=hh["shape_id"] + 100), T.motion("fraction", 37, 23), pd), (hh, T.motion("fraction", 37, 23), pd * 2.0),
                                       (hh, np.full((23, 37, 2), np.nan), pd)):
            out = T.accumulate(cc, hist_k, xy.astype(dtype), prev_depth.astype(dtype))
            assert all(np.array_equal(out[k], cc[k]) for k in cc)
            got = host_accumulate(cc, hist_k, xy.astype(dtype), prev_depth.astype(dtype))
            assert all(np.array_equal(got[k], cc[k]) for k in cc)
    # the patch without samples, under identity motion and no other test
    out = T.accumulate(T.cast(cur, np.float64, ()), T.cast(hist, np.float64, ()), T.motion("identity", 37, 23))
    patch = h["count"] == 0
    assert patch.any() and np.array_equal(out["rgb"][patch], c["rgb"][patch]) and np.array_equal(out["count"][patch], c["count"][patch])
    assert (out["count"][~patch] > c["count"][~patch]).all()


@pytest.mark.parametrize("mh", [1, 5, 64])
def test_count_never_exceeds_max_history_plus_the_frame(mh):
    cur, hist, pd = T.frames(37, 23)
    acc = hist
    for k, m in enumerate(("random", "fraction", "identity", "integer", "random", "identity")):
        acc = T.accumulate(cur, acc, T.motion(m, 37, 23), pd, max_history=mh)
        assert (acc["count"] <= mh + cur["count"]).all() and (acc["count"] >= cur["count"]).all()
    assert (acc["count"] == mh + cur["count"]).any()


def test_the_variance_of_an_accumulated_plane_falls_as_one_over_n():
    """initial_variance(count, m1, m2) — the variance of the pixel mean the variance-guided filter starts from — of K
    pooled frames of constant-variance samples: its image mean is sigma^2 / (K c) within the sampling error of the
    estimate (relative 3 * sqrt(2 / (n - 1) / pixels) at three standard deviations)"""
    rng = np.random.default_rng(9)
    shape, c, sigma = (70, 130), 4, 0.25
    xy = T.motion("identity", shape[1], shape[0])
    acc = None
    for K in range(1, 9):
        f, _ = constant_variance_frame(rng, shape, c, sigma=sigma)
        acc = T.accumulate(f, acc, xy, max_history=1000)
        n = K * c
        got, want = float(V.initial_variance(acc["count"], acc["m1"], acc["m2"]).mean()), sigma * sigma / n
        bar = 3.0 * np.sqrt(2.0 / (n - 1) / (shape[0] * shape[1]))
        print(f"{n} samples: mean variance of the mean {got:.4e}, sigma^2 / n {want:.4e}, relative {got / want - 1:+.4f}, bar {bar:.4f}")
        assert (acc["count"] == n).all() and abs(got / want - 1) <= bar
