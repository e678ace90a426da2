"""CPU side of the first-hit feature buffers (take_hip_render_features and its _device twin, include/take_hip.h): the
two symbols are exported, declared to ctypes through cdefs.FEATURE_PROTOTYPES and bound by capi.Scene, they are no new
ABI version, and a NULL scene, options or buffer struct is refused with a message before a device is looked for."""
import ctypes as C

import pytest

from take_amd import capi
from take_amd import cdefs as D

SYMBOLS = ("take_hip_render_features", "take_hip_render_features_device")


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_the_two_symbols_are_exported_and_declared(lib):
    assert set(D.FEATURE_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert name in capi.EXPORTS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.FEATURE_PROTOTYPES[name], name
    assert len(D.FEATURE_PROTOTYPES["take_hip_render_features"]) == 3
    assert len(D.FEATURE_PROTOTYPES["take_hip_render_features_device"]) == 4
    assert callable(capi.Scene.render_features) and callable(capi.Scene.render_features_device)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version


def test_the_struct_is_six_pointers_in_the_header_s_order():
    assert [n for n, _ in D.TakeFeatureBuffers._fields_] == ["albedo", "normal", "depth", "alpha", "shape_id", "material_id"]
    assert C.sizeof(D.TakeFeatureBuffers) == 6 * C.sizeof(C.c_void_p)
    assert list(D.FEATURE_PLANES) == [n for n, _ in D.TakeFeatureBuffers._fields_]


def test_null_arguments_are_refused_with_a_message(lib):
    """TAKE_E_INVALID, not TAKE_E_NO_GPU: the arguments are looked at before the device — and before the scene — is.
    (`scene` below is not a scene: a call that went past the argument check would not survive it.)"""
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    opts, bufs = D.TakeRenderOpts(), D.TakeFeatureBuffers()
    opts.spp = 1
    o, b = C.byref(opts), C.byref(bufs)
    calls = [lambda: lib.take_hip_render_features(None, o, b),
             lambda: lib.take_hip_render_features(scene, None, b),
             lambda: lib.take_hip_render_features(scene, o, None),
             lambda: lib.take_hip_render_features_device(None, o, b, None),
             lambda: lib.take_hip_render_features_device(scene, None, b, None),
             lambda: lib.take_hip_render_features_device(scene, o, None, None)]
    for call in calls:
        lib.take_hip_scene_build_info(None, None, None)  # (leaves another message behind)
        assert b"null scene" in lib.take_hip_last_error()
        assert call() == D.TAKE_E_INVALID
        assert b"null argument" in lib.take_hip_last_error()
