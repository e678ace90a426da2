"""CPU side of re-posing a resident scene (take_hip_scene_set_instance_transforms, its _device twin and
take_hip_scene_set_camera, include/take_hip.h): the three symbols are exported, declared to ctypes and bound by
capi.Scene, they refuse a NULL scene with a message before they look for a device, and they are no new ABI version."""
import ctypes as C

import pytest

from take_amd import capi
from take_amd import cdefs as D

SYMBOLS = ("take_hip_scene_set_instance_transforms", "take_hip_scene_set_instance_transforms_device", "take_hip_scene_set_camera")


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_the_three_symbols_are_exported_and_declared(lib):
    for name in SYMBOLS:
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.SCENE_UPDATE_PROTOTYPES[name], name
    assert len(D.SCENE_UPDATE_PROTOTYPES["take_hip_scene_set_instance_transforms"]) == 3
    assert len(D.SCENE_UPDATE_PROTOTYPES["take_hip_scene_set_instance_transforms_device"]) == 4
    assert callable(capi.Scene.set_instance_transforms) and callable(capi.Scene.set_camera)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version


def test_a_null_scene_is_refused_with_a_message(lib):
    """TAKE_E_INVALID, not TAKE_E_NO_GPU: the arguments are looked at before the device is"""
    x = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    cam = D.TakeCamera(4, 4, D.c_double3(0, 0, 1), D.c_double3(0, 0, 0), D.c_double3(0, 1, 0), 40.0)
    calls = [lambda: lib.take_hip_scene_set_instance_transforms(None, C.cast(x, C.c_void_p), 1),
             lambda: lib.take_hip_scene_set_instance_transforms_device(None, C.cast(x, C.c_void_p), 1, None),
             lambda: lib.take_hip_scene_set_camera(None, C.byref(cam))]
    for call in calls:
        lib.take_hip_scene_build_info(None, None, None)  # (leaves another message behind)
        assert b"null scene" in lib.take_hip_last_error()
        assert call() == D.TAKE_E_INVALID
        assert b"null argument" in lib.take_hip_last_error()
