"""CPU side of moving the vertices of meshes of any resident scene, two-level ones included (take_hip_scene_update_meshes,
include/take_hip.h): the symbol is exported, declared to ctypes and bound by capi.Scene, it is no new ABI version and no
new struct, every refusal that needs no scene comes with TAKE_E_INVALID and a message before the device is looked at,
and a well-formed call without a device is TAKE_E_NO_GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from take_amd import capi
from take_amd import cdefs as D

NAME = "take_hip_scene_update_meshes"
OLD = "take_hip_scene_set_mesh_vertices"


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def updates(*recs):
    """(mesh, flags, positions, normals) tuples -> a TakeMeshUpdate array"""
    out = (D.TakeMeshUpdate * max(len(recs), 1))()
    for k, (mesh, flags, pos, nrm) in enumerate(recs):
        out[k].mesh, out[k].flags, out[k].positions, out[k].normals = mesh, flags, pos, nrm
    return out


def test_the_symbol_is_exported_and_declared(lib):
    assert NAME in capi.EXPORTS and hasattr(lib, NAME)
    assert getattr(lib, NAME).argtypes == D.SCENE_UPDATE_PROTOTYPES[NAME]
    assert D.SCENE_UPDATE_PROTOTYPES[NAME] == D.SCENE_UPDATE_PROTOTYPES[OLD]  # TakeMeshUpdate is reused
    assert callable(capi.Scene.update_meshes) and callable(capi.Scene.set_mesh_vertices)
    assert C.sizeof(D.TakeMeshUpdate) == 24
    assert lib.take_hip_abi_version() == 5  # a new symbol is no new ABI version


def test_the_header_declares_it():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "take_hip.h")
    with open(header) as f:
        text = f.read()
    assert f"int {NAME}(TakeScene *scene, const TakeMeshUpdate *updates, int32_t n_updates);" in text
    assert f"int {OLD}(TakeScene *scene, const TakeMeshUpdate *updates, int32_t n_updates);" in text


def test_refusals_that_need_no_scene(lib):
    """TAKE_E_INVALID, not TAKE_E_NO_GPU: these arguments are looked at before the device — and before the scene — is;
    the messages are take_hip_scene_set_mesh_vertices' own"""
    handle = C.cast((C.c_char * 64)(), C.c_void_p)  # never read
    pos = np.zeros((4, 3))
    p = pos.ctypes.data
    cases = [
        (None, updates((0, 0, p, None)), 1, b"null argument"),
        (handle, None, 1, b"null argument"),
        (handle, updates((0, 0, p, None)), 0, b"n_updates"),
        (handle, updates((0, 0, p, None)), -3, b"n_updates"),
        (handle, updates((-1, 0, p, None)), 1, b"out of range"),
        (handle, updates((0, 0, p, None), (1, 0, None, None)), 2, b"positions is null"),
        (handle, updates((0, 2, p, None)), 1, b"unknown flag"),
        (handle, updates((0, D.TAKE_MESH_DEVICE_ARRAYS | 4, p, None)), 1, b"unknown flag"),
        (handle, updates((3, 0, p, None), (1, 0, p, None), (3, 0, p, p)), 3, b"more than once"),
    ]
    for scene, recs, n, message in cases:
        lib.take_hip_scene_build_info(None, None, None)  # (leaves another message behind)
        assert getattr(lib, NAME)(scene, recs, n) == D.TAKE_E_INVALID, message
        ours = lib.take_hip_last_error()
        assert message in ours, (message, ours)
        lib.take_hip_scene_build_info(None, None, None)
        assert getattr(lib, OLD)(scene, recs, n) == D.TAKE_E_INVALID
        assert lib.take_hip_last_error() == ours  # the argument checks are shared


def test_without_gpu_a_well_formed_call_is_no_gpu(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the no-GPU contract is checked in the CPU container")
    handle = (C.c_char * 64)()  # never read: without a device no scene exists, and the entry point says so first
    pos = np.zeros((4, 3))
    recs = updates((0, 0, pos.ctypes.data, pos.ctypes.data), (2, D.TAKE_MESH_DEVICE_ARRAYS, pos.ctypes.data, None))
    assert getattr(lib, NAME)(C.cast(handle, C.c_void_p), recs, 2) == D.TAKE_E_NO_GPU
