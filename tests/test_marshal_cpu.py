"""What every wrapper of the binding shares (take_amd/_marshal.py), without a GPU: host arrays and stand-ins for device
tensors through array(), and the lifetime of a library handle with a recording destroy function."""
import ctypes as C
import gc

import numpy as np
import pytest

from take_amd import _marshal as M


class FakeTensor:
    """what array() reads of a torch device tensor"""

    def __init__(self, shape, dtype="torch.float64", is_cuda=True, contiguous=True, device="cuda:0"):
        self.shape, self.dtype, self.is_cuda, self.device, self._contiguous = shape, dtype, is_cuda, device, contiguous

    def data_ptr(self):
        return 0x1000

    def is_contiguous(self):
        return self._contiguous


def test_host_array_is_converted_kept_and_pointed_at():
    keep = []
    ptr = M.array([[1, 2, 3], [4, 5, 6]], np.float64, (-1, 3), "positions", False, keep)
    assert len(keep) == 1 and keep[0].dtype == np.float64 and keep[0].shape == (2, 3) and keep[0].flags.c_contiguous
    assert ptr == keep[0].ctypes.data
    assert np.array_equal(keep[0], [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    # an array that already fits is the one kept; a strided one is copied
    a = np.arange(6, dtype=np.float64).reshape(2, 3)
    assert M.array(a, np.float64, (2, 3), "a", False, keep) == a.ctypes.data and keep[-1] is a
    assert M.array(a.T, np.float64, (3, 2), "a", False, keep) == keep[-1].ctypes.data and keep[-1].flags.c_contiguous


def test_none_stays_none_and_keeps_nothing():
    keep = []
    assert M.array(None, np.float64, (-1, 3), "normals", False, keep) is None
    assert M.array(None, np.float64, (-1, 3), "normals", True, keep) is None
    assert keep == []
    with pytest.raises(ValueError, match="positions is required"):
        M.required(None, "positions")
    assert M.required(0, "n") == 0


def test_free_extents_an_empty_array_and_an_unchecked_shape():
    keep = []
    M.array(np.zeros((1, 3)), np.float64, (-1, 3), "positions", False, keep)
    M.array(np.zeros((0, 3)), np.float64, (-1, 3), "positions", False, keep)
    M.array(np.zeros((2, 3), np.int32), np.int32, (2, -1), "joints", False, keep)
    M.array(np.zeros(7), np.float64, None, "anything", False, keep)
    assert [a.shape for a in keep] == [(1, 3), (0, 3), (2, 3), (7,)]


@pytest.mark.parametrize("shape, got", [((-1, 3), (2, 2)), ((1, 3), (2, 3)), ((-1, 3), (3,)), ((-1, 3), (1, 2, 3))])
def test_wrong_shape_is_refused_by_name(shape, got):
    keep = []
    with pytest.raises(ValueError, match="weights must have shape") as e:
        M.array(np.zeros(got), np.float64, shape, "weights", False, keep)
    assert str(tuple("n" if w < 0 else w for w in shape)) in str(e.value) and str(got) in str(e.value)
    assert keep == []


def test_a_set_of_dtypes_keeps_its_members_and_converts_the_rest_to_the_first():
    keep = []
    for given, kept in ((np.float32, np.float32), (np.float64, np.float64), (np.int32, np.float64), (np.float16, np.float64)):
        M.array(np.ones((1, 1, 3), given), (np.float64, np.float32), (-1, -1, 3), "image", False, keep)
        assert keep[-1].dtype == kept
    M.array([[[1, 2, 3]]], (np.float64, np.float32), (-1, -1, 3), "image", False, keep)
    assert keep[-1].dtype == np.float64


def test_device_tensor_is_taken_by_its_pointer():
    keep = []
    t = FakeTensor((2, 3))
    assert M.on_device(t) and not M.on_device(np.zeros(3)) and not M.on_device(FakeTensor((2, 3), is_cuda=False))
    assert M.array(t, np.float64, (-1, 3), "positions", True, keep) == 0x1000 and keep == [t]
    f = FakeTensor((1, 1, 3), "torch.float32")
    assert M.array(f, (np.float64, np.float32), (-1, -1, 3), "image", True, keep) == 0x1000 and keep[-1] is f
    assert M.pointer(t) == 0x1000 and M.pointer(77) == 77 and M.pointer(None) is None


@pytest.mark.parametrize("bad", [FakeTensor((2, 3), "torch.float32"), FakeTensor((2, 3), contiguous=False), np.zeros((2, 3)),
                                 FakeTensor((2, 3), is_cuda=False)],
                         ids=["dtype", "strided", "host_array", "host_tensor"])
def test_device_branch_refusals(bad):
    keep = []
    with pytest.raises(ValueError, match="normals: arrays on the device must be contiguous float64 tensors"):
        M.array(bad, np.float64, (-1, 3), "normals", True, keep)
    assert keep == []


def test_device_tensor_of_a_wrong_shape_is_refused():
    with pytest.raises(ValueError, match="cage must have shape"):
        M.array(FakeTensor((2, 2)), np.float64, (2, 3), "cage", True, [])


def test_ref():
    x = C.c_int32(5)
    assert M.ref(None) is None
    assert C.cast(M.ref(x), C.POINTER(C.c_int32)).contents.value == 5


class FakeLib:
    def __init__(self, fail=False):
        self.destroyed, self.fail = [], fail

    def thing_destroy(self, h):
        self.destroyed.append(h.value)
        if self.fail:
            raise OSError("the library is gone")


class Thing(M.Handle):
    _destroy = "thing_destroy"

    def __init__(self, value=0x40):
        C.cast(self._new(), C.POINTER(C.c_void_p)).contents.value = value


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(M, "lib", lambda: lib)
    return lib


def test_close_destroys_once(fake):
    t = Thing()
    assert t._h and t._h.value == 0x40
    t.close()
    assert not t._h and fake.destroyed == [0x40]
    t.close()
    assert fake.destroyed == [0x40]
    t.__del__()
    assert fake.destroyed == [0x40]


def test_with_closes_and_handle_of_wants_an_open_handle(fake):
    with Thing(0x50) as t:
        assert M.handle_of(t, Thing, "thing") is t._h and fake.destroyed == []
    assert fake.destroyed == [0x50]
    with pytest.raises(ValueError, match="thing must be an open Thing"):
        M.handle_of(t, Thing, "thing")
    with pytest.raises(ValueError, match="thing must be an open Thing"):
        M.handle_of(object(), Thing, "thing")


def test_collection_destroys_and_swallows_what_destroy_raises(fake):
    Thing(0x60)
    gc.collect()
    assert fake.destroyed == [0x60]
    fake.fail = True
    t = Thing(0x70)
    with pytest.raises(OSError):
        t.close()
    t.__del__()  # (the handle is still set: destroy is tried again, and its error goes nowhere)
    assert fake.destroyed == [0x60, 0x70, 0x70]
    t._h = None  # (nothing is left for the collector to close)


def test_a_handle_that_was_never_created_closes_quietly(fake):
    class Unborn(M.Handle):
        _destroy = "thing_destroy"

    Unborn().close()
    assert fake.destroyed == []
