"""What every wrapper of the binding does to its arguments: arrays and tensors to pointers, streams, and the lifetime of
library handles.  torch is imported only where a call is given a device tensor."""
import ctypes as C

import numpy as np

from ._lib import lib


def on_device(a):
    """a torch tensor in device memory?"""
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def ref(x):
    """a struct by reference; None stays None (a NULL pointer: the library's defaults)"""
    return None if x is None else C.byref(x)


def pointer(a):
    """device pointer of a torch tensor, or the integer itself; None stays None"""
    return None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else int(a))


def required(a, name):
    """`a`, for array() — which lets None through — where an array must be given"""
    if a is None:
        raise ValueError(f"{name} is required")
    return a


def array(a, dtypes, shape, name, device, keep):
    """one array argument -> its pointer (None stays None); what the pointer points into is appended to `keep`, for the
    caller to keep alive and to read the shape of.  `device`: `a` must be a contiguous torch tensor on the device; else
    it is read from host memory through numpy (a host tensor too).  dtypes: a numpy dtype, or a tuple of the dtypes
    taken as they are — anything else in host memory is converted to the first.  shape: a pattern with -1 for a free
    extent, or None = not checked here."""
    if a is None:
        return None
    dtypes = dtypes if isinstance(dtypes, tuple) else (dtypes,)
    if device:
        names = [np.dtype(t).name for t in dtypes]
        if not on_device(a) or str(a.dtype) not in ["torch." + n for n in names] or not a.is_contiguous():
            raise ValueError(f"{name}: arrays on the device must be contiguous {' or '.join(names)} tensors, and all arrays of a call on the device")
        got = tuple(a.shape)
    else:
        a = a.numpy() if hasattr(a, "data_ptr") else a  # (a torch tensor in host memory)
        a = np.ascontiguousarray(a, None if len(dtypes) > 1 and np.asarray(a).dtype in dtypes else dtypes[0])
        got = a.shape
    if shape is not None and (len(got) != len(shape) or any(w >= 0 and g != w for g, w in zip(got, shape))):
        raise ValueError(f"{name} must have shape {tuple('n' if w < 0 else w for w in shape)}, not {tuple(got)}")
    keep.append(a)
    return a.data_ptr() if device else a.ctypes.data


def stream_of(stream, tensor):
    """the stream a call that reads `tensor` runs on or after: `stream`, or torch's current stream on the tensor's device"""
    if stream is None:
        import torch

        stream = torch.cuda.current_stream(tensor.device).cuda_stream
    return stream


def wait_for(stream, device):
    """block until the work queued on `stream` (None: torch's current stream) of `device` is done; device None: no
    device tensor among the arguments, nothing to wait for"""
    if device is not None:
        import torch

        (torch.cuda.current_stream(device) if stream is None else torch.cuda.ExternalStream(int(stream), device=device)).synchronize()


class Closing:
    """close() when the object is collected; an error then is swallowed (interpreter shutdown: the library may be gone)"""

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Handle(Closing):
    """A handle of the library and the name of the entry point that destroys it.  A context manager; close() may be
    called any number of times and destroys once."""
    _h = None
    _destroy = None

    def _new(self):
        """-> what the create call writes the handle through"""
        self._h = C.c_void_p()
        return C.byref(self._h)

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def handle_of(x, cls, what):
    """the handle of an open `cls`, for another call to use"""
    if not isinstance(x, cls) or not x._h:
        raise ValueError(f"{what} must be an open {cls.__name__}")
    return x._h
