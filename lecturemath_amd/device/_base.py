"""What every module of the package shares: the buffer backend, the lifecycle of a library handle, and the host-side list
flattening and capacity retry that several entry points of the C ABI ask for."""
import numpy as np

from .. import _lib


class Backend:
    """Allocates buffers the library can address: CUDA(HIP) tensors, or numpy for the emulated build."""

    def __init__(self, lib):
        self.lib = lib
        self.device = lib.is_device_build
        if self.device:
            import torch
            if not torch.cuda.is_available():
                raise _lib.LecturemathLibraryError("liblecturemath_hip.so needs a GPU (torch.cuda.is_available() is False)")
            self.torch = torch

    _T = {np.uint8: "uint8", np.int32: "int32", np.float32: "float32", np.int64: "int64", np.int16: "int16", np.float64: "float64"}

    def empty(self, shape, dtype):
        if self.device:
            return self.torch.empty(shape, dtype=getattr(self.torch, self._T[dtype]), device="cuda")
        # emulated build: 64-byte aligned like device allocations (packed record blocks hold 32-byte aligned structs)
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        raw = np.empty(nbytes + 64, np.uint8)
        off = (-raw.ctypes.data) % 64
        return raw[off:off + nbytes].view(dtype).reshape(shape)

    def from_host(self, a):
        a = np.ascontiguousarray(a)
        if self.device:
            return self.torch.from_numpy(a).cuda()
        return a.copy()

    def to_host(self, x):
        if self.device:
            return x.cpu().numpy()
        return np.asarray(x)

    def stream(self):
        if self.device:
            return self.torch.cuda.current_stream().cuda_stream
        return None

    def synchronize(self):
        if self.device:
            self.torch.cuda.synchronize()


class DeviceHandle:
    """Owner of one library handle (`handle`, made by the subclass with `lib`): close() destroys it once, garbage collection closes,
    pickling is refused and _live() is the handle of an object that is still open."""

    DESTROY = None          # name of the library function that frees the handle
    handle = None

    def _open(self, handle, code=_lib.LM_ERR_ARG):
        """takes what a create function of self.lib returned; NULL raises with the library's message"""
        if not handle:
            raise _lib.LecturemathError(code, self.lib.last_error())
        self.handle = handle

    def _destroy(self):
        """frees self.handle; a subclass wraps what it has to do before or after that"""
        getattr(self.lib, self.DESTROY)(self.handle)

    def close(self):
        if self.handle:
            self._destroy()
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __reduce__(self):
        raise TypeError("%s is a handle to device memory and cannot be pickled" % type(self).__name__)

    def _live(self):
        if self.handle is None:
            raise ValueError("%s: the handle is closed" % type(self).__name__)
        return self.handle


def csr(lists):
    """(offsets int64 [len + 1], concatenated int32 items; one zero stands in for no items at all)"""
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(lst) for lst in lists])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(lst, np.int32).reshape(-1) for lst in lists])) if off[-1] else np.zeros(1, np.int32)
    return off, flat


def flatten_images(boxes, images, as_bool=False):
    """(boxes int32 [n][4], byte offsets int64 [n + 1], the images' bytes end to end) as lm_image_pairs_overlap and
    lm_kf_create_from_images read them; as_bool: every non-zero value becomes 1.  One zero byte stands in for no images."""
    n = len(images)
    hb = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(n, 4))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([im.size for im in images])
    parts = [((im != 0).astype(np.uint8) if as_bool else np.asarray(im, np.uint8)).ravel() for im in images]
    return hb, off, np.ascontiguousarray(np.concatenate(parts)) if n else np.zeros(1, np.uint8)


def call_with_room(lib, cap, call):
    """call(cap) -> (rc, found, buffers) makes one library call with output room for `cap` entries.  All entry points of this kind
    report the full count with LM_ERR_CAPACITY, so one second call with exactly that room suffices.  Returns (found, buffers)."""
    rc, found, out = call(cap)
    if rc == _lib.LM_ERR_CAPACITY and found > cap:
        rc, found, out = call(found)
    lib.check(rc)
    return found, out
