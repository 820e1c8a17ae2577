"""The 8-bit grayscale PNG hand-off codec on the device (csrc/lm_png.hip): the compressed_frames / CC_RECONSTRUCTED_OUTPUT
lists the step scripts pass along (FCN_lecturenet_binarizer.py:56, helper.py:31, cc_stability_estimator.py:678).

    pngs = encode_gray8_device(frames)                # device uint8 [n, H, W] -> list of numpy uint8 PNG files
    frames = decode_gray8_device(pngs, width, height) # list of PNG files -> device uint8 [n, H, W]

Host zlib (lecturemath_amd/png.py) stays the default of the drop-in scripts; LM_PNG_CODEC=device (read at call time, see
codec()) switches them to this module.  Encoded files are valid PNGs of other bytes than png.encode_gray8's; decoded pixels
are the same.  Files the device decoder reports UNSUPPORTED (other colour types, bit depths, interlace) are decoded by
png.decode_gray8 and uploaded; a CORRUPT file raises PngDecodeError naming its index.
"""
import os
import struct

import numpy as np

from . import _lib, png
from .device import Backend

BATCH = 64


class PngDecodeError(ValueError):
    def __init__(self, index, msg):
        super().__init__("PNG %d: %s" % (index, msg))
        self.index = index


def codec():
    """'host' (default) or 'device', from the LM_PNG_CODEC environment variable at the time of the call."""
    v = os.environ.get("LM_PNG_CODEC", "host").strip().lower() or "host"
    if v not in ("host", "device"):
        raise ValueError("LM_PNG_CODEC must be 'host' or 'device', not %r" % v)
    return v


def png_size(data):
    """(width, height) from a PNG file's IHDR."""
    head = bytes(np.asarray(data, np.uint8)[:24].tobytes()) if not isinstance(data, (bytes, bytearray)) else bytes(data[:24])
    if head[:8] != png._SIG or head[12:16] != b"IHDR":
        raise ValueError("not a PNG file")
    return struct.unpack(">II", head[16:24])


class PngCodec:
    """Device PNG encoder / decoder for frames of one size (batches of up to max_batch files per library call)."""

    def __init__(self, width, height, max_batch=BATCH, lib=None):
        self.lib = lib or _lib.load()
        self.be = Backend(self.lib)
        self.width, self.height, self.max_batch = int(width), int(height), int(max_batch)
        self.h = self.lib.lm_png_create(self.width, self.height, self.max_batch)
        if not self.h:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, self.lib.last_error())
        self.bound = int(self.lib.lm_png_encode_bound(self.width, self.height))
        self._slots = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.lm_png_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _frames(self, frames):
        if isinstance(frames, np.ndarray):
            frames = np.ascontiguousarray(frames, np.uint8)
            if frames.ndim == 2:
                frames = frames[None]
            return self.be.from_host(frames)
        if len(frames.shape) == 2:
            frames = frames.unsqueeze(0)
        return frames.contiguous()

    def encode(self, frames):
        """uint8 [n, H, W] (device tensor, or numpy) -> list of n numpy uint8 arrays, each a PNG file."""
        frames = self._frames(frames)
        n = int(frames.shape[0])
        assert tuple(int(s) for s in frames.shape[1:]) == (self.height, self.width), "frames of %s, codec for %dx%d" % (
            tuple(frames.shape), self.height, self.width)
        if self._slots is None:
            self._slots = self.be.empty((self.max_batch, self.bound), np.uint8)
            self._sizes = self.be.empty((self.max_batch,), np.int64)
        out = []
        for b0 in range(0, n, self.max_batch):
            m = min(self.max_batch, n - b0)
            self.lib.check(self.lib.lm_png_encode(self.h, _lib.ptr(frames[b0:b0 + m]), m, _lib.ptr(self._slots), self.bound,
                                                  _lib.ptr(self._sizes), self.be.stream()))
            sizes = self.be.to_host(self._sizes[:m]).astype(np.int64)
            offs = np.zeros(m + 1, np.int64)
            np.cumsum(sizes, out=offs[1:])
            packed = self.be.empty((int(offs[-1]),), np.uint8)
            d_offs = self.be.from_host(offs[:m])
            self.lib.check(self.lib.lm_png_pack(_lib.ptr(self._slots), self.bound, _lib.ptr(self._sizes), _lib.ptr(d_offs), m, _lib.ptr(packed),
                                                self.be.stream()))
            host = self.be.to_host(packed)                     # the one copy of the compressed bytes
            out.extend(host[offs[i]:offs[i + 1]].copy() for i in range(m))
        return out

    def decode(self, pngs, out=None):
        """list of PNG files (bytes / numpy uint8) -> device uint8 [n, H, W] (written into `out` when given)."""
        n = len(pngs)
        if out is None:
            out = self.be.empty((n, self.height, self.width), np.uint8)
        for b0 in range(0, n, self.max_batch):
            batch = [np.frombuffer(p, np.uint8) if isinstance(p, (bytes, bytearray)) else np.asarray(p, np.uint8).reshape(-1)
                     for p in pngs[b0:b0 + self.max_batch]]
            m = len(batch)
            lens = np.asarray([len(p) for p in batch], np.int64)
            offs = np.zeros(m, np.int64)
            np.cumsum(lens[:-1], out=offs[1:])
            # offsets, lengths and files in one buffer: one host-to-device copy
            host = np.empty(16 * m + int(lens.sum()), np.uint8)
            host[:8 * m] = offs.view(np.uint8)
            host[8 * m:16 * m] = lens.view(np.uint8)
            if m:
                host[16 * m:] = np.concatenate(batch)
            dev = self.be.from_host(host)
            status = self.be.empty((m,), np.int32)
            base = _lib.ptr(dev)
            self.lib.check(self.lib.lm_png_decode(self.h, base + 16 * m, base, base + 8 * m, m, _lib.ptr(out[b0:b0 + m]), _lib.ptr(status),
                                                  self.be.stream()))
            st = self.be.to_host(status)
            for i in np.flatnonzero(st != _lib.LM_PNG_OK):
                if st[i] == _lib.LM_PNG_CORRUPT:
                    raise PngDecodeError(b0 + int(i), "corrupt (or not %dx%d)" % (self.width, self.height))
                frame = png.decode_gray8(batch[i])              # UNSUPPORTED: a PNG flavour the device decoder leaves to the host
                if frame is None or frame.shape != (self.height, self.width):
                    raise PngDecodeError(b0 + int(i), "not a %dx%d frame" % (self.width, self.height))
                self._put(out, b0 + int(i), frame)
        return out

    def _put(self, out, i, frame):
        if self.be.device:
            out[i].copy_(self.be.torch.from_numpy(np.ascontiguousarray(frame, np.uint8)))
        else:
            out[i] = frame


_codecs = {}


def get_codec(width, height, lib=None):
    """A cached PngCodec per (library, size)."""
    lib = lib or _lib.load()
    key = (id(lib), int(width), int(height))
    c = _codecs.get(key)
    if c is None or c.lib is not lib:
        c = _codecs[key] = PngCodec(width, height, BATCH, lib)
    return c


def encode_gray8_device(frames, lib=None):
    """uint8 [n, H, W] or [H, W] (device tensor, or numpy on the emulated build) -> list of numpy uint8 PNG files."""
    h, w = int(frames.shape[-2]), int(frames.shape[-1])
    return get_codec(w, h, lib).encode(frames)


def decode_gray8_device(pngs, width, height, lib=None):
    """list of 8-bit grayscale PNG files of width x height -> device uint8 [n, height, width]."""
    return get_codec(width, height, lib).decode(pngs)
