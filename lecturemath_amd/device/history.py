"""The pixel history of a binary stream (lm_hist_*): per-pixel ink counts and first ink over frame ranges."""
import numpy as np

from .. import _lib
from ._base import Backend, DeviceHandle, csr
from .group_images import GroupImages


class FrameHistory(DeviceHandle):
    """The frames of one binary stream as bit rows on the device (lm_hist_* in include/lecturemath_amd.h): for every pixel, in how
    many frames of a frame range was it ink, and when first?  Serves CCStabilityEstimator.compute_group_images_from_raw_binary and
    KeyframeExtractor.extract.  max_frames * height * ceil(width / 32) * 4 bytes of device memory, allocated here.

    A frame range [t0, t1] holds at most MAX_RANGE frames (the counters are 16 bit-sliced planes)."""

    DESTROY = "lm_hist_destroy"
    MAX_RANGE = 65535
    UPLOAD_BYTES = 256 << 20    # host frames travel in batches of at most this size

    def __init__(self, width, height, max_frames, lib=None):
        self.lib = lib or _lib.load()
        self.be = Backend(self.lib)
        self.width, self.height, self.max_frames = int(width), int(height), int(max_frames)
        self.appends = 0            # append() calls that added frames (tests assert that a shared history uploads once)
        self._open(self.lib.lm_hist_create(self.width, self.height, self.max_frames))

    @classmethod
    def from_frames(cls, frames, lib=None):
        """A history that holds exactly `frames` (host uint8 [n, H, W], a list of [H, W] arrays, or a device uint8 tensor)."""
        if hasattr(frames, "shape"):
            if len(frames.shape) != 3 or int(frames.shape[0]) == 0:
                raise ValueError("FrameHistory: frames of shape %s, expected [n, H, W] with n > 0" % (tuple(frames.shape),))
            n, h, w = (int(v) for v in frames.shape)
        else:
            if len(frames) == 0:
                raise ValueError("FrameHistory: no frames")
            n, (h, w) = len(frames), np.shape(frames[0])
        self = cls(w, h, n, lib)
        try:
            self.append(frames)
        except Exception:
            self.close()
            raise
        return self

    def __len__(self):
        return int(self.lib.lm_hist_count(self._live()))

    def _append_device(self, frames):
        rc = self.lib.lm_hist_append(self.handle, _lib.ptr(frames), int(frames.shape[0]), self.be.stream())
        if rc in (_lib.LM_ERR_ARG, _lib.LM_ERR_CAPACITY):
            raise ValueError(self.lib.last_error())
        self.lib.check(rc)

    def append(self, frames):
        """frames: host uint8 [n, H, W], a list of [H, W] arrays, or a device uint8 tensor [n, H, W]; 255 = ink, 0 = none.  A wrong
        shape, another byte value or more frames than max_frames raise ValueError and leave the history as it was."""
        self._live()
        before = len(self)
        shape = (self.height, self.width)
        if self.be.device and hasattr(frames, "data_ptr"):
            if str(frames.dtype) != "torch.uint8" or frames.dim() != 3 or tuple(frames.shape[1:]) != shape or not frames.is_cuda:
                raise ValueError("FrameHistory.append: device frames must be uint8 [n, %d, %d]" % shape)
            if before + int(frames.shape[0]) > self.max_frames:
                raise ValueError("FrameHistory.append: %d + %d frames, room for %d" % (before, int(frames.shape[0]), self.max_frames))
            if int(frames.shape[0]):
                self._append_device(frames.contiguous())
                self.appends += 1
            return
        if not isinstance(frames, np.ndarray):
            frames = list(frames)
            if any(np.shape(f) != shape for f in frames):
                raise ValueError("FrameHistory.append: every frame must be [%d, %d]" % shape)
        n = len(frames)
        if isinstance(frames, np.ndarray) and (frames.ndim != 3 or frames.shape[1:] != shape):
            raise ValueError("FrameHistory.append: frames of shape %s, expected [n, %d, %d]" % ((frames.shape,) + shape))
        if any(np.asarray(f).dtype != np.uint8 for f in (frames[:1] if isinstance(frames, np.ndarray) else frames)):
            raise ValueError("FrameHistory.append: frames must be uint8")
        if before + n > self.max_frames:
            raise ValueError("FrameHistory.append: %d + %d frames, room for %d" % (before, n, self.max_frames))
        step = max(1, self.UPLOAD_BYTES // (self.height * self.width))
        try:
            for i in range(0, n, step):
                part = frames[i:i + step]
                self._append_device(self.be.from_host(part if isinstance(part, np.ndarray) else np.stack(part)))
        except Exception:
            self.lib.lm_hist_truncate(self.handle, before)
            raise
        if n:
            self.appends += 1

    def ink_counts(self, first=0, count=None):
        """ink pixels of frames first .. first + count - 1 (all from `first` on by default): int64 numpy"""
        handle = self._live()
        count = len(self) - int(first) if count is None else int(count)
        if first < 0 or count < 0 or first + count > len(self):
            raise ValueError("FrameHistory.ink_counts: frames %d .. %d of %d" % (first, first + count - 1, len(self)))
        out = np.zeros(count, np.int64)
        self.lib.check(self.lib.lm_hist_ink_counts(handle, int(first), count, out.ctypes.data))
        return out

    def frame(self, t):
        """frame t as the host uint8 0 / 255 array it was appended as"""
        handle = self._live()
        if not 0 <= int(t) < len(self):
            raise IndexError("FrameHistory.frame: frame %d of %d" % (t, len(self)))
        wpr = (self.width + 31) >> 5
        words = np.zeros((self.height, wpr), "<u4")
        self.lib.check(self.lib.lm_hist_read_bits(handle, int(t), 1, words.ctypes.data, self.be.stream()))
        bits = np.unpackbits(words.view(np.uint8).reshape(self.height, wpr * 4), axis=1, bitorder="little")
        return (bits[:, :self.width] * 255).astype(np.uint8)

    def _check_range(self, t0, t1, who):
        n = len(self)
        if not (0 <= t0 <= t1 < n):
            raise ValueError("%s: frame range [%d, %d] outside the %d frames held (or empty)" % (who, t0, t1, n))
        if t1 - t0 + 1 > self.MAX_RANGE:
            raise ValueError("%s: frame range [%d, %d] is longer than %d frames" % (who, t0, t1, self.MAX_RANGE))

    def segment_stats(self, t0, t1, host=False):
        """(sum, age) float32 [H, W] over the frames t0 .. t1 (inclusive): frames with ink, and the index of the first frame with ink
        (0 where none).  Device tensors, or numpy arrays with host=True."""
        handle = self._live()
        t0, t1 = int(t0), int(t1)
        self._check_range(t0, t1, "FrameHistory.segment_stats")
        both = self.be.empty((2, self.height, self.width), np.float32)
        self.lib.check(self.lib.lm_hist_segment_stats(handle, t0, t1, _lib.ptr(both[0]), _lib.ptr(both[1]), self.be.stream()))
        if host:
            both = self.be.to_host(both)
            return both[0].copy(), both[1].copy()
        return both[0], both[1]

    def masked_images(self, masks, boxes, ranges, mask_lists, threshold, item_first=None):
        """One image per job: job j has the box boxes[j] = (min_x, max_x, min_y, max_y), the frames ranges[j] = (t0, t1) inclusive and
        the items mask_lists[j] of the GroupImages `masks`; its image is ((c * 255) // max c) > threshold, c = frames of the range
        whose pixel is ink under the OR of the mask items.  Returns (GroupImages of the images in job order, maxima int64)."""
        handle = self._live()
        n = len(boxes)
        if len(ranges) != n or len(mask_lists) != n:
            raise ValueError("FrameHistory.masked_images: %d boxes, %d ranges, %d mask lists" % (n, len(ranges), len(mask_lists)))
        if not isinstance(masks, GroupImages) or (masks.width, masks.height) != (self.width, self.height):
            raise ValueError("FrameHistory.masked_images: masks must be a GroupImages placed in the %d x %d frame" % (self.width, self.height))
        if threshold != threshold:
            raise ValueError("FrameHistory.masked_images: threshold is NaN")
        hb = np.ascontiguousarray(np.asarray(boxes, np.int64).reshape(n, 4))
        hr = np.ascontiguousarray(np.asarray(ranges, np.int64).reshape(n, 2))
        held = len(self)
        wrong = np.flatnonzero((hr[:, 0] < 0) | (hr[:, 1] < hr[:, 0]) | (hr[:, 1] >= held) | (hr[:, 1] - hr[:, 0] + 1 > self.MAX_RANGE))
        if len(wrong):
            self._check_range(int(hr[wrong[0], 0]), int(hr[wrong[0], 1]), "FrameHistory.masked_images")
        bad = (hb[:, 0] < 0) | (hb[:, 2] < 0) | (hb[:, 1] < hb[:, 0]) | (hb[:, 3] < hb[:, 2]) | (hb[:, 1] >= self.width) | (hb[:, 3] >= self.height)
        if bad.any():
            raise ValueError("FrameHistory.masked_images: box %s outside the %d x %d frame" % (tuple(hb[np.flatnonzero(bad)[0]]), self.width, self.height))
        off, flat = csr(mask_lists)
        if off[-1] and (flat.min() < 0 or flat.max() >= len(masks)):
            raise ValueError("FrameHistory.masked_images: a mask item outside the table of %d" % len(masks))
        hb, hr = hb.astype(np.int32), hr.astype(np.int32)
        maxima = np.zeros(n, np.int64)
        out = self.lib.lm_hist_masked_images(handle, masks._live(), hb.ctypes.data, hr.ctypes.data, off.ctypes.data, flat.ctypes.data, n,
                                             float(threshold), maxima.ctypes.data, self.be.stream())
        if not out:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, self.lib.last_error())
        shapes = np.stack([hb[:, 3] - hb[:, 2] + 1, hb[:, 1] - hb[:, 0] + 1], axis=1).astype(np.int64)
        return GroupImages(self.lib, out, self.width, self.height, shapes, item_first=item_first), maxima


def as_frame_history(frames, lib=None):
    """(history, owned): `frames` itself when it is a FrameHistory, else a new one that holds them (the caller closes it)"""
    if isinstance(frames, FrameHistory):
        return frames, False
    return FrameHistory.from_frames(frames, lib), True
