"""Step 01's labelling context (lm_ctx_*, lm_threshold*, lm_label_*, lm_cc_stats_*) and the exact frame sums of step 04."""
import numpy as np

from .. import _lib
from ._base import Backend, DeviceHandle


class FrameLabeler(DeviceHandle):
    """Batched scipy.ndimage.label + CC_AgeBoundaries on device frames (labeler.py:126, accessmath_lib.c:357-413)."""

    DESTROY = "lm_ctx_destroy"

    def __init__(self, width, height, max_batch=1, lib=None):
        self.lib = lib or _lib.load()
        self.be = Backend(self.lib)
        self.width, self.height, self.max_batch = width, height, max_batch
        self._open(self.lib.lm_ctx_create(width, height, max_batch), _lib.LM_ERR_HIP)

    @property
    def ctx(self):
        """the LmCtx (the handle under the name the benchmark and the tools read)"""
        return self.handle

    def threshold_invert(self, logits, thr=128):
        """logits: device fp32 array -> device uint8 {0,255}, already inverted (255 = ink)."""
        out = self.be.empty(tuple(logits.shape), np.uint8)
        n = int(np.prod(logits.shape))
        self.lib.check(self.lib.lm_threshold_invert(_lib.ptr(logits), _lib.ptr(out), n, thr, self.be.stream()))
        return out

    def label(self, binary, want_labels=True):
        """binary: device uint8 [B,H,W] -> (device int32 labels [B,H,W] or None, host int32 counts [B])."""
        b = binary.shape[0]
        assert tuple(binary.shape[1:]) == (self.height, self.width) and b <= self.max_batch
        labels = self.be.empty((b, self.height, self.width), np.int32) if want_labels else None
        self.lib.check(self.lib.lm_label_batch(self.handle, _lib.ptr(binary), b, _lib.ptr(labels), self.be.stream()))
        counts = np.zeros(b, np.int32)
        self.lib.check(self.lib.lm_label_counts(self.handle, counts.ctypes.data, self.be.stream()))
        return labels, counts

    def label_logits(self, logits, thr=128, invert=True, want_binary=False, want_labels=True):
        """fp32 logits [B,H,W] -> (labels or None, counts, {0,255} frames or None): threshold (+ the worker's inversion) and labelling in
        one pass over the logits (lm_label_batch_logits)."""
        b = logits.shape[0]
        assert tuple(logits.shape[1:]) == (self.height, self.width) and b <= self.max_batch
        labels = self.be.empty((b, self.height, self.width), np.int32) if want_labels else None
        binary = self.be.empty((b, self.height, self.width), np.uint8) if want_binary else None
        self.lib.check(self.lib.lm_label_batch_logits(self.handle, _lib.ptr(logits), b, thr, 1 if invert else 0, _lib.ptr(binary), _lib.ptr(labels),
                                                      self.be.stream()))
        counts = np.zeros(b, np.int32)
        self.lib.check(self.lib.lm_label_counts(self.handle, counts.ctypes.data, self.be.stream()))
        return labels, counts, binary

    def stats(self, counts):
        """CC_AgeBoundaries arrays of every frame of the last batch: list of int32 [5, n] (mins_y, maxs_y, mins_x, maxs_x, counts)."""
        self.lib.check(self.lib.lm_cc_stats_batch(self.handle, self.be.stream()))
        out = []
        for f, n in enumerate(counts):
            a = np.zeros((5, int(n)), np.int32)
            rows = [a[i].ctypes.data if n else None for i in range(5)]
            self.lib.check(self.lib.lm_cc_stats_read(self.handle, f, int(n), *rows, self.be.stream()))
            out.append(a)
        return out


def frame_sums(frames, lib=None):
    """Exact per-frame sums of a device uint8 tensor [n, H, W] (step 04, VideoSegmenter.compute_binary_sums): int64 numpy."""
    lib = lib or _lib.load()
    be = Backend(lib)
    n = int(frames.shape[0])
    out = be.empty((n,), np.int64)
    lib.check(lib.lm_frame_sums(_lib.ptr(frames), n, int(frames.shape[1]) * int(frames.shape[2]), _lib.ptr(out), be.stream()))
    return be.to_host(out)
