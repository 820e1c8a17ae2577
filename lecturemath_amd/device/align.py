"""Translation alignment of binary keyframes (lm_align_*)."""
import numpy as np

from .. import _lib
from ._base import Backend, DeviceHandle

ALIGN_MAX_WINDOW = 128      # LM_ALIGN_MAX_WINDOW of csrc/lm_align.hip


class TranslationAligner(DeviceHandle):
    """Aligner.computeTranslationAlignment (AccessMath/preprocessing/content/aligner.py:27-83) for many pairs of equally sized
    images at once (lm_align_* in include/lecturemath_amd.h): the images are packed to bit rows on the device once, the
    (2w + 1)^2 match counts of every pair come from one launch, and the reference's scores are its own divisions on those integers.

    set_images(images)             [n][H][W] or [n][H][W][C] uint8, a numpy array (host) or a torch device tensor (read in place)
    totals()                       ink pixels per image
    match_counts(pairs, w)         int64 [len(pairs)][2w + 1][2w + 1], [dy + w][dx + w]
    align(pairs, w, sort_by=0)     per pair the reference's tuple (f_score, recall, precision, disp_y, disp_x)"""

    DESTROY = "lm_align_destroy"

    def __init__(self, width, height, max_images=64, max_window=ALIGN_MAX_WINDOW, lib=None):
        self.lib = lib or _lib.load()
        self.be = Backend(self.lib)
        self.width, self.height = int(width), int(height)
        self.max_images, self.max_window = int(max_images), int(max_window)
        self.n_images = 0
        self._totals = None
        self._keep = None           # the device tensor an asynchronous set_images is reading
        self._open(self.lib.lm_align_create(self.width, self.height, self.max_images, self.max_window, self.be.stream()))

    def _destroy(self):
        super()._destroy()
        self._keep = None

    def set_images(self, images, content_lum=255, channel=None, on_device=None):
        """images: [n][H][W] uint8, or [n][H][W][C] with `channel` (default 0) naming the plane to read -- in place, nothing is
        copied on the device.  on_device None: a torch tensor is device memory, a numpy array host memory."""
        handle = self._live()
        is_tensor = hasattr(images, "data_ptr")
        if on_device is None:
            on_device = bool(is_tensor and images.is_cuda)
        if is_tensor:
            if str(images.dtype) != "torch.uint8":
                raise ValueError("TranslationAligner.set_images: uint8 images expected, got %s" % images.dtype)
            images = images.contiguous()
        else:
            images = np.asarray(images)
            if images.dtype != np.uint8:
                raise ValueError("TranslationAligner.set_images: uint8 images expected, got %s" % images.dtype)
            images = np.ascontiguousarray(images)
        shape = tuple(int(v) for v in images.shape)
        if len(shape) not in (3, 4) or shape[1:3] != (self.height, self.width):
            raise ValueError("TranslationAligner.set_images: shape %s, expected [n][%d][%d] or [n][%d][%d][C]"
                             % (shape, self.height, self.width, self.height, self.width))
        stride = shape[3] if len(shape) == 4 else 1
        channel = 0 if channel is None else int(channel)
        if not 0 <= channel < stride:
            raise ValueError("TranslationAligner.set_images: channel %d of %d" % (channel, stride))
        n = shape[0]
        self.n_images, self._totals = 0, None
        self.lib.check(self.lib.lm_align_set_images(handle, (_lib.ptr(images) + channel) if n else None, 1 if on_device else 0, n, stride,
                                                    int(content_lum), self.be.stream()))
        self.n_images = n
        self._keep = images if on_device else None
        return self

    def totals(self):
        """int64 numpy array [n_images]"""
        if self._totals is None:
            out = np.zeros(self.n_images, np.int64)
            self.lib.check(self.lib.lm_align_totals(self._live(), out.ctypes.data if self.n_images else None, self.be.stream()))
            self._totals, self._keep = out, None
        return self._totals

    def match_counts(self, pairs, max_window):
        handle = self._live()
        hp = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        w = int(max_window)
        side = 2 * max(w, 0) + 1
        out = np.zeros((len(hp), side, side), np.int32)
        self.lib.check(self.lib.lm_align_run(handle, hp.ctypes.data if len(hp) else None, len(hp), w, out.ctypes.data if len(hp) else None,
                                             self.be.stream()))
        self._keep = None
        return out.astype(np.int64)

    @staticmethod
    def best_alignment(matches, total_first, total_second, sort_by=0):
        """The tuple the reference returns for one pair, from its integer match counts ([2w + 1][2w + 1], dy-major) and ink totals
        (aligner.py:39-83): the first displacement, dy then dx ascending, that attains the maximum of field sort_by."""
        total_first, total_second = int(total_first), int(total_second)
        if total_first == 0 or total_second == 0:
            return 0.0, 0.0, 0.0, 0, 0
        m = np.asarray(matches, np.int64)
        side = m.shape[0]
        w = (side - 1) // 2
        flat = m.reshape(-1)
        # float64 quotients of integers below 2^53 are what Python's int / int gives; the products and sums are IEEE in both
        recall, precision = flat / float(total_first), flat / float(total_second)
        both = recall + precision
        f_score = np.where(both > 0, (2 * recall * precision) / np.where(both > 0, both, 1.0), 0.0)
        disp = np.arange(side, dtype=np.int64) - w
        keys = (f_score, recall, precision, np.repeat(disp, side), np.tile(disp, side))
        k = int(np.argmax(keys[sort_by]))       # first occurrence: the reference's stable sort keeps ties in the original order
        matched = int(flat[k])
        r, p = matched / total_first, matched / total_second
        f = (2 * r * p) / (r + p) if r + p > 0 else 0
        return f, r, p, k // side - w, k % side - w

    def align(self, pairs, max_window, sort_by=0):
        pairs = [(int(i), int(j)) for i, j in pairs]
        counts = self.match_counts(pairs, max_window)
        totals = self.totals()
        return [self.best_alignment(counts[k], totals[i], totals[j], sort_by) for k, (i, j) in enumerate(pairs)]
