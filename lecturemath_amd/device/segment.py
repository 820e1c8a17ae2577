"""Step 04's conflict signal (lm_conflict_signal) and the overlap pairs of host images (lm_image_pairs_overlap)."""
import numpy as np

from .. import _lib
from ._base import Backend, call_with_room, flatten_images


class ConflictSignal:
    """conflicts_per_frame of step 04's conflict-minimisation method (video_segmenter.py:206-278) for any segment of one lecture.

    pairs = (gap_first, gap_last, alive_from, alive_until, weight): five equally long arrays, one entry per conflicting pair of
    groups in the order the reference visits them (lm_conflict_signal in include/lecturemath_amd.h).  They are uploaded once;
    signal(start, end) is one launch and one small copy per node of the recursive split."""

    def __init__(self, pairs, lib=None):
        self.lib = lib or _lib.load()
        self.be = Backend(self.lib)
        gap_first, gap_last, alive_from, alive_until, weight = pairs
        host = [np.ascontiguousarray(a, np.int32) for a in (gap_first, gap_last, alive_from, alive_until)]
        host.append(np.ascontiguousarray(weight, np.float64))
        self.n_pairs = int(host[0].shape[0])
        if any(a.shape != (self.n_pairs,) for a in host):
            raise ValueError("ConflictSignal: the five pair arrays must be one-dimensional and equally long")
        self._dev = [self.be.from_host(a) for a in host] if self.n_pairs else [None] * 5

    def signal(self, start_frame, end_frame):
        """float64 numpy array [end_frame - start_frame + 1]"""
        n = int(end_frame) - int(start_frame) + 1
        if n <= 0:
            raise ValueError("ConflictSignal.signal: empty segment %d..%d" % (start_frame, end_frame))
        out = self.be.empty((n,), np.float64)
        self.lib.check(self.lib.lm_conflict_signal(*[_lib.ptr(a) for a in self._dev], self.n_pairs, int(start_frame), int(end_frame),
                                                   _lib.ptr(out), self.be.stream()))
        return self.be.to_host(out)


def image_pairs_overlap(boxes, images, lib=None):
    """Pairs (i < j), sorted, of {0,255} images placed at their boxes (min_x, max_x, min_y, max_y inclusive) that share an ink
    pixel (step 05: compute_overlapping_CC_groups / keyframe conflicts).  Box join + bit tests on the device."""
    lib = lib or _lib.load()
    n = len(images)
    if n < 2:
        return []
    hb, off, flat = flatten_images(boxes, images)
    be = Backend(lib)

    def call(cap):
        pairs = np.zeros((cap, 2), np.int32)
        found = np.zeros(1, np.int64)
        rc = lib.lm_image_pairs_overlap(hb.ctypes.data, flat.ctypes.data, off.ctypes.data, n, pairs.ctypes.data, cap, found.ctypes.data, be.stream())
        return rc, int(found[0]), pairs

    found, pairs = call_with_room(lib, max(1024, 8 * n), call)
    return [(int(a), int(b)) for a, b in pairs[:found]]
