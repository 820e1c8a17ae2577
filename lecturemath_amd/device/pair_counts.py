"""Shared ink of pairs of connected components on a bit-row table (lm_kf_pair_counts): the integer primitive of the summary evaluation."""
import numpy as np

from .. import _lib
from ._base import Backend, DeviceHandle, call_with_room, csr, flatten_images

CC_PAIR_MAX_RADIUS = 8      # LM_CCM_MAX_RADIUS of csrc/lm_ccmatch.hip


class _PairCounts(DeviceHandle):
    """counts() of a bit-row table (the handle is its LmKeyframes, self.calls the lm_kf_pair_counts calls made)"""

    DESTROY = "lm_kf_destroy"

    def counts(self, queries, radius, cap=None):
        handle = self._live()
        queries = list(queries)
        n_q, r = len(queries), int(radius)
        a_off, a_items = csr([q[0] for q in queries])
        b_off, b_items = csr([q[1] for q in queries])
        disp = np.ascontiguousarray(np.asarray([q[2] for q in queries], np.int64).reshape(n_q, 2))
        if n_q and np.abs(disp).max() > 0x7fffffff:
            raise ValueError("CCPairCounts.counts: displacement beyond int32")
        disp = np.ascontiguousarray(disp.astype(np.int32))
        side = 2 * max(r, 0) + 1

        def call(room):
            rows = np.zeros((room, 3), np.int32)
            counts = np.zeros((room, side, side), np.int32)
            found = np.zeros(1, np.int64)
            self.calls += 1
            rc = self.lib.lm_kf_pair_counts(handle, a_off.ctypes.data, a_items.ctypes.data, b_off.ctypes.data, b_items.ctypes.data,
                                            disp.ctypes.data if n_q else None, n_q, r, rows.ctypes.data, counts.ctypes.data, room,
                                            found.ctypes.data, self.be.stream())
            return rc, int(found[0]), (rows, counts)

        cap = int(cap) if cap is not None else max(1024, 4 * int(a_off[-1] + b_off[-1]))
        n, (rows, counts) = call_with_room(self.lib, cap, call)      # the retry gets the exact room
        return rows[:n].copy(), counts[:n].astype(np.int64)


class CCPairCounts(_PairCounts):
    """Shared ink of pairs of connected components under a displacement (lm_kf_pair_counts in include/lecturemath_amd.h): the
    integer primitive of the reference's summary evaluation (AccessMath/evaluation/evaluator.py).

    CCPairCounts(cc_lists, width, height)   cc_lists: one list per keyframe of objects with min_x, max_x, min_y, max_y and img
                                            (ConnectedComponent) or of (box, img) tuples, box = (min_x, max_x, min_y, max_y); all of
                                            them become items of one bit-row table, uploaded once.  `extra` appends full images such
                                            as an object mask: (box, img) tuples that form one more list.
    item(k, i)                              table item of element i of list k
    counts(queries, radius)                 queries: (items of A, items of B, (dy, dx)) -> rows int32 [n][3] = (query, position in
                                            A, position in B), sorted, and counts int64 [n][2r + 1][2r + 1], [ey + r][ex + r]"""

    created = 0          # instances made (uploads) in this process; tests assert that the device-keyframe route makes none

    def __init__(self, cc_lists, width, height, extra=(), lib=None):
        CCPairCounts.created += 1
        self.lib = lib or _lib.load()
        self.be = Backend(self.lib)
        self.width, self.height = int(width), int(height)
        lists = [list(lst) for lst in cc_lists] + [list(extra)]
        self.list_off = np.zeros(len(lists) + 1, np.int64)
        self.list_off[1:] = np.cumsum([len(lst) for lst in lists])
        boxes, images = [], []
        for lst in lists:
            for cc in lst:
                box, img = cc if isinstance(cc, tuple) else ((cc.min_x, cc.max_x, cc.min_y, cc.max_y), cc.img)
                boxes.append([int(v) for v in box])
                images.append(np.asarray(img))
        n = len(images)
        hb, off, flat = flatten_images(boxes, images, as_bool=True)
        self._open(self.lib.lm_kf_create_from_images(hb.ctypes.data if n else None, flat.ctypes.data if n else None,
                                                     off.ctypes.data if n else None, n, self.width, self.height, self.be.stream()))
        self.n_items = n
        self.calls = 0              # lm_kf_pair_counts calls made (tests assert that cached results launch nothing)

    def item(self, k, i):
        return int(self.list_off[k]) + int(i)

    def items(self, k):
        """the items of list k (k = -1: the extra list)"""
        k = k % (len(self.list_off) - 1)
        return np.arange(self.list_off[k], self.list_off[k + 1], dtype=np.int32)


class PairTableView:
    """CCPairCounts' interface (item / items / counts / calls) over the items of a live KeyframeCCs: nothing is uploaded."""

    def __init__(self, table, lists, extra_items):
        self.table = table
        self._lists = [np.asarray(lst, np.int32).reshape(-1) for lst in lists] + [np.asarray(extra_items, np.int32).reshape(-1)]
        self.calls = 0

    def close(self):
        pass

    def item(self, k, i):
        return int(self._lists[k][int(i)])

    def items(self, k):
        return self._lists[k % len(self._lists)].copy()

    def counts(self, queries, radius, cap=None):
        before = self.table.calls
        try:
            return self.table.counts(queries, radius, cap)
        finally:
            self.calls += self.table.calls - before
