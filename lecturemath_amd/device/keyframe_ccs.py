"""The connected components of keyframes as one bit-row table (lm_kf_create_from_frames) with lazily read CC objects, and the pixel
sums of the summary evaluation (lm_kf_pixel_sums)."""
import weakref

import numpy as np

from .. import _lib
from ._base import Backend
from .pair_counts import PairTableView, _PairCounts

def _plain_cc(cls, state):
    cc = cls.__new__(cls)
    cc.__dict__.update(state)
    return cc


_plain_cc.__module__ = "lecturemath_amd.device"      # the name pickles of a device-backed CC carry; the package re-exports it

_device_cc = {}


def device_cc_class():
    """ConnectedComponent subclass whose `img` is read from a KeyframeCCs table on first access.  It remembers its table, its item
    and the item's box (a CC moved by translateBox no longer is that item); it pickles as a plain ConnectedComponent."""
    from AM_CommonTools.data.connected_component import ConnectedComponent
    cls = _device_cc.get(ConnectedComponent)
    if cls is None:
        class DeviceConnectedComponent(ConnectedComponent):
            def __init__(self, table, item, cc_id, min_x, max_x, min_y, max_y, size):
                self._img, self._own_img = None, False
                self.table, self.item = table, int(item)
                self.item_box = (int(min_x), int(max_x), int(min_y), int(max_y))
                ConnectedComponent.__init__(self, cc_id, min_x, max_x, min_y, max_y, size, None)

            @property
            def img(self):
                if self._img is None:
                    self._img = self.table.image(self.item)
                return self._img

            @img.setter
            def img(self, value):
                self._img, self._own_img = value, value is not None

            def in_place(self):
                """the CC still is its item: same box, image not replaced"""
                return not self._own_img and (int(self.min_x), int(self.max_x), int(self.min_y), int(self.max_y)) == self.item_box

            def __reduce__(self):
                state = {k: v for k, v in self.__dict__.items() if k not in ("_img", "_own_img", "table", "item", "item_box")}
                state["img"] = self.img
                return (_plain_cc, (ConnectedComponent, state))

        cls = _device_cc[ConnectedComponent] = DeviceConnectedComponent
    return cls


class KeyframeCCs(_PairCounts):
    """The connected components of keyframes resident on the device as one bit-row table (lm_kf_create_from_frames in
    include/lecturemath_amd.h): KeyFrameAnnotation.update_binary_cc (AccessMath/annotation/keyframe_annotation.py:139-146) for a whole
    keyframe set without the per-keyframe host round trip.  The table is what CCPairCounts uploads, so the summary evaluation counts
    on it directly.

    from_frames(frames, masks)   frames [n][H][W] or [n][H][W][C] uint8 (channel 0 is read; ink iff != 255), a numpy array or a torch
                                 device tensor; masks [n][H][W], non-zero = object, or None
    frame_off, records           int64 [n + 1] and int32 [n_cc][6] = cc_id, min_x, max_x, min_y, max_y, size
    items(k), mask_item(k)       table items of keyframe k's CCs (ascending label) and of its mask
    image(item)                  uint8 0 / 255 image of an item
    counts(queries, radius)      as CCPairCounts.counts
    ccs(k)                       what the overlay's Labeler.extractSpatioTemporalContent(255 - channel0, zeros, False) returns, with
                                 images read from the table on first access"""

    def __init__(self, lib, handle, width, height, n_frames, n_masks):
        self.lib = lib
        self.be = Backend(lib)
        self.handle = handle
        self.width, self.height, self.n_frames, self.n_masks = int(width), int(height), int(n_frames), int(n_masks)
        self.calls = 0
        self.frame_off = np.zeros(self.n_frames + 1, np.int64)
        lib.check(lib.lm_kf_cc_records(handle, self.frame_off.ctypes.data, None))
        n_cc = int(self.frame_off[-1])
        self.records = np.zeros((n_cc, 6), np.int32)
        lib.check(lib.lm_kf_cc_records(handle, None, self.records.ctypes.data if n_cc else None))
        self.n_items = int(lib.lm_kf_count(handle))
        self._ccs = {}
        self._mask_arrays = {}      # id(host array) -> (the array, its mask item): how the evaluator recognises a mask of this table
        KeyframeCCs._tables.add(self)

    _tables = weakref.WeakSet()

    def register_mask(self, k, array):
        """`array` (the host object_mask of keyframe k, not to be modified afterwards) stands for mask item k"""
        self._mask_arrays[id(array)] = (array, self.mask_item(k))

    @classmethod
    def mask_owner(cls, array):
        """(table, item) of a registered mask array of a live table, by identity; or None"""
        for table in list(cls._tables):
            hit = table._mask_arrays.get(id(array))
            if hit is not None and hit[0] is array and table.live:
                return table, hit[1]
        return None

    @classmethod
    def pair_view(cls, cc_lists, extra=()):
        """A PairTableView when every CC of every list is a device-backed CC of ONE live table that still is its item and every extra
        is a registered mask of that table; else None (the caller uploads)."""
        table, lists, extras = None, [], []
        for lst in cc_lists:
            items = []
            for cc in lst:
                t = getattr(cc, "table", None)
                if not isinstance(t, cls) or (table is not None and t is not table) or not cc.in_place():
                    return None
                table = t
                items.append(cc.item)
            lists.append(items)
        for _, img in extra:
            hit = cls.mask_owner(img)
            if hit is None or (table is not None and hit[0] is not table):
                return None
            table = hit[0]
            extras.append(hit[1])
        if table is None or not table.live:
            return None
        return PairTableView(table, lists, extras)

    @staticmethod
    def _side(x, be, on_device, name):
        """`x` as contiguous uint8 memory on the side the frames live on"""
        if hasattr(x, "data_ptr"):
            if str(x.dtype) == "torch.bool":
                x = x.to(be.torch.uint8)
            if str(x.dtype) != "torch.uint8":
                raise ValueError("KeyframeCCs.from_frames: %s must be uint8, got %s" % (name, x.dtype))
            x = x.contiguous()
            return (x if x.is_cuda else x.cuda()) if on_device else x.cpu().numpy()
        x = np.asarray(x)
        if x.dtype == np.bool_:
            x = x.astype(np.uint8)
        if x.dtype != np.uint8:
            raise ValueError("KeyframeCCs.from_frames: %s must be uint8, got %s" % (name, x.dtype))
        x = np.ascontiguousarray(x)
        return be.from_host(x) if on_device else x

    @classmethod
    def from_frames(cls, frames, masks=None, min_pixels=1, max_batch=8, lib=None):
        lib = lib or _lib.load()
        be = Backend(lib)
        on_device = bool(hasattr(frames, "data_ptr") and frames.is_cuda)
        frames = cls._side(frames, be, on_device, "frames")
        shape = tuple(int(v) for v in frames.shape)
        if len(shape) not in (3, 4) or min(shape[1:3]) < 1:
            raise ValueError("KeyframeCCs.from_frames: frames of shape %s, expected [n][H][W] or [n][H][W][C]" % (shape,))
        n, height, width = shape[:3]
        stride = shape[3] if len(shape) == 4 else 1
        if stride < 1 or int(min_pixels) < 0 or int(max_batch) < 1:
            raise ValueError("KeyframeCCs.from_frames: bad arguments (channels=%d, min_pixels=%r, max_batch=%r)" % (stride, min_pixels, max_batch))
        n_masks = 0
        if masks is not None:
            masks = cls._side(masks, be, on_device, "masks")
            if tuple(int(v) for v in masks.shape) != (n, height, width):
                raise ValueError("KeyframeCCs.from_frames: masks of shape %s, expected %s" % (tuple(masks.shape), (n, height, width)))
            n_masks = n
        ctx = lib.lm_ctx_create(width, height, max(1, min(int(max_batch), n)))
        if not ctx:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, lib.last_error())
        try:
            handle = lib.lm_kf_create_from_frames(ctx, _lib.ptr(frames) if n else None, 1 if on_device else 0, n, stride,
                                                  _lib.ptr(masks) if n_masks else None, n_masks, int(min_pixels), be.stream())
            if not handle:
                raise _lib.LecturemathError(_lib.LM_ERR_ARG, lib.last_error())
        finally:
            lib.lm_ctx_destroy(ctx)
        try:
            return cls(lib, handle, width, height, n, n_masks)
        except Exception:
            lib.lm_kf_destroy(handle)
            raise

    def __len__(self):
        return self.n_items

    @property
    def live(self):
        return self.handle is not None

    def _frame(self, k):
        k = int(k)
        if not 0 <= k < self.n_frames:
            raise IndexError("KeyframeCCs: keyframe %d of %d" % (k, self.n_frames))
        return k

    def items(self, k):
        k = self._frame(k)
        return np.arange(self.frame_off[k], self.frame_off[k + 1], dtype=np.int32)

    def mask_item(self, k):
        k = self._frame(k)
        if not self.n_masks:
            raise ValueError("KeyframeCCs: the table was made without masks")
        return int(self.frame_off[-1]) + k

    def box(self, item):
        """(min_x, max_x, min_y, max_y) of an item"""
        item = int(item)
        if item < int(self.frame_off[-1]):
            return tuple(int(v) for v in self.records[item, 1:5])
        return (0, self.width - 1, 0, self.height - 1)

    def image(self, item):
        handle = self._live()
        item = int(item)
        if not 0 <= item < self.n_items:
            raise IndexError("KeyframeCCs: item %d of %d" % (item, self.n_items))
        b = self.box(item)
        out = np.zeros((b[3] - b[2] + 1, b[1] - b[0] + 1), np.uint8)
        self.lib.check(self.lib.lm_kf_image(handle, item, out.ctypes.data, out.size, self.be.stream()))
        return out

    def ccs(self, k):
        """the CC objects of keyframe k (the same list on every call)"""
        self._live()
        k = self._frame(k)
        if k not in self._ccs:
            cls = device_cc_class()
            out = []
            for item in range(int(self.frame_off[k]), int(self.frame_off[k + 1])):
                cc_id, mnx, mxx, mny, mxy, size = (np.int32(v) for v in self.records[item])
                cc = cls(self, item, int(cc_id), mnx, mxx, mny, mxy, size)
                cc.start_time = cc.end_time = np.float32(0.0)
                out.append(cc)
            self._ccs[k] = out
        return self._ccs[k]


def pixel_sums(gt, summ, masks=None, lib=None):
    """The integer sums of Evaluator.compute_pixel_binary_metrics for pairs of keyframes (lm_kf_pixel_sums): gt, summ [n][H][W] or
    [n][H][W][C] uint8 on the device (channel 0 is read in place), masks [n][H][W] uint8 on the device or None.  uint64 numpy [n][4] =
    sum(255 - gt), sum(255 - summ), sum(255 - summ where gt != 255), sum(255 - summ where mask == 0)."""
    lib = lib or _lib.load()
    be = Backend(lib)
    gs, ss = tuple(int(v) for v in gt.shape), tuple(int(v) for v in summ.shape)
    if len(gs) not in (3, 4) or len(ss) not in (3, 4) or gs[:3] != ss[:3]:
        raise ValueError("pixel_sums: frames of shapes %s and %s" % (gs, ss))
    n, px = gs[0], gs[1] * gs[2]
    if masks is not None and tuple(int(v) for v in masks.shape) != gs[:3]:
        raise ValueError("pixel_sums: masks of shape %s, expected %s" % (tuple(masks.shape), gs[:3]))
    for name, x in (("gt", gt), ("summ", summ), ("masks", masks)):
        if x is not None and "uint8" not in str(x.dtype):
            raise ValueError("pixel_sums: %s must be uint8, got %s" % (name, x.dtype))
        if x is not None and not (x.is_contiguous() if hasattr(x, "is_contiguous") else x.flags["C_CONTIGUOUS"]):
            raise ValueError("pixel_sums: %s must be contiguous" % name)
    if n == 0:
        return np.zeros((0, 4), np.uint64)
    if px == 0:
        raise ValueError("pixel_sums: empty frames")
    out = be.empty((n, 4), np.int64)
    lib.check(lib.lm_kf_pixel_sums(_lib.ptr(gt), gs[3] if len(gs) == 4 else 1, _lib.ptr(summ), ss[3] if len(ss) == 4 else 1,
                                   _lib.ptr(masks), n, px, _lib.ptr(out), be.stream()))
    be.synchronize()
    return be.to_host(out).view(np.uint64).copy()
