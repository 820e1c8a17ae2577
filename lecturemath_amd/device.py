"""Thin Python layer over the C ABI: device buffers (torch on the GPU), contexts and frame streams.

PyTorch is plumbing only (device memory + streams); all arithmetic happens in liblecturemath_hip.so.
With the test-only emulated library (tests/hipemu) "device" memory is host memory and numpy arrays
stand in for torch tensors; the product never selects that path by itself (see _lib.load).
"""
import ctypes
import weakref

import numpy as np

from . import _lib


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


class FrameLabeler:
    """Batched scipy.ndimage.label + CC_AgeBoundaries on device frames (labeler.py:126, accessmath_lib.c:357-413)."""

    def __init__(self, width, height, max_batch=1, lib=None):
        self.lib = lib or _lib.load()
        self.be = Backend(self.lib)
        self.width, self.height, self.max_batch = width, height, max_batch
        self.ctx = self.lib.lm_ctx_create(width, height, max_batch)
        if not self.ctx:
            raise _lib.LecturemathError(_lib.LM_ERR_HIP, self.lib.last_error())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.lm_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

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
        self.lib.check(self.lib.lm_label_batch(self.ctx, _lib.ptr(binary), b, _lib.ptr(labels), self.be.stream()))
        counts = np.zeros(b, np.int32)
        self.lib.check(self.lib.lm_label_counts(self.ctx, counts.ctypes.data, self.be.stream()))
        return labels, counts

    def label_logits(self, logits, thr=128, invert=True, want_binary=False, want_labels=True):
        """fp32 logits [B,H,W] -> (labels or None, counts, {0,255} frames or None): threshold (+ the worker's inversion) and labelling in
        one pass over the logits (lm_label_batch_logits)."""
        b = logits.shape[0]
        assert tuple(logits.shape[1:]) == (self.height, self.width) and b <= self.max_batch
        labels = self.be.empty((b, self.height, self.width), np.int32) if want_labels else None
        binary = self.be.empty((b, self.height, self.width), np.uint8) if want_binary else None
        self.lib.check(self.lib.lm_label_batch_logits(self.ctx, _lib.ptr(logits), b, thr, 1 if invert else 0, _lib.ptr(binary), _lib.ptr(labels),
                                                      self.be.stream()))
        counts = np.zeros(b, np.int32)
        self.lib.check(self.lib.lm_label_counts(self.ctx, counts.ctypes.data, self.be.stream()))
        return labels, counts, binary

    def stats(self, counts):
        """CC_AgeBoundaries arrays of every frame of the last batch: list of int32 [5, n] (mins_y, maxs_y, mins_x, maxs_x, counts)."""
        self.lib.check(self.lib.lm_cc_stats_batch(self.ctx, self.be.stream()))
        out = []
        for f, n in enumerate(counts):
            a = np.zeros((5, int(n)), np.int32)
            rows = [a[i].ctypes.data if n else None for i in range(5)]
            self.lib.check(self.lib.lm_cc_stats_read(self.ctx, f, int(n), *rows, self.be.stream()))
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
    hb = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(n, 4))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([im.size for im in images])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(im, np.uint8).ravel() for im in images]))
    be = Backend(lib)
    cap = max(1024, 8 * n)
    while True:
        pairs = np.zeros((cap, 2), np.int32)
        found = np.zeros(1, np.int64)
        rc = lib.lm_image_pairs_overlap(hb.ctypes.data, flat.ctypes.data, off.ctypes.data, n, pairs.ctypes.data, cap, found.ctypes.data, be.stream())
        if rc == _lib.LM_ERR_CAPACITY and int(found[0]) > cap:
            cap = int(found[0])
            continue
        lib.check(rc)
        return [(int(a), int(b)) for a, b in pairs[:int(found[0])]]


class GroupImages:
    """Step 05 on the device: a table of images placed in the frame, held as bit rows (lm_kf_* in include/lecturemath_amd.h).

    from_grouping(grouping)   a view of the group images step 03 left on the device: item gimg_item_off[g] + k is segment image k
                              of group g (`item_first`); nothing is copied or expanded.  The Grouping is kept alive by the view and
                              closes the view when it is closed itself.
    from_host(boxes, images, width, height)   host uint8 images (conventions of image_pairs_overlap), uploaded and packed once.
    overlaps / render answer for all video segments in one call each."""

    created = 0          # instances made in this process (tests assert that the host route makes none)

    def __init__(self, lib, handle, width, height, shapes, owner=None, item_first=None):
        self.lib, self.be = lib, Backend(lib)
        self.handle, self.width, self.height = handle, int(width), int(height)
        self._shapes = shapes                   # [n_items][2] = h, w
        self._owner = owner
        self.item_first = item_first
        GroupImages.created += 1

    @classmethod
    def from_grouping(cls, grouping):
        if getattr(grouping, "handle", None) is None:
            raise ValueError("GroupImages.from_grouping: the Grouping is closed")
        lib = grouping.lib
        handle = lib.lm_kf_create_from_group(grouping.handle)
        if not handle:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, lib.last_error())
        off = grouping.array("gimg_item_off")
        b = grouping.array("bounds").reshape(-1, 4).astype(np.int64)
        per_group = np.stack([b[:, 3] - b[:, 2] + 1, b[:, 1] - b[:, 0] + 1], axis=1)
        self = cls(lib, handle, grouping.stream.width, grouping.stream.height, np.repeat(per_group, np.diff(off), axis=0), grouping, off[:-1].copy())
        grouping._views.add(self)
        return self

    @classmethod
    def from_host(cls, boxes, images, width, height, lib=None):
        lib = lib or _lib.load()
        n = len(images)
        hb = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(n, 4))
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([im.size for im in images])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(im, np.uint8).ravel() for im in images])) if n else np.zeros(1, np.uint8)
        handle = lib.lm_kf_create_from_images(hb.ctypes.data if n else None, flat.ctypes.data if n else None, off.ctypes.data if n else None, n,
                                              int(width), int(height), Backend(lib).stream())
        if not handle:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, lib.last_error())
        return cls(lib, handle, width, height, np.stack([hb[:, 3] - hb[:, 2] + 1, hb[:, 1] - hb[:, 0] + 1], axis=1).astype(np.int64))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lm_kf_destroy(self.handle)
            self.handle = None
        self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __reduce__(self):
        raise TypeError("GroupImages is a handle to device memory and cannot be pickled")

    def __len__(self):
        return int(self.lib.lm_kf_count(self._live()))

    def _live(self):
        if getattr(self, "handle", None) is None:
            raise ValueError("GroupImages: the handle is closed")
        return self.handle

    @staticmethod
    def _csr(lists):
        off = np.zeros(len(lists) + 1, np.int64)
        off[1:] = np.cumsum([len(lst) for lst in lists])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(lst, np.int32).reshape(-1) for lst in lists])) if off[-1] else np.zeros(1, np.int32)
        return off, flat

    def overlaps(self, item_lists):
        """item_lists: one list of items per video segment -> per segment the sorted pairs (i < j) of list positions whose images
        share an ink pixel."""
        handle = self._live()
        off, flat = self._csr(item_lists)
        cap = max(1024, 8 * int(off[-1]))
        while True:
            triples = np.zeros((cap, 3), np.int32)
            found = np.zeros(1, np.int64)
            rc = self.lib.lm_kf_overlaps(handle, off.ctypes.data, flat.ctypes.data, len(item_lists), triples.ctypes.data, cap, found.ctypes.data,
                                         self.be.stream())
            if rc == _lib.LM_ERR_CAPACITY and int(found[0]) > cap:
                cap = int(found[0])
                continue
            self.lib.check(rc)
            break
        out = [[] for _ in item_lists]
        for s, i, j in triples[:int(found[0])].tolist():
            out[s].append((i, j))
        return out

    def render(self, draw_lists, channels=3, out=None):
        """One keyframe per list: device uint8 [len(draw_lists), height, width, channels], 0 where a listed item has ink, else 255."""
        handle = self._live()
        off, flat = self._csr(draw_lists)
        shape = (len(draw_lists), self.height, self.width, int(channels))
        if out is None:
            out = self.be.empty(shape, np.uint8)
        elif tuple(out.shape) != shape:
            raise ValueError("GroupImages.render: out has shape %s, expected %s" % (tuple(out.shape), shape))
        self.lib.check(self.lib.lm_kf_render(handle, off.ctypes.data, flat.ctypes.data, len(draw_lists), int(channels), _lib.ptr(out), self.be.stream()))
        return out

    def image(self, item):
        """item as the reference's uint8 0 / 255 array (h, w)"""
        handle = self._live()
        if not 0 <= int(item) < len(self._shapes):
            raise IndexError("GroupImages.image: item %d of %d" % (item, len(self._shapes)))
        h, w = (int(v) for v in self._shapes[int(item)])
        out = np.zeros((h, w), np.uint8)
        self.lib.check(self.lib.lm_kf_image(handle, int(item), out.ctypes.data, h * w, self.be.stream()))
        return out

    def crowded_tiles(self):
        """(tile, keyframe) units of render() that took the crowded-tile path so far"""
        n = np.zeros(1, np.int64)
        self.lib.check(self.lib.lm_kf_crowded_tiles(self._live(), n.ctypes.data, self.be.stream()))
        return int(n[0])


class FrameHistory:
    """The frames of one binary stream as bit rows on the device (lm_hist_* in include/lecturemath_amd.h): for every pixel, in how
    many frames of a frame range was it ink, and when first?  Serves CCStabilityEstimator.compute_group_images_from_raw_binary and
    KeyframeExtractor.extract.  max_frames * height * ceil(width / 32) * 4 bytes of device memory, allocated here.

    A frame range [t0, t1] holds at most MAX_RANGE frames (the counters are 16 bit-sliced planes)."""

    MAX_RANGE = 65535
    UPLOAD_BYTES = 256 << 20    # host frames travel in batches of at most this size

    def __init__(self, width, height, max_frames, lib=None):
        self.lib = lib or _lib.load()
        self.be = Backend(self.lib)
        self.width, self.height, self.max_frames = int(width), int(height), int(max_frames)
        self.appends = 0            # append() calls that added frames (tests assert that a shared history uploads once)
        self.handle = self.lib.lm_hist_create(self.width, self.height, self.max_frames)
        if not self.handle:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, self.lib.last_error())

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

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lm_hist_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __reduce__(self):
        raise TypeError("FrameHistory is a handle to device memory and cannot be pickled")

    def _live(self):
        if getattr(self, "handle", None) is None:
            raise ValueError("FrameHistory: the handle is closed")
        return self.handle

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
        off, flat = GroupImages._csr(mask_lists)
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


ALIGN_MAX_WINDOW = 128      # LM_ALIGN_MAX_WINDOW of csrc/lm_align.hip


class TranslationAligner:
    """Aligner.computeTranslationAlignment (AccessMath/preprocessing/content/aligner.py:27-83) for many pairs of equally sized
    images at once (lm_align_* in include/lecturemath_amd.h): the images are packed to bit rows on the device once, the
    (2w + 1)^2 match counts of every pair come from one launch, and the reference's scores are its own divisions on those integers.

    set_images(images)             [n][H][W] or [n][H][W][C] uint8, a numpy array (host) or a torch device tensor (read in place)
    totals()                       ink pixels per image
    match_counts(pairs, w)         int64 [len(pairs)][2w + 1][2w + 1], [dy + w][dx + w]
    align(pairs, w, sort_by=0)     per pair the reference's tuple (f_score, recall, precision, disp_y, disp_x)"""

    def __init__(self, width, height, max_images=64, max_window=ALIGN_MAX_WINDOW, lib=None):
        self.lib = lib or _lib.load()
        self.be = Backend(self.lib)
        self.width, self.height = int(width), int(height)
        self.max_images, self.max_window = int(max_images), int(max_window)
        self.n_images = 0
        self._totals = None
        self._keep = None           # the device tensor an asynchronous set_images is reading
        self.handle = self.lib.lm_align_create(self.width, self.height, self.max_images, self.max_window, self.be.stream())
        if not self.handle:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, self.lib.last_error())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lm_align_destroy(self.handle)
            self.handle = None
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __reduce__(self):
        raise TypeError("TranslationAligner is a handle to device memory and cannot be pickled")

    def _live(self):
        if getattr(self, "handle", None) is None:
            raise ValueError("TranslationAligner: the handle is closed")
        return self.handle

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


CC_PAIR_MAX_RADIUS = 8      # LM_CCM_MAX_RADIUS of csrc/lm_ccmatch.hip


class _PairCounts:
    """counts() of a bit-row table (self._live() is its LmKeyframes handle, self.calls the lm_kf_pair_counts calls made)"""

    def counts(self, queries, radius, cap=None):
        handle = self._live()
        queries = list(queries)
        n_q, r = len(queries), int(radius)
        a_off, a_items = GroupImages._csr([q[0] for q in queries])
        b_off, b_items = GroupImages._csr([q[1] for q in queries])
        disp = np.ascontiguousarray(np.asarray([q[2] for q in queries], np.int64).reshape(n_q, 2))
        if n_q and np.abs(disp).max() > 0x7fffffff:
            raise ValueError("CCPairCounts.counts: displacement beyond int32")
        disp = np.ascontiguousarray(disp.astype(np.int32))
        side = 2 * max(r, 0) + 1
        cap = int(cap) if cap is not None else max(1024, 4 * int(a_off[-1] + b_off[-1]))
        for attempt in range(2):
            rows = np.zeros((cap, 3), np.int32)
            counts = np.zeros((cap, side, side), np.int32)
            found = np.zeros(1, np.int64)
            self.calls += 1
            rc = self.lib.lm_kf_pair_counts(handle, a_off.ctypes.data, a_items.ctypes.data, b_off.ctypes.data, b_items.ctypes.data,
                                            disp.ctypes.data if n_q else None, n_q, r, rows.ctypes.data, counts.ctypes.data, cap,
                                            found.ctypes.data, self.be.stream())
            if rc == _lib.LM_ERR_CAPACITY and int(found[0]) > cap and attempt == 0:
                cap = int(found[0])         # the retry gets the exact room
                continue
            self.lib.check(rc)
            break
        n = int(found[0])
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
        hb = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(n, 4))
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([im.size for im in images])
        flat = np.ascontiguousarray(np.concatenate([(im != 0).astype(np.uint8).ravel() for im in images])) if n else np.zeros(1, np.uint8)
        self.handle = self.lib.lm_kf_create_from_images(hb.ctypes.data if n else None, flat.ctypes.data if n else None,
                                                        off.ctypes.data if n else None, n, self.width, self.height, self.be.stream())
        if not self.handle:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, self.lib.last_error())
        self.n_items = n
        self.calls = 0              # lm_kf_pair_counts calls made (tests assert that cached results launch nothing)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lm_kf_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __reduce__(self):
        raise TypeError("CCPairCounts is a handle to device memory and cannot be pickled")

    def _live(self):
        if getattr(self, "handle", None) is None:
            raise ValueError("CCPairCounts: the handle is closed")
        return self.handle

    def item(self, k, i):
        return int(self.list_off[k]) + int(i)

    def items(self, k):
        """the items of list k (k = -1: the extra list)"""
        k = k % (len(self.list_off) - 1)
        return np.arange(self.list_off[k], self.list_off[k + 1], dtype=np.int32)


def _plain_cc(cls, state):
    cc = cls.__new__(cls)
    cc.__dict__.update(state)
    return cc


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

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lm_kf_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __reduce__(self):
        raise TypeError("KeyframeCCs is a handle to device memory and cannot be pickled")

    def __len__(self):
        return self.n_items

    @property
    def live(self):
        return getattr(self, "handle", None) is not None

    def _live(self):
        if getattr(self, "handle", None) is None:
            raise ValueError("KeyframeCCs: the handle is closed")
        return self.handle

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


class _LazyImageList:
    """cc_group_images[g]: len() and [k] backed by GroupImages.image, nothing held"""

    def __init__(self, gi, first, count):
        self._gi, self._first, self._count = gi, int(first), int(count)

    def __len__(self):
        return self._count

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(self._count))]
        k = int(k)
        if k < 0:
            k += self._count
        if not 0 <= k < self._count:
            raise IndexError("list index out of range")
        return self._gi.image(self._first + k)

    def __iter__(self):
        return (self[k] for k in range(self._count))


class LazyGroupImages:
    """Read-only stand-in for SpaceTimeStruct.cc_group_images ({group: [uint8 image per age segment]}) over a GroupImages view:
    an image is expanded when it is indexed.  Pickles as the plain dict of lists it stands for."""

    def __init__(self, gi, item_off, groups=None):
        self._gi = gi
        self._off = np.asarray(item_off, np.int64)          # [n_groups + 1]
        # the groups that are keys, ascending (compute_group_images_from_raw_binary skips empty groups); None: all of them
        self._groups = None if groups is None else [int(g) for g in groups]

    @property
    def device_images(self):
        """the GroupImages behind the images (its item_first names the first item of every group)"""
        return self._gi

    def __len__(self):
        return len(self._off) - 1 if self._groups is None else len(self._groups)

    def __iter__(self):
        return iter(self.keys())

    def __contains__(self, g):
        if not isinstance(g, (int, np.integer)) or not 0 <= g < len(self._off) - 1:
            return False
        return self._groups is None or int(g) in self._groups

    def keys(self):
        return range(len(self)) if self._groups is None else list(self._groups)

    def __getitem__(self, g):
        if g not in self:
            raise KeyError(g)
        return _LazyImageList(self._gi, self._off[g], self._off[g + 1] - self._off[g])

    def values(self):
        return (self[g] for g in self)

    def items(self):
        return ((g, self[g]) for g in self)

    def __reduce__(self):
        return (dict, ({g: list(self[g]) for g in self},))


def decode_crop(words, min_x, max_x, min_y, max_y):
    """bit-row crop (absolute 32-px column alignment) -> uint8 0/255 (h, w) like ConnectedComponent.img."""
    wx0 = min_x >> 5
    nw = (max_x >> 5) - wx0 + 1
    h = max_y - min_y + 1
    w = np.asarray(words, dtype="<u4").reshape(h, nw)
    bits = np.unpackbits(w.view(np.uint8).reshape(h, nw * 4), axis=1, bitorder="little")
    x0 = min_x - wx0 * 32
    return (bits[:, x0:x0 + (max_x - min_x + 1)] * 255).astype(np.uint8)


class FrameStream:
    """Device-resident CCStabilityEstimator.add_frame state (cc_stability_estimator.py:11-155)."""

    def __init__(self, width, height, max_frames, min_recall=0.85, min_precision=0.85, max_gap=85, min_pixels=20,
                 max_batch=16, max_ccs=None, max_crop_words=None, max_uniques=None, lib=None):
        self.labeler = FrameLabeler(width, height, max_batch, lib)
        self.lib, self.be = self.labeler.lib, self.labeler.be
        self.width, self.height = width, height
        self.min_pixels = min_pixels
        self._create_args = None
        px = width * height
        max_ccs = max_ccs or max_frames * max(px // 256, 64)
        max_crop_words = max_crop_words or max_frames * max(px // 4, 4096)
        max_uniques = max_uniques or max_ccs
        self.handle = self.lib.lm_stream_create(self.labeler.ctx, max_frames, max_ccs, max_crop_words, max_uniques,
                                                min_recall, min_precision, max_gap, min_pixels)
        if not self.handle:
            raise _lib.LecturemathError(_lib.LM_ERR_HIP, self.lib.last_error())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lm_stream_destroy(self.handle)
            self.handle = None
        self.labeler.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.lib.check(self.lib.lm_stream_reset(self.handle, self.be.stream()))

    def set_min_pixels(self, min_pixels):
        self.lib.check(self.lib.lm_stream_set_min_pixels(self.handle, int(min_pixels)))
        self.min_pixels = int(min_pixels)

    def push(self, binary, labels_out=None):
        """binary: device uint8 [n,H,W] (any n; split into batches internally). Asynchronous."""
        self.lib.check(self.lib.lm_stream_push(self.handle, _lib.ptr(binary), int(binary.shape[0]), _lib.ptr(labels_out),
                                               self.be.stream()))

    def push_records(self, binary, labels_out=None):
        """Per-frame half only (label, stats, records, crops): no temporal matching."""
        self.lib.check(self.lib.lm_stream_push_records(self.handle, _lib.ptr(binary), int(binary.shape[0]), _lib.ptr(labels_out),
                                                       self.be.stream()))

    def match(self, n_frames):
        """Sequential temporal matching over the next n_frames unmatched frames."""
        self.lib.check(self.lib.lm_stream_match(self.handle, int(n_frames), self.be.stream()))

    def pack(self, first_frame, n_frames):
        """Records + crops of frames [first_frame, first_frame + n_frames) as one flat device uint8 buffer (lm_stream_pack)."""
        nb = ctypes.c_int64(0)
        self.lib.check(self.lib.lm_stream_pack_size(self.handle, int(first_frame), int(n_frames), ctypes.addressof(nb), self.be.stream()))
        buf = self.be.empty((max(int(nb.value), 32),), np.uint8)
        self.lib.check(self.lib.lm_stream_pack(self.handle, int(first_frame), int(n_frames), _lib.ptr(buf), int(nb.value), self.be.stream()))
        return buf

    def append_packed(self, buf):
        """Append a packed block (device uint8 buffer from pack(), possibly received from another rank) behind the last frame."""
        self.lib.check(self.lib.lm_stream_append_packed(self.handle, _lib.ptr(buf), int(buf.shape[0]), self.be.stream()))

    def export_assign(self):
        """What the temporal matching added to the records, as one flat device uint8 buffer (lm_stream_export_assign): the hand-off of
        a matched stream to the rank that runs step 03, together with pack(0, n_frames)."""
        nb = ctypes.c_int64(0)
        self.lib.check(self.lib.lm_stream_assign_bytes(self.handle, ctypes.addressof(nb), self.be.stream()))
        buf = self.be.empty((int(nb.value),), np.uint8)
        self.lib.check(self.lib.lm_stream_export_assign(self.handle, _lib.ptr(buf), int(nb.value), self.be.stream()))
        return buf

    def import_assign(self, buf):
        self.lib.check(self.lib.lm_stream_import_assign(self.handle, _lib.ptr(buf), int(buf.shape[0]), self.be.stream()))

    def counters(self):
        k = np.zeros(7, np.int64)
        self.lib.check(self.lib.lm_stream_counters(self.handle, k.ctypes.data, self.be.stream()))
        return dict(n_frames=int(k[0]), n_cc=int(k[1]), n_crop_words=int(k[2]), n_unique=int(k[3]), n_active=int(k[4]),
                    tempo_count=int(k[5]))

    def read(self, with_crops=True):
        """Host copy of the stream: records, frame offsets, crops, active list."""
        k = self.counters()
        rec = np.zeros((max(k["n_cc"], 1), 8), np.int32)
        foff = np.zeros(k["n_frames"] + 1, np.int64)
        coff = np.zeros(max(k["n_cc"], 1), np.int64)
        crop = np.zeros(max(k["n_crop_words"], 1), np.uint32) if with_crops else None
        active = np.zeros(max(k["n_active"], 1), np.int32)
        self.lib.check(self.lib.lm_stream_read(self.handle, rec.ctypes.data, foff.ctypes.data, coff.ctypes.data,
                                               crop.ctypes.data if with_crops else None, active.ctypes.data, self.be.stream()))
        return dict(k, rec=rec[:k["n_cc"]], frame_off=foff, crop_off=coff[:k["n_cc"]], crop=crop, active=active[:k["n_active"]])

    def export_state(self):
        """Host snapshot (numpy) of everything needed to rebuild the stream: records, crops, active list."""
        r = self.read(with_crops=True)
        rec = r["rec"]
        nu = r["n_unique"]
        first = np.full(nu, -1, np.int64)
        last = np.zeros(nu, np.int32)
        if len(rec):
            order = np.arange(len(rec) - 1, -1, -1)
            first[rec[order, 7]] = order                  # smallest CC index wins (written last)
            np.maximum.at(last, rec[:, 7], rec[:, 6])
        act = r["active"].astype(np.int32)
        return {"width": self.width, "height": self.height, "rec": rec, "frame_off": r["frame_off"], "crop_off": r["crop_off"],
                "crop": r["crop"][:r["n_crop_words"]], "n_unique": nu, "tempo_count": r["tempo_count"], "active": act,
                "active_cc": first[act].astype(np.int32), "active_last": last[act].astype(np.int32), "uniq_first_cc": first}

    def import_state(self, st):
        """Inverse of export_state (capacities of this stream must suffice)."""
        rec = np.ascontiguousarray(st["rec"], np.int32)
        foff = np.ascontiguousarray(st["frame_off"], np.int64)
        coff = np.ascontiguousarray(st["crop_off"], np.int64)
        crop = np.ascontiguousarray(st["crop"], np.uint32)
        act = np.ascontiguousarray(st["active"], np.int32)
        acc = np.ascontiguousarray(st["active_cc"], np.int32)
        acl = np.ascontiguousarray(st["active_last"], np.int32)
        self.lib.check(self.lib.lm_stream_import(
            self.handle, rec.ctypes.data if len(rec) else None, foff.ctypes.data, coff.ctypes.data if len(rec) else None,
            crop.ctypes.data if len(crop) else (np.zeros(1, np.uint32).ctypes.data if len(rec) else None), len(foff) - 1, len(rec),
            len(crop), int(st["n_unique"]), int(st["tempo_count"]), act.ctypes.data if len(act) else None,
            acc.ctypes.data if len(act) else None, acl.ctypes.data if len(act) else None, len(act),
            int(st.get("n_matched", len(foff) - 1)), self.be.stream()))

    def result(self, with_crops=True):
        """Same plain-data view the oracle produces (reference attribute names):
        unique_recs, unique_crops, unique_cc_frames, cc_idx_per_frame, tempo_count, active."""
        r = self.read(with_crops)
        rec, foff = r["rec"], r["frame_off"]
        nu = r["n_unique"]
        first = np.full(nu, -1, np.int64)
        frames = [[] for _ in range(nu)]
        per_frame = []
        for f in range(r["n_frames"]):
            lst = []
            for c in range(foff[f], foff[f + 1]):
                u = int(rec[c, 7])
                if first[u] < 0:
                    first[u] = c
                frames[u].append((f, int(rec[c, 0]) + 1))
                lst.append((u, int(rec[c, 0])))
            per_frame.append(lst)
        urec = rec[first][:, [1, 2, 3, 4, 5]].copy() if nu else np.zeros((0, 5), np.int32)
        crops = []
        if with_crops:
            for u in range(nu):
                c = first[u]
                mnx, mxx, mny, mxy = (int(v) for v in rec[c, 1:5])
                nwords = ((mxx >> 5) - (mnx >> 5) + 1) * (mxy - mny + 1)
                o = int(r["crop_off"][c])
                crops.append(decode_crop(r["crop"][o:o + nwords], mnx, mxx, mny, mxy))
        return {"width": self.width, "height": self.height, "unique_recs": urec, "unique_crops": crops,
                "unique_cc_frames": frames, "cc_idx_per_frame": per_frame, "tempo_count": r["tempo_count"],
                "active": r["active"], "raw": r}


_G_DTYPES = {0: np.int32, 1: np.int64, 2: np.int32, 3: np.int32, 4: np.int32, 5: np.int32, 6: np.int32, 7: np.int32,
             8: np.int64, 9: np.int32, 10: np.float64, 11: np.float64, 12: np.int64, 13: np.int32, 14: np.int32, 15: np.int32,
             16: np.int32, 17: np.int64, 18: np.int32, 19: np.int32, 20: np.int64, 21: np.int32, 22: np.int64, 23: np.int32,
             24: np.int32, 25: np.int32, 26: np.int64, 27: np.int64, 28: np.int64, 29: np.float64, 30: np.int32, 31: np.int64,
             32: np.int64, 33: np.uint8, 34: np.int64}
_G_NAMES = ["uniq_cc", "ulist_off", "ulist_cc", "assign", "stable", "pair_a", "pair_b", "pair_match", "tov_off", "tov_other",
            "tov_recall", "tov_precision", "aov_off", "aov_other", "aov_matched", "aov_size_other", "aov_size_self", "grp_off",
            "grp_members", "gid", "ages_off", "ages", "gpf_off", "gpf", "conf_g1", "conf_g2", "conf_matched", "conf_unmatched",
            "conf_union", "conf_inter", "bounds", "gimg_off", "gimg_item_off", "gimg", "scalars"]


class Grouping:
    """Step 03 over a finished FrameStream (pre_ST3D_v3.0_03_cc_grouping.py:22-118)."""

    def __init__(self, stream, max_gap=85, min_times=3, t_window=5, min_recall=0.5, img_threshold=0.5, reconstruct=True):
        self.stream = stream
        self.lib, self.be = stream.lib, stream.be
        self.handle = self.lib.lm_group_run(stream.handle, max_gap, min_times, t_window, min_recall, img_threshold,
                                            1 if reconstruct else 0, self.be.stream())
        self._views = weakref.WeakSet()         # GroupImages views of this run's bit rows: closed before the run is destroyed
        if not self.handle:
            raise _lib.LecturemathError(_lib.LM_ERR_HIP, self.lib.last_error())

    def close(self):
        if getattr(self, "handle", None):
            for view in list(self._views):
                view.close()
            self.lib.lm_group_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def array(self, which):
        """Copy of one result array (see the id table in include/lecturemath_amd.h)."""
        if isinstance(which, str):
            which = _G_NAMES.index(which)
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self.lib.check(self.lib.lm_group_array(self.handle, which, ctypes.addressof(p), ctypes.addressof(n)))
        dt = np.dtype(_G_DTYPES[which])
        if n.value == 0:
            return np.zeros(0, dt)
        buf = (ctypes.c_char * (n.value * dt.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=dt).copy()

    def render(self, first, n, out=None):
        """frames_from_groups channel 0 for frames [first, first+n) -> device uint8 [n,H,W]."""
        out = out if out is not None else self.be.empty((n, self.stream.height, self.stream.width), np.uint8)
        self.lib.check(self.lib.lm_group_render(self.handle, first, n, _lib.ptr(out), self.be.stream()))
        return out

    def frame_sums(self, first, n):
        """Exact sums of the bytes of the reconstructed frames [first, first+n) -- frame_sums(render(first, n)) -- read off the
        cover counts of the render tiles: no frame is written (lm_group_frame_sums).  int64 numpy."""
        out = self.be.empty((max(int(n), 0),), np.int64)
        self.lib.check(self.lib.lm_group_frame_sums(self.handle, first, n, _lib.ptr(out) if n > 0 else None, self.be.stream()))
        return np.asarray(self.be.to_host(out), np.int64)

    def result(self, with_images=True, with_clean=True):
        """Plain-data view with the reference's names (same shape as oracle.grouping.run_step03)."""
        A = {name: self.array(i) for i, name in enumerate(_G_NAMES) if name != "gimg" or with_images}
        sc = A["scalars"]
        nu, ng, nf = int(sc[3]), int(sc[2]), int(sc[4])

        def csr(off, *cols):
            return [[tuple(c[j].item() for c in cols) if len(cols) > 1 else cols[0][j].item()
                     for j in range(off[i], off[i + 1])] for i in range(len(off) - 1)]

        out = {
            "n_split": int(sc[0]), "total_intersections": int(sc[1]),
            "stable_idxs": [int(v) for v in A["stable"]],
            "time_overlapping_cc": csr(A["tov_off"], A["tov_other"], A["tov_recall"], A["tov_precision"]),
            "all_overlapping_cc": csr(A["aov_off"], A["aov_other"], A["aov_matched"], A["aov_size_other"], A["aov_size_self"]),
            "cc_groups": csr(A["grp_off"], A["grp_members"]),
            "group_idx_per_cc": {u: int(g) for u, g in enumerate(A["gid"]) if g >= 0},
            "group_ages": {g: lst for g, lst in enumerate(csr(A["ages_off"], A["ages"]))},
            "groups_per_frame": csr(A["gpf_off"], A["gpf"]),
            "group_boundaries": {g: tuple(int(v) for v in A["bounds"][4 * g:4 * g + 4]) for g in range(ng)},
            "arrays": A,
        }
        conf = {g: {} for g in range(ng)}
        # lm_group_run emits the rows grouped by conf_g1, each group in the reference's first-insertion order: the inner dicts keep it
        for i in range(len(A["conf_g1"])):
            conf[int(A["conf_g1"][i])][int(A["conf_g2"][i])] = {
                "matched": int(A["conf_matched"][i]), "unmatched": int(A["conf_unmatched"][i]),
                "area_union": int(A["conf_union"][i]), "area_intersection": float(A["conf_inter"][i])}
        out["conflicts"] = conf
        if with_images:
            imgs = {}
            for g in range(ng):
                x0, x1, y0, y1 = out["group_boundaries"][g]
                w, h = x1 - x0 + 1, y1 - y0 + 1
                lst = []
                for it in range(A["gimg_item_off"][g], A["gimg_item_off"][g + 1]):
                    o = A["gimg_off"][it]
                    lst.append(A["gimg"][o:o + w * h].reshape(h, w))
                imgs[g] = lst
            out["group_images"] = imgs
        if with_clean and nf:
            out["clean_binary"] = list(self.be.to_host(self.render(0, nf)))
        # unique_cc_frames / cc_idx_per_frame after the split
        rec = self.stream.read(with_crops=False)["rec"]
        out["unique_cc_frames"] = [[(int(rec[c, 6]), int(rec[c, 0]) + 1) for c in A["ulist_cc"][A["ulist_off"][u]:A["ulist_off"][u + 1]]]
                                   for u in range(nu)]
        foff = self.stream.read(with_crops=False)["frame_off"]
        out["cc_idx_per_frame"] = [[(int(A["assign"][c]), int(rec[c, 0])) for c in range(foff[f], foff[f + 1])] for f in range(nf)]
        return out
