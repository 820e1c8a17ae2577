"""Tables of placed bit-row images (lm_kf_*): the group images of step 03 and their lazy dict stand-in, and bit-row decoding."""
import numpy as np

from .. import _lib
from ._base import Backend, DeviceHandle, call_with_room, csr, flatten_images


class GroupImages(DeviceHandle):
    """Step 05 on the device: a table of images placed in the frame, held as bit rows (lm_kf_* in include/lecturemath_amd.h).

    from_grouping(grouping)   a view of the group images step 03 left on the device: item gimg_item_off[g] + k is segment image k
                              of group g (`item_first`); nothing is copied or expanded.  The Grouping is kept alive by the view and
                              closes the view when it is closed itself.
    from_host(boxes, images, width, height)   host uint8 images (conventions of image_pairs_overlap), uploaded and packed once.
    overlaps / render answer for all video segments in one call each."""

    DESTROY = "lm_kf_destroy"
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
        hb, off, flat = flatten_images(boxes, images)
        handle = lib.lm_kf_create_from_images(hb.ctypes.data if n else None, flat.ctypes.data if n else None, off.ctypes.data if n else None, n,
                                              int(width), int(height), Backend(lib).stream())
        if not handle:
            raise _lib.LecturemathError(_lib.LM_ERR_ARG, lib.last_error())
        return cls(lib, handle, width, height, np.stack([hb[:, 3] - hb[:, 2] + 1, hb[:, 1] - hb[:, 0] + 1], axis=1).astype(np.int64))

    def _destroy(self):
        super()._destroy()
        self._owner = None

    def __len__(self):
        return int(self.lib.lm_kf_count(self._live()))

    _csr = staticmethod(csr)

    def overlaps(self, item_lists):
        """item_lists: one list of items per video segment -> per segment the sorted pairs (i < j) of list positions whose images
        share an ink pixel."""
        handle = self._live()
        off, flat = csr(item_lists)

        def call(cap):
            triples = np.zeros((cap, 3), np.int32)
            found = np.zeros(1, np.int64)
            rc = self.lib.lm_kf_overlaps(handle, off.ctypes.data, flat.ctypes.data, len(item_lists), triples.ctypes.data, cap, found.ctypes.data,
                                         self.be.stream())
            return rc, int(found[0]), triples

        found, triples = call_with_room(self.lib, max(1024, 8 * int(off[-1])), call)
        out = [[] for _ in item_lists]
        for s, i, j in triples[:found].tolist():
            out[s].append((i, j))
        return out

    def render(self, draw_lists, channels=3, out=None):
        """One keyframe per list: device uint8 [len(draw_lists), height, width, channels], 0 where a listed item has ink, else 255."""
        handle = self._live()
        off, flat = csr(draw_lists)
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
