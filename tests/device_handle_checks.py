"""Checks of the lecturemath_amd.device package shared by the CPU tests (emulated library) and the GPU tests: the lifecycle every
handle class takes from device.DeviceHandle (close, pickling, use after close, who closes whom), the counters the other tests
rely on, the names the package exports, and the host-side helpers against the expressions they replaced.

The lifecycle does not depend on the frame shape, so the frames are the smallest that still hold two glyph-sized blobs: three
frames of 24 x 48 with the same two rectangles."""
import io
import pickle

import numpy as np
import pytest

import dropin_checks

W, H, N = 48, 24, 3
BOXES = [(4, 12, 3, 10), (25, 40, 12, 20)]          # min_x, max_x, min_y, max_y: 72 and 144 pixels


def frames():
    """uint8 [N][H][W], 255 = ink"""
    f = np.zeros((N, H, W), np.uint8)
    for x0, x1, y0, y1 in BOXES:
        f[:, y0:y1 + 1, x0:x1 + 1] = 255
    return f


def box_images():
    return [np.full((y1 - y0 + 1, x1 - x0 + 1), 255, np.uint8) for x0, x1, y0, y1 in BOXES]


def pushed_stream(device, lib):
    fs = device.FrameStream(W, H, N, 0.85, 0.85, 2, 20, max_batch=N, lib=lib)
    fs.push(fs.be.from_host(frames()))
    return fs


def assert_closes_twice(obj, name="handle"):
    obj.close()
    assert getattr(obj, name) is None
    obj.close()
    assert getattr(obj, name) is None


def assert_not_picklable(obj):
    with pytest.raises(TypeError, match="%s is a handle to device memory and cannot be pickled" % type(obj).__name__):
        pickle.dumps(obj)


def assert_closed(obj, call):
    with pytest.raises(ValueError, match="%s: the handle is closed" % type(obj).__name__):
        call()


# ---- 1. the eight handle classes -------------------------------------------------------------------------------------------------------
def check_labeler(lib):
    from lecturemath_amd import device
    lab = device.FrameLabeler(W, H, 2, lib)
    assert lab.ctx and lab.ctx == lab.handle
    assert_not_picklable(lab)
    assert_closes_twice(lab, "ctx")
    assert lab.handle is None


def check_stream_and_grouping(lib):
    from lecturemath_amd import device
    fs = pushed_stream(device, lib)
    try:
        assert fs.counters()["n_frames"] == N and fs.counters()["n_unique"] == len(BOXES)
        assert_not_picklable(fs)
        gr = device.Grouping(fs, max_gap=2, min_times=2, t_window=1)
        try:
            assert int(gr.array("scalars")[2]) >= 1, "no group"
            assert_not_picklable(gr)
            before = device.GroupImages.created
            views = [device.GroupImages.from_grouping(gr), device.GroupImages.from_grouping(gr)]
            assert device.GroupImages.created == before + 2
            assert all(len(v) == len(views[0]) >= 1 and v._owner is gr for v in views)
            views[0].close()                                # a view closed by hand stays closed, the other is closed by the run
        finally:
            gr.close()
        assert_closes_twice(gr)
        for v in views:
            assert v.handle is None and v._owner is None
            assert_closed(v, lambda: len(v))
        with pytest.raises(ValueError, match="closed"):
            device.GroupImages.from_grouping(gr)
    finally:
        fs.close()
    assert_closes_twice(fs)
    assert fs.labeler.ctx is None, "closing the stream closes its labeler"


def check_group_images(lib):
    from lecturemath_amd import device
    before = device.GroupImages.created
    gi = device.GroupImages.from_host(BOXES, box_images(), W, H, lib)
    assert device.GroupImages.created == before + 1
    assert len(gi) == 2 and gi.overlaps([[0, 1]]) == [[]] and (gi.image(1) == 255).all()
    assert_not_picklable(gi)
    assert_closes_twice(gi)
    assert_closed(gi, lambda: len(gi))
    assert_closed(gi, lambda: gi.overlaps([[0, 1]]))
    empty = device.GroupImages.from_host([], [], W, H, lib)
    assert len(empty) == 0
    assert_closes_twice(empty)


def check_history(lib):
    from lecturemath_amd import device
    hist = device.FrameHistory.from_frames(frames(), lib)
    assert hist.appends == 1 and len(hist) == N
    assert hist.ink_counts().tolist() == [72 + 144] * N
    same, owned = device.as_frame_history(hist, lib)
    assert same is hist and not owned and hist.appends == 1
    assert_not_picklable(hist)
    assert_closes_twice(hist)
    assert_closed(hist, lambda: len(hist))
    assert_closed(hist, lambda: hist.append(frames()))
    assert hist.appends == 1


def check_aligner(lib):
    from lecturemath_amd import device
    al = device.TranslationAligner(W, H, max_images=2, max_window=2, lib=lib)
    al.set_images(frames()[:2])
    assert al.totals().tolist() == [216, 216]
    assert al.align([(0, 1)], 2) == [(1.0, 1.0, 1.0, 0, 0)]
    assert_not_picklable(al)
    assert_closes_twice(al)
    assert al._keep is None
    assert_closed(al, lambda: al.set_images(frames()[:2]))
    assert_closed(al, lambda: al.match_counts([(0, 1)], 2))


def check_pair_counts(lib):
    from lecturemath_amd import device
    ccs = list(zip(BOXES, box_images()))
    created = device.CCPairCounts.created
    table = device.CCPairCounts([ccs], W, H, lib=lib)
    assert device.CCPairCounts.created == created + 1 and table.calls == 0 and table.n_items == 2
    query = [([0, 1], [0, 1], (0, 0))]
    rows, counts = table.counts(query, 0)
    assert table.calls == 1
    assert rows.tolist() == [[0, 0, 0], [0, 1, 1]] and counts.reshape(-1).tolist() == [72, 144]
    rows2, counts2 = table.counts(query, 0, cap=1)          # room for one row of two: one retry with the exact room
    assert table.calls == 3
    assert (rows2 == rows).all() and (counts2 == counts).all()
    assert_not_picklable(table)
    assert_closes_twice(table)
    assert_closed(table, lambda: table.counts(query, 0))
    assert table.calls == 3


def check_keyframe_ccs(lib):
    from lecturemath_amd import device
    table = device.KeyframeCCs.from_frames(255 - frames(), lib=lib)
    assert table in device.KeyframeCCs._tables and table.live and table.calls == 0
    assert len(table) == N * len(BOXES) and table.frame_off.tolist() == [0, 2, 4, 6]
    assert [table.box(i) for i in (0, 1)] == BOXES
    table.counts([([0], [2], (0, 0))], 0)
    assert table.calls == 1
    assert_not_picklable(table)
    assert_closes_twice(table)
    assert not table.live
    assert_closed(table, lambda: table.image(0))
    assert_closed(table, lambda: table.counts([([0], [2], (0, 0))], 0))
    assert table.calls == 1


# ---- 2. the package's surface ----------------------------------------------------------------------------------------------------------
PUBLIC_NAMES = ["Backend", "FrameLabeler", "frame_sums", "ConflictSignal", "image_pairs_overlap", "GroupImages", "FrameHistory",
                "as_frame_history", "ALIGN_MAX_WINDOW", "TranslationAligner", "CC_PAIR_MAX_RADIUS", "CCPairCounts", "device_cc_class",
                "KeyframeCCs", "PairTableView", "pixel_sums", "LazyGroupImages", "decode_crop", "FrameStream", "Grouping",
                "_G_NAMES", "_G_DTYPES", "_plain_cc"]


def check_public_names():
    from lecturemath_amd import device
    missing = [name for name in PUBLIC_NAMES if not hasattr(device, name)]
    assert not missing, missing
    assert device.ALIGN_MAX_WINDOW == 128 and device.CC_PAIR_MAX_RADIUS == 8
    assert len(device._G_NAMES) == len(device._G_DTYPES) == 35 and device._G_NAMES.index("gimg") == 33


def check_device_cc_pickles_plain(lib):
    dropin_checks.use_library(lib)
    from AM_CommonTools.data.connected_component import ConnectedComponent
    from lecturemath_amd import device
    assert pickle.Unpickler(io.BytesIO(b"")).find_class("lecturemath_amd.device", "_plain_cc") is device._plain_cc
    table = device.KeyframeCCs.from_frames(255 - frames()[:1], lib=lib)
    try:
        cc = table.ccs(0)[1]
        assert type(cc) is device.device_cc_class() and cc.table is table
        blob = pickle.dumps(cc, protocol=2)
        assert b"lecturemath_amd.device\n_plain_cc" in blob, "the pickle names another home of _plain_cc"
        back = pickle.loads(blob)
        assert type(back) is ConnectedComponent
        assert back.img.dtype == cc.img.dtype and back.img.shape == (9, 16) and (back.img == cc.img).all()
        assert (back.min_x, back.max_x, back.min_y, back.max_y, back.size) == BOXES[1] + (144,)
        assert not hasattr(back, "table")
    finally:
        table.close()


# ---- 3. the host-side helpers against the expressions they replaced ---------------------------------------------------------------------
def old_csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(lst) for lst in lists])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(lst, np.int32).reshape(-1) for lst in lists])) if off[-1] else np.zeros(1, np.int32)
    return off, flat


def old_flatten(boxes, images, as_bool):
    n = len(images)
    hb = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(n, 4))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([im.size for im in images])
    if as_bool:
        flat = np.ascontiguousarray(np.concatenate([(im != 0).astype(np.uint8).ravel() for im in images])) if n else np.zeros(1, np.uint8)
    else:
        flat = np.ascontiguousarray(np.concatenate([np.asarray(im, np.uint8).ravel() for im in images])) if n else np.zeros(1, np.uint8)
    return hb, off, flat


def assert_same_arrays(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all() and a.flags["C_CONTIGUOUS"]


def check_helpers():
    from lecturemath_amd import device
    from lecturemath_amd.device._base import csr, flatten_images
    for lists in ([], [[]], [[], []], [[3]], [[1, 2], [], np.arange(5, dtype=np.int64), (7,)]):
        assert_same_arrays(csr(lists), old_csr(lists))
    assert device.GroupImages._csr is csr
    rng = np.random.default_rng(11)
    images = [rng.integers(0, 3, (3, 5)).astype(np.uint8) * 100, np.array([[0, 255]], np.uint8), (rng.random((4, 1)) < 0.5)]
    boxes = [(0, 4, 0, 2), [7, 8, 1, 1], np.array([2, 2, 3, 6])]
    for as_bool in (False, True):
        assert_same_arrays(flatten_images([], [], as_bool), old_flatten([], [], as_bool))
        assert_same_arrays(flatten_images(np.zeros((0, 4)), [], as_bool), old_flatten(np.zeros((0, 4)), [], as_bool))
        for k in (1, 3):
            assert_same_arrays(flatten_images(boxes[:k], images[:k], as_bool), old_flatten(boxes[:k], images[:k], as_bool))
    assert flatten_images(boxes, images, True)[2].max() == 1 and flatten_images(boxes, images)[2].max() == 255
