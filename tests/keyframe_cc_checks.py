"""Checks of the keyframe CC table (lm_kf_create_from_frames / lm_kf_cc_records / lm_kf_pixel_sums, device.KeyframeCCs,
lecturemath_amd.keyframes, the overlay Evaluator's view route) shared by the CPU tests (emulated library) and the GPU tests.
Everything is compared exactly.  Comparators: the overlay Labeler route on the same plane (Labeler.extractSpatioTemporalContent(255 -
channel 0, zeros, False), verified against the oracle elsewhere), hand-computed expectations for the drawn shapes, numpy for counts and
sums, and what the UNMODIFIED reference returned for the G24 keyframes (tests/golden/make_golden_keyframe_ccs.py)."""
import contextlib
import copy
import io
import json
import os
import pickle
import types

import numpy as np

import dropin_checks
import evaluation_checks as ec
import lm_checks

PAPER = 255


def modules(lib):
    dropin_checks.use_library(lib)
    from lecturemath_amd import device, keyframes
    return device, keyframes


def labeler():
    from AccessMath.preprocessing.content.labeler import Labeler
    return Labeler


def host_ccs(plane, min_pixels=1):
    """the parent route: the overlay Labeler on 255 - plane (filter_small=False), then the size filter (ids are not renumbered)"""
    h, w = plane.shape
    ccs = labeler().extractSpatioTemporalContent(255 - plane, np.zeros((h, w), np.float32), False)
    return [cc for cc in ccs if cc.size >= min_pixels]


def assert_same_cc(got, want, what):
    for name in ("cc_id", "min_x", "max_x", "min_y", "max_y", "size", "start_time", "end_time"):
        a, b = getattr(got, name), getattr(want, name)
        assert type(a) is type(b) and a == b, (what, name, a, b, type(a), type(b))
    assert got.img.dtype == want.img.dtype and got.img.shape == want.img.shape and (got.img == want.img).all(), (what, "img")
    assert got.strID() == want.strID()


def compare_with_labeler(lib, frames, masks=None, min_pixels=1, max_batch=8):
    """the table of `frames` ([n][H][W] or [n][H][W][C]) against the Labeler route, frame by frame; returns the CC counts"""
    device, _ = modules(lib)
    frames = np.asarray(frames)
    planes = frames if frames.ndim == 3 else frames[..., 0]
    n, h, w = planes.shape
    table = device.KeyframeCCs.from_frames(frames, masks=masks, min_pixels=min_pixels, max_batch=max_batch, lib=lib)
    try:
        assert table.frame_off.dtype == np.int64 and table.frame_off.shape == (n + 1,) and table.frame_off[0] == 0
        assert table.records.dtype == np.int32 and table.records.shape == (int(table.frame_off[-1]), 6)
        assert len(table) == int(table.frame_off[-1]) + (n if masks is not None else 0)
        counts = []
        for k in range(n):
            want = host_ccs(np.ascontiguousarray(planes[k]), min_pixels)
            got = table.ccs(k)
            assert len(got) == len(want) == len(table.items(k)), (k, len(got), len(want))
            for j, (a, b) in enumerate(zip(got, want)):
                assert a.item == int(table.items(k)[j]) and a.table is table
                assert_same_cc(a, b, (k, j))
                assert (table.records[a.item] == [b.cc_id, b.min_x, b.max_x, b.min_y, b.max_y, b.size]).all()
            counts.append(len(got))
            if masks is not None:
                assert (table.image(table.mask_item(k)) == (np.asarray(masks[k]) != 0) * np.uint8(255)).all(), k
        return counts
    finally:
        table.close()


def paper(n, h, w):
    return np.full((n, h, w), PAPER, np.uint8)


# ---- 1. shapes ----------------------------------------------------------------------------------------------------------------------
def word_arithmetic_frames():
    """frames of 40 x 97 and the boxes drawn on them as solid rectangles, (frame, min_x, max_x, min_y, max_y): left edges with
    min_x & 31 = 0, 1, 31; widths 1, 2 (columns 31-32: two crop words, one item word), 32, 33, 64; the frame's right edge (96)"""
    boxes = [(0, 0, 0, 0, 2), (0, 31, 32, 0, 1), (0, 33, 33, 4, 9), (0, 64, 95, 0, 0), (0, 1, 33, 12, 13), (0, 31, 94, 16, 18),
             (0, 96, 96, 3, 30), (0, 32, 63, 22, 22), (0, 31, 63, 25, 27), (0, 0, 63, 33, 33), (0, 1, 64, 36, 37), (0, 66, 96, 39, 39),
             (1, 0, 96, 0, 39)]
    frames = paper(2, 40, 97)
    for f, x0, x1, y0, y1 in boxes:
        frames[f, y0:y1 + 1, x0:x1 + 1] = 0
    return frames, boxes


def check_word_arithmetic(lib):
    device, _ = modules(lib)
    frames, boxes = word_arithmetic_frames()
    table = device.KeyframeCCs.from_frames(frames, lib=lib)
    try:
        want = sorted(boxes, key=lambda b: (b[0], b[3], b[1]))              # scipy's order: first pixel in raster order
        assert len(table) == len(want)
        assert table.frame_off.tolist() == [0, len(boxes) - 1, len(boxes)]
        for item, (f, x0, x1, y0, y1) in enumerate(want):
            rec = table.records[item].tolist()
            assert rec[1:] == [x0, x1, y0, y1, (x1 - x0 + 1) * (y1 - y0 + 1)], (item, rec)
            img = table.image(item)
            assert img.shape == (y1 - y0 + 1, x1 - x0 + 1) and (img == 255).all(), item
        assert [r[0] for r in table.records.tolist()] == list(range(len(boxes) - 1)) + [0]
    finally:
        table.close()
    assert compare_with_labeler(lib, frames) == [len(boxes) - 1, 1]
    # the same shapes with a hole punched into each (images that are not all ink), three channels, a frame 33 x 64 and tiny frames
    holes = frames.copy()
    holes[0, ::3, ::5] = PAPER
    compare_with_labeler(lib, np.repeat(holes[..., None], 3, axis=3))
    rng = np.random.default_rng(7)
    for h, w in ((33, 64), (1, 1), (1, 65)):
        f = np.where(rng.random((3, h, w)) < 0.4, 0, PAPER).astype(np.uint8)
        f[0] = 0
        assert compare_with_labeler(lib, f)[0] == 1


def check_ring_and_comb(lib):
    device, _ = modules(lib)
    frames = paper(2, 45, 70)
    frames[0, 5:16, 29:40] = 0              # ring (columns 29 .. 39 straddle a word boundary) around a dot
    frames[0, 6:15, 30:39] = PAPER
    frames[0, 10, 34] = 0
    frames[1, 3:40, 2:68:2] = 0             # comb: 33 teeth joined at the last row only
    frames[1, 40, 2:67] = 0
    table = device.KeyframeCCs.from_frames(frames, lib=lib)
    try:
        assert table.frame_off.tolist() == [0, 2, 3]
        ring, dot, comb = table.image(0), table.image(1), table.image(2)
        assert table.records[0].tolist() == [0, 29, 39, 5, 15, 121 - 81] and table.records[1].tolist() == [1, 34, 34, 10, 10, 1]
        assert ring.shape == (11, 11) and ring[5, 5] == 0 and np.count_nonzero(ring) == 40 and dot.shape == (1, 1) and dot[0, 0] == 255
        # neither contains the other: no shared ink at displacement 0
        rows, counts = table.counts([([0], [1], (0, 0))], 0)
        assert rows.tolist() == [[0, 0, 0]] and counts.reshape(-1).tolist() == [0]
        assert table.records[2].tolist() == [0, 2, 66, 3, 40, 33 * 37 + 65]
        assert (comb[:-1, 1::2] == 0).all() and (comb[:-1, 0::2] == 255).all() and (comb[-1] == 255).all()
    finally:
        table.close()
    compare_with_labeler(lib, frames)


def check_non_binary_empty_full(lib):
    device, _ = modules(lib)
    frames = paper(4, 33, 64)
    frames[0, 4, 7] = 17                    # any byte but 255 is ink
    frames[0, 4, 8] = 254
    frames[0, 9, 9] = 1
    frames[2] = 0                           # all ink; frames 1 and 3 are empty
    frames[2, 5, 5] = 128
    table = device.KeyframeCCs.from_frames(frames, lib=lib)
    try:
        assert table.frame_off.tolist() == [0, 2, 2, 3, 3] and len(table) == 3
        assert table.records.tolist() == [[0, 7, 8, 4, 4, 2], [1, 9, 9, 9, 9, 1], [0, 0, 63, 0, 32, 33 * 64]]
        assert len(table.items(1)) == 0 and table.ccs(3) == [] and (table.image(2) == 255).all()
    finally:
        table.close()
    compare_with_labeler(lib, frames)
    empty = device.KeyframeCCs.from_frames(np.zeros((0, 33, 64), np.uint8), lib=lib)
    try:
        assert len(empty) == 0 and empty.frame_off.tolist() == [0] and empty.records.shape == (0, 6)
    finally:
        empty.close()


def check_batching_and_min_pixels(lib):
    rng = np.random.default_rng(11)
    frames = np.where(rng.random((5, 45, 70)) < 0.3, 0, PAPER).astype(np.uint8)
    frames[3] = PAPER                       # a batch that ends with an empty frame and one that starts with it
    masks = rng.random((5, 45, 70)) < 0.4
    all_ccs = compare_with_labeler(lib, frames, masks=masks, max_batch=2)
    assert all_ccs[3] == 0 and min(all_ccs[:3]) > 300
    kept = compare_with_labeler(lib, frames, min_pixels=3, max_batch=2)
    assert all(0 < k < a for k, a in zip(kept[:3], all_ccs[:3]))
    device, _ = modules(lib)
    table = device.KeyframeCCs.from_frames(frames, min_pixels=3, max_batch=2, lib=lib)
    try:
        ids = table.records[table.items(0), 0]
        assert (np.diff(ids) > 0).all() and ids[-1] >= len(ids) and (table.records[:, 5] >= 3).all()      # ids keep their gaps
    finally:
        table.close()


def check_clean_tails(lib):
    """an item against an all-ink full-frame mask: its size at every displacement that keeps it inside the frame"""
    device, _ = modules(lib)
    frames, boxes = word_arithmetic_frames()
    rng = np.random.default_rng(3)
    noise = np.where(rng.random((1, 40, 97)) < 0.3, 0, PAPER).astype(np.uint8)
    frames = np.concatenate([frames, noise])
    table = device.KeyframeCCs.from_frames(frames, masks=np.ones(frames.shape, np.uint8), lib=lib)
    try:
        for k in range(len(frames)):
            items = table.items(k)
            for radius in (0, 2):
                rows, counts = table.counts([([table.mask_item(k)], items, (0, 0))], radius)
                assert rows[:, 2].tolist() == list(range(len(items)))
                for j, c in zip(rows[:, 2].tolist(), counts):
                    x0, x1, y0, y1, size = table.records[items[j], 1:].tolist()
                    assert c[radius][radius] == size, (k, j)
                    if x0 >= radius and y0 >= radius and x1 + radius < 97 and y1 + radius < 40:
                        assert (c == size).all(), (k, j, radius)
                    assert c.max() == size
    finally:
        table.close()


# ---- 2. the reference's values ---------------------------------------------------------------------------------------------------------
_cache = {}


def g24():
    if "g" not in _cache:
        g = np.load(os.path.join(lm_checks.GOLD, "g24_keyframe_ccs.npz"))
        _cache["g"] = ({k: g[k] for k in g.files}, json.loads(bytes(g["recorded"]).decode()))
    return _cache["g"]


def g24_inputs():
    """frames [6][H][W] (ground truth, then binarized), masks bool [6][H][W] (none on the binarized side)"""
    g, _ = g24()
    h, w = (int(v) for v in g["shape"])
    masks = np.unpackbits(g["gt_masks"], axis=2)[:, :, :w].astype(bool)
    return np.concatenate([g["gt_planes"], g["summ_planes"]]), np.concatenate([masks, np.zeros_like(masks)])


def check_fixture_not_vacuous():
    g, rec = g24()
    per = np.diff(g["gt_cc_off"]).tolist() + np.diff(g["summ_cc_off"]).tolist()
    assert min(per) >= 30 and max(per) >= 399
    assert int(np.count_nonzero((g["gt_planes"] != 0) & (g["gt_planes"] != 255))) >= 20            # non-binary bytes
    rec_all = np.concatenate([g["gt_cc_rec"], g["summ_cc_rec"]])
    assert int(np.count_nonzero(rec_all[:, 1] // 32 != rec_all[:, 2] // 32)) >= 10                  # boxes across a word boundary
    assert int(np.count_nonzero(rec_all[:, 2] == 69)) >= 5 and int(np.count_nonzero(rec_all[:, 5] == 1)) >= 300
    metrics = ec.decode(rec["metrics"])
    assert len(rec["range_names"]) >= 4 and "all" in metrics
    pixel = ec.decode(rec["pixel"])
    assert 0.05 < pixel["recall"] < 0.95 and pixel["board_precision"] > pixel["precision"]
    assert np.isnan(ec.decode(rec["pixel_empty"])["precision"]) and ec.decode(rec["pixel_covered"])["board_precision"] == 1.0
    assert ec.decode(rec["pixel_disjoint"])["fmeasure"] == 0.0 and ec.decode(rec["pixel_disjoint"])["precision"] == 0.0


def check_g24_ccs(lib):
    device, _ = modules(lib)
    g, _ = g24()
    frames, masks = g24_inputs()
    table = device.KeyframeCCs.from_frames(np.repeat(frames[..., None], 3, axis=3), masks=masks, max_batch=4, lib=lib)
    try:
        want_rec = np.concatenate([g["gt_cc_rec"], g["summ_cc_rec"]])
        want_off = np.concatenate([g["gt_cc_off"], g["summ_cc_off"][1:] + g["gt_cc_off"][-1]])
        assert (table.frame_off == want_off).all() and (table.records == want_rec).all()
        item = 0
        for prefix in ("gt", "summ"):
            flat, off = np.unpackbits(g[prefix + "_cc_bits"]), g[prefix + "_cc_img_off"]
            for k, r in enumerate(g[prefix + "_cc_rec"].tolist()):
                img = flat[off[k]:off[k + 1]].reshape(r[4] - r[3] + 1, r[2] - r[1] + 1) * np.uint8(255)
                assert (table.image(item) == img).all(), (prefix, k)
                item += 1
    finally:
        table.close()


def device_sets(lib):
    """(gt keyframes, binarized keyframes) over ONE table"""
    _, keyframes = modules(lib)
    frames, masks = g24_inputs()
    kfs = keyframes.keyframes_from_frames(np.repeat(frames[..., None], 3, axis=3), masks=masks, max_batch=4, lib=lib)
    for k, kf in enumerate(kfs):
        kf.idx = k % 3
    return kfs[:3], kfs[3:]


def host_sets(lib):
    """the parent route on the same inputs: host keyframes whose CCs come from the overlay Labeler (made once, not modified)"""
    modules(lib)
    if "host" in _cache:
        return _cache["host"]
    frames, masks = g24_inputs()
    out = []
    for k in range(len(frames)):
        kf = types.SimpleNamespace(idx=k % 3, binary_image=np.repeat(frames[k][:, :, None], 3, axis=2), raw_image=None,
                                   object_mask=masks[k].copy(), binary_cc=host_ccs(frames[k]))
        kf.check_cc_overlaps_background = types.MethodType(ec.overlaps_background, kf)
        out.append(kf)
    _cache["host"] = (out[:3], out[3:])
    return _cache["host"]


def summary_of(gt, summ, keyframes):
    Evaluator = ec.overlay()
    gt_groups, gt_cc_group, gt_segments = keyframes.generate_fake_keyframe_info(gt)
    _, _, summ_segments = keyframes.generate_fake_keyframe_info(summ)
    with contextlib.redirect_stdout(io.StringIO()):
        metrics, names = Evaluator.compute_summary_metrics(gt_segments, gt, gt_groups, gt_cc_group, summ_segments, summ)
    prints = {}
    for name in names:
        for fn in ("print_summary_recall_metrics", "print_summary_precision_metrics", "print_compact_CC_metrics"):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                getattr(Evaluator, fn)(metrics[name], name)
            prints[fn + "|" + name] = buf.getvalue()
    return metrics, names, prints


def check_keyframe_objects(lib):
    device, keyframes = modules(lib)
    _, rec = g24()
    frames, masks = g24_inputs()
    gt, summ = device_sets(lib)
    try:
        table = gt[0].table
        assert all(kf.table is table for kf in gt + summ) and table.live
        for k, kf in enumerate(gt + summ):
            img = kf.binary_image
            assert img is kf.binary_image and img.shape == (45, 70, 3) and img.dtype == np.uint8 and (img == frames[k][:, :, None]).all()
            assert kf.object_mask.dtype == np.bool_ and (kf.object_mask == masks[k]).all()
            ccs = kf.binary_cc
            kf.update_binary_cc(False)
            assert kf.binary_cc is ccs and kf.time == float(k) and kf.objects is None and kf.raw_image is None
        # GenerateFakeKeyframeInfo
        for name, kfs in (("fake_gt", gt), ("fake_summ", summ)):
            groups, cc_group, segments = keyframes.generate_fake_keyframe_info(kfs)
            want = rec[name]
            assert segments == [tuple(s) for s in want["segments"]] and [list(d.keys()) for d in cc_group] == want["keys"]
            assert [[g.start_frame, g.cc_refs[0].strID(), len(g.cc_refs)] for g in groups] == want["groups"]
        # check_cc_overlaps_background against the restated reference method, CCs moved in and out of the frame
        host = types.SimpleNamespace(object_mask=masks[0])
        CC = ec.cc_class()
        for cc in summ[0].binary_cc[::9]:
            for dx, dy in ((0, 0), (-3, -2), (-69, 0), (-80, -50), (5, 40), (75, 0)):
                moved = CC(cc.cc_id, cc.min_x + dx, cc.max_x + dx, cc.min_y + dy, cc.max_y + dy, cc.size, cc.img)
                assert gt[0].check_cc_overlaps_background(moved) == ec.overlaps_background(host, moved), (cc.strID(), dx, dy)
        # pickling writes plain ConnectedComponents
        back = pickle.loads(pickle.dumps(summ[2].binary_cc[:5]))
        for a, b in zip(back, summ[2].binary_cc[:5]):
            assert type(a) is CC and not hasattr(a, "table")
            assert_same_cc(a, b, "pickle")
        with np.testing.assert_raises(TypeError):
            pickle.dumps(table)
        table.close()
        with np.testing.assert_raises(ValueError):
            table.image(0)
        with np.testing.assert_raises(ValueError):
            table.counts([], 0)
        with np.testing.assert_raises(ValueError):
            table.ccs(0)
    finally:
        gt[0].set.close()


def check_evaluator_reference(lib):
    """compute_summary_metrics and its reports on device keyframes: the reference's recorded values, and nothing is uploaded"""
    device, keyframes = modules(lib)
    _, rec = g24()
    gt, summ = device_sets(lib)
    try:
        created, calls = device.CCPairCounts.created, gt[0].table.calls
        metrics, names, prints = summary_of(gt, summ, keyframes)
        assert device.CCPairCounts.created == created and gt[0].table.calls > calls
        assert names == rec["range_names"]
        ec.same(metrics, ec.decode(rec["metrics"]), "metrics")
        assert prints == rec["prints"]
    finally:
        gt[0].set.close()


def check_evaluator_host_route(lib):
    """the same evaluation on the table and through the overlay's own upload route on host keyframes of the same inputs (the two
    sparser keyframes of either set; the densest is covered by the recorded values above)"""
    device, keyframes = modules(lib)
    gt, summ = device_sets(lib)
    try:
        created = device.CCPairCounts.created
        metrics, names, prints = summary_of(gt[1:], summ[1:], keyframes)
        assert device.CCPairCounts.created == created
        hgt, hsumm = host_sets(lib)
        hmetrics, hnames, hprints = summary_of(hgt[1:], hsumm[1:], keyframes)
        assert device.CCPairCounts.created > created
        assert hnames == names and hprints == prints
        ec.same(hmetrics, metrics, "host route")
    finally:
        gt[0].set.close()


def check_evaluator_moved_cc(lib):
    """after translateBox on one CC the upload route is taken and agrees with the host route given the same move"""
    device, keyframes = modules(lib)
    gt, summ = device_sets(lib)
    try:
        hgt, hsumm = host_sets(lib)
        moved_host = copy.copy(hsumm[1])
        moved_host.binary_cc = copy.deepcopy(hsumm[1].binary_cc)
        moved_host.check_cc_overlaps_background = types.MethodType(ec.overlaps_background, moved_host)
        pos = len(summ[1].binary_cc) // 2
        assert device.KeyframeCCs.pair_view([summ[1].binary_cc, gt[1].binary_cc]) is not None
        for kf in (summ[1], moved_host):
            kf.binary_cc[pos].translateBox(1, -1)
        assert not summ[1].binary_cc[pos].in_place() and device.KeyframeCCs.pair_view([summ[1].binary_cc]) is None
        assert device.KeyframeCCs.pair_view([summ[0].binary_cc, gt[1].binary_cc]) is not None
        created = device.CCPairCounts.created
        m1, n1, p1 = summary_of(gt[1:2], summ[1:2], keyframes)
        assert device.CCPairCounts.created > created
        m2, n2, p2 = summary_of(hgt[1:2], [moved_host], keyframes)
        assert n1 == n2 and p1 == p2
        ec.same(m1, m2, "moved")
        summ[1].binary_cc[pos].translateBox(-1, 1)                      # back in place: the table's item again
        assert device.KeyframeCCs.pair_view([summ[1].binary_cc]) is not None
    finally:
        gt[0].set.close()


# ---- 3. pixel metrics --------------------------------------------------------------------------------------------------------------------
def numpy_sums(gt, summ, mask):
    g, s = 255 - gt.astype(np.int64), 255 - summ.astype(np.int64)
    return [int(g.sum()), int(s.sum()), int(s[g > 0].sum()), int(s[mask == 0].sum())]


def check_pixel_sums(lib, shapes=((3, 45, 70), (2, 40, 97), (2, 1, 1), (1, 1, 65), (1, 64, 128))):
    """the device sums against numpy: non-binary bytes, with a mask and without, strides 1 and 3 (and mixed), pixel counts that are
    and are not multiples of 16"""
    device, _ = modules(lib)
    be = device.Backend(lib)
    rng = np.random.default_rng(5)
    for n, h, w in shapes:
        def frames(c):
            f = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
            f[rng.random((n, h, w)) < 0.5] = PAPER
            return f if c > 1 else f[..., 0]
        mask = (rng.random((n, h, w)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (n, h, w), dtype=np.uint8)
        for cg, cs in ((1, 1), (3, 3), (1, 3)):
            gt, summ = frames(cg), frames(cs)
            for m in (None, mask):
                got = device.pixel_sums(be.from_host(gt), be.from_host(summ), None if m is None else be.from_host(m), lib=lib)
                assert got.dtype == np.uint64 and got.shape == (n, 4)
                for k in range(n):
                    want = numpy_sums(gt[k] if cg == 1 else gt[k, :, :, 0], summ[k] if cs == 1 else summ[k, :, :, 0],
                                      m[k] if m is not None else np.zeros((h, w), np.uint8))
                    assert got[k].tolist() == want, (n, h, w, cg, cs, m is None, k)
    assert device.pixel_sums(be.from_host(np.zeros((0, 4, 4), np.uint8)), be.from_host(np.zeros((0, 4, 4), np.uint8)), lib=lib).shape == (0, 4)


def check_pixel_metrics(lib):
    device, keyframes = modules(lib)
    Evaluator = ec.overlay()
    g, rec = g24()
    gt, summ = device_sets(lib)
    extra = keyframes.keyframes_from_frames(g["extra_planes"], lib=lib)
    try:
        hgt, hsumm = host_sets(lib)
        want = Evaluator.compute_pixel_binary_metrics(hgt, hsumm)
        calls = []
        original = device.pixel_sums
        device.pixel_sums = lambda *a, **k: calls.append(1) or original(*a, **k)
        try:
            got = Evaluator.compute_pixel_binary_metrics(gt, summ)                  # one run of consecutive frames: one launch
            assert len(calls) == 1
            ec.same(got, want, "device against host")
            ec.same(got, ec.decode(rec["pixel"]), "device against the reference")
            # the degenerate branches, each against the reference and the host route (pairs from two tables: a launch per pair)
            for name, kf in zip(("pixel_empty", "pixel_covered", "pixel_disjoint"), extra):
                hkf = types.SimpleNamespace(binary_image=kf.binary_image)
                with np.errstate(all="ignore"):
                    got = Evaluator.compute_pixel_binary_metrics(gt[:1], [kf])
                    ec.same(got, Evaluator.compute_pixel_binary_metrics(hgt[:1], [hkf]), name)
                ec.same(got, ec.decode(rec[name]), name)
            assert len(calls) == 4
            # a host keyframe on either side: the host route
            ec.same(Evaluator.compute_pixel_binary_metrics(gt, hsumm), want, "mixed")
            assert len(calls) == 4
        finally:
            device.pixel_sums = original
    finally:
        gt[0].set.close()
        extra[0].set.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def check_argument_errors(lib):
    import pytest
    from lecturemath_amd import _lib
    device, keyframes = modules(lib)
    be = device.Backend(lib)
    good = paper(2, 8, 40)
    good[:, 2:4, 3:9] = 0
    with pytest.raises(ValueError, match="shape"):
        device.KeyframeCCs.from_frames(good[0], lib=lib)
    with pytest.raises(ValueError, match="uint8"):
        device.KeyframeCCs.from_frames(good.astype(np.int32), lib=lib)
    with pytest.raises(ValueError, match="masks"):
        device.KeyframeCCs.from_frames(good, masks=np.zeros((1, 8, 40), np.uint8), lib=lib)
    with pytest.raises(ValueError, match="min_pixels"):
        device.KeyframeCCs.from_frames(good, min_pixels=-1, lib=lib)
    with pytest.raises(ValueError, match="max_batch"):
        device.KeyframeCCs.from_frames(good, max_batch=0, lib=lib)
    # the C entry points themselves
    ctx = lib.lm_ctx_create(40, 8, 2)
    assert ctx
    try:
        dev = be.from_host(good)
        for args in ((None, 1, 2, 1, None, 0, 1), (_lib.ptr(dev), 1, -1, 1, None, 0, 1), (_lib.ptr(dev), 1, 2, 0, None, 0, 1),
                     (_lib.ptr(dev), 1, 2, 1, None, 1, 1), (_lib.ptr(dev), 1, 2, 1, None, 2, 1), (_lib.ptr(dev), 1, 2, 1, None, 0, -1)):
            assert not lib.lm_kf_create_from_frames(ctx, *args, be.stream()) and "bad arguments" in lib.last_error(), args
        assert not lib.lm_kf_create_from_frames(None, _lib.ptr(dev), 1, 2, 1, None, 0, 1, be.stream())
        handle = lib.lm_kf_create_from_frames(ctx, _lib.ptr(dev), 1, 2, 1, None, 0, 1, be.stream())       # the context is still usable
        assert handle and lib.lm_kf_count(handle) == 2
        lib.lm_kf_destroy(handle)
    finally:
        lib.lm_ctx_destroy(ctx)
    # records only of tables made from frames
    t = ec.table_of(lib, [[((1, 2, 1, 2), np.ones((2, 2), bool))]], 8, 8)
    try:
        assert lib.lm_kf_cc_records(t._live(), None, None) == _lib.LM_ERR_STATE and "lm_kf_create_from_frames" in lib.last_error()
    finally:
        t.close()
    assert lib.lm_kf_cc_records(None, None, None) == _lib.LM_ERR_ARG
    # pixel sums
    a = be.from_host(good)
    with pytest.raises(ValueError, match="shapes"):
        device.pixel_sums(a, be.from_host(good[:, :4]), lib=lib)
    with pytest.raises(ValueError, match="masks"):
        device.pixel_sums(a, a, be.from_host(good[:1]), lib=lib)
    sums = be.empty((2, 4), np.int64)
    for args in ((None, 1, _lib.ptr(a), 1, None, 2, 320), (_lib.ptr(a), 0, _lib.ptr(a), 1, None, 2, 320), (_lib.ptr(a), 1, _lib.ptr(a), 1, None, -1, 320),
                 (_lib.ptr(a), 1, _lib.ptr(a), 1, None, 2, 0)):
        assert lib.lm_kf_pixel_sums(*args, _lib.ptr(sums), be.stream()) == _lib.LM_ERR_ARG, args
    assert lib.lm_kf_pixel_sums(None, 1, None, 1, None, 0, 320, None, be.stream()) == _lib.LM_OK
    table = device.KeyframeCCs.from_frames(good, lib=lib)
    try:
        with pytest.raises(IndexError):
            table.items(2)
        with pytest.raises(IndexError):
            table.image(len(table))
        with pytest.raises(ValueError, match="without masks"):
            table.mask_item(0)
    finally:
        table.close()
    with pytest.raises(ValueError, match="closed"):
        table.image(0)
    with pytest.raises(ValueError, match="masks"):
        keyframes.keyframes_from_frames(good, masks=np.zeros((2, 8, 41), bool), lib=lib)


# ---- 5. full size (GPU) ------------------------------------------------------------------------------------------------------------------
def check_glyph_grid_1080p(lib):
    """one synthetic 1080p frame with a grid of about 4,000 glyphs, three channels on the device: every record and image against the
    Labeler route"""
    device, _ = modules(lib)
    rng = np.random.default_rng(21)
    plane = np.full((1080, 1920), PAPER, np.uint8)
    glyphs = 0
    for y in range(4, 1080 - 18, 24):
        for x in range(3, 1920 - 20, 21):
            lo, hi = rng.integers(0, 6, 14), rng.integers(6, 13, 14)          # a run per row across column 5: one component per cell
            g = (np.arange(12)[None, :] >= lo[:, None]) & (np.arange(12)[None, :] < hi[:, None])
            plane[y:y + 14, x:x + 12][g] = 0
            glyphs += 1
    assert glyphs >= 4000
    be = device.Backend(lib)
    frames = be.from_host(np.repeat(plane[None, :, :, None], 3, axis=3))
    table = device.KeyframeCCs.from_frames(frames, lib=lib)
    try:
        want = host_ccs(plane)
        assert len(want) == glyphs == len(table)
        assert (table.records == np.asarray([[c.cc_id, c.min_x, c.max_x, c.min_y, c.max_y, c.size] for c in want], np.int32)).all()
        for item in range(0, glyphs, 37):
            assert (table.image(item) == want[item].img).all(), item
        # every item at once: shared ink with itself = its size
        rows, counts = table.counts([(table.items(0), table.items(0), (0, 0))], 0)
        own = rows[:, 1] == rows[:, 2]
        assert (counts[own].reshape(-1) == table.records[rows[own, 1], 5]).all() and (counts[~own] == 0).all()
    finally:
        table.close()


def check_pipeline_1080p(lib):
    """the accumulate_erase stream enlarged four times to 1920 x 1080 through LecturePipeline.finish(keyframes="device",
    keyframe_ccs=True): the keyframes' CCs against the Labeler route on the host copies, and the evaluation of the set against
    itself on the table against the upload route"""
    device, keyframes = modules(lib)
    from lecturemath_amd.pipeline import LecturePipeline
    _, spec, frames = lm_checks.load_stream("accumulate_erase")
    _, params = dropin_checks.g7("accumulate_erase")
    big = np.repeat(np.repeat(frames, 4, axis=1), 4, axis=2)
    assert big.shape[1:] == (1080, 1920)
    pipe = LecturePipeline(1920, 1080, conf=dict(params[2], CC_STABILITY_MAX_GAP=spec["gap2"]), lib=lib)
    pipe.add_binary_frames(big, [1000.0 * i for i in range(len(big))], list(range(len(big))))
    out = pipe.finish(keyframes="device", keyframe_ccs=True)
    kfs = out["keyframe_ccs"]
    try:
        assert len(kfs) == len(out["keyframes"]) >= 2 and [kf.idx for kf in kfs] == list(out["summary_indices"])
        host = []
        for kf, img in zip(kfs, out["keyframes"]):
            assert (kf.binary_image == np.asarray(img)).all()
            want = host_ccs(np.ascontiguousarray(np.asarray(img)[:, :, 0]))
            assert len(want) == len(kf.binary_cc) > 10
            for j, (a, b) in enumerate(zip(kf.binary_cc, want)):
                assert_same_cc(a, b, (kf.idx, j))
            hk = types.SimpleNamespace(idx=kf.idx, binary_image=np.asarray(img), raw_image=None, object_mask=kf.object_mask.copy(), binary_cc=want)
            hk.check_cc_overlaps_background = types.MethodType(ec.overlaps_background, hk)
            host.append(hk)
        created = device.CCPairCounts.created
        metrics, names, prints = summary_of(kfs, kfs, keyframes)
        assert device.CCPairCounts.created == created
        hmetrics, hnames, hprints = summary_of(host, host, keyframes)
        assert names == hnames and prints == hprints
        ec.same(metrics, hmetrics, "1080p")
        Evaluator = ec.overlay()
        ec.same(Evaluator.compute_pixel_binary_metrics(kfs, kfs), Evaluator.compute_pixel_binary_metrics(host, host), "1080p pixel")
    finally:
        kfs[0].set.close()
