"""Checks of step 05 on the device (lm_kf_* / device.GroupImages / KeyframeExtractor.GenerateFromGroupImages /
LecturePipeline.finish(keyframes="device")) shared by the CPU tests (emulated library) and the GPU tests.  Everything is compared
bit for bit: against the reference's keyframes and CC times (G8: three segmentations of each golden stream; G8b: tie-heavy
structures), against numpy, and against device.image_pairs_overlap.

What the data exercises (check_not_vacuous computes these counts from the fixtures on the CPU, no library involved, and asserts
the inequalities; the figures are what it found when the seeds were fixed):
  * G8: in every stream EVERY segmentation has a segment with an alive group that is NOT drawn -- groups alive / drawn, summed over
    the segments, for the three segmentations: accumulate_erase 123/118, 99/81, 144/126; occluder_return 266/247, 131/86,
    173/137; short_gap_jitter 33/31, 33/31, 45/44.  A renderer that drew every alive group would fail on all three streams.
  * G8b: largest number of members of ONE overlap component that start at the same frame: case 0: 7, case 1: 180, case 2: 318
    (the tie-break of the greedy walk decides among them; at least 3 are asked for).
  * random_structure(seed=3, n=60, side=96), the generator of the overlaps checks: 129 pairs of boxes overlap, 88 of them share an
    ink pixel and 41 do not; dense_structure(): all 3,160 pairs of its 80 boxes overlap, more than the first guess of the
    candidate region of a segment (8 n + 64 = 704), so the join's capacity retry runs."""
import contextlib
import json
import os
import pickle
import sys
import types

import numpy as np

import dropin_checks
import lm_checks

WIDTHS = [1, 5, 31, 32, 33, 40, 64, 65]


def extractor():
    if dropin_checks.DROPIN not in sys.path:
        sys.path.insert(0, dropin_checks.DROPIN)
    from AccessMath.preprocessing.content.keyframe_extractor import KeyframeExtractor
    return KeyframeExtractor


# ---- fixtures (loaded once, never modified) ---------------------------------------------------------------------------------------
_cache = {}


def g4_structure(name):
    """(spec, ages, bounds, images) of a golden stream: the reference's own step-03 outputs, as check_step_05 builds them"""
    if ("g4", name) not in _cache:
        g4, spec, _ = lm_checks.load_stream(name)
        ng = len(g4["gimg_count"])
        ages = {k: [int(v[0]) for v in lm_checks.unrag(g4["ages"], g4["ages_off"])[k]] for k in range(ng)}
        bounds = {k: tuple(int(v) for v in g4["bounds"][k]) for k in range(ng)}
        images, off = {}, 0
        for k in range(ng):
            w, h = bounds[k][1] - bounds[k][0] + 1, bounds[k][3] - bounds[k][2] + 1
            images[k] = []
            for _ in range(int(g4["gimg_count"][k])):
                images[k].append(g4["gimg"][off:off + w * h].reshape(h, w).copy())
                off += w * h
        _cache[("g4", name)] = (spec, ages, bounds, images)
    return _cache[("g4", name)]


def g8(name):
    if ("g8", name) not in _cache:
        g = np.load(os.path.join(lm_checks.GOLD, "g8_step05_%s.npz" % name))
        d = {k: g[k] for k in g.files}
        d["segments"] = [[tuple(sg) for sg in segs] for segs in json.loads(bytes(d["segments"]).decode())]
        _cache[("g8", name)] = d
    return _cache[("g8", name)]


def g8b(case):
    """(meta, ages, bounds, images, golden arrays) of a tie-heavy structure"""
    if ("g8b", case) not in _cache:
        g = np.load(os.path.join(lm_checks.GOLD, "g8b_step05_ties.npz"))
        meta = json.loads(bytes(g["meta_%d" % case]).decode())
        ng, off = meta["n_groups"], g["ages_off_%d" % case]
        ages = {k: [int(v) for v in g["ages_%d" % case][off[k]:off[k + 1]]] for k in range(ng)}
        bounds = {k: tuple(int(v) for v in g["bounds_%d" % case][k]) for k in range(ng)}
        bits = np.unpackbits(g["images_%d" % case])
        images, pos = {}, 0
        for k in range(ng):
            w, h = bounds[k][1] - bounds[k][0] + 1, bounds[k][3] - bounds[k][2] + 1
            images[k] = []
            for _ in range(len(ages[k]) - 1):
                images[k].append((bits[pos:pos + w * h].reshape(h, w) * 255).astype(np.uint8))
                pos += w * h
        gold = {k: g[k] for k in g.files if k.startswith("keyframes_%d_" % case) or k.startswith("times_%d_" % case)}
        _cache[("g8b", case)] = (meta, ages, bounds, images, gold)
    return _cache[("g8b", case)]


def flat_table(ages, images, bounds):
    """the structure's images in item order (group, segment): (item_first, boxes, image list)"""
    item_first, boxes, flat = {}, [], []
    for g in ages:
        item_first[g] = len(flat)
        for im in images[g]:
            boxes.append(bounds[g])
            flat.append(im)
    return item_first, boxes, flat


def from_host(lib, ages, images, bounds, w, h):
    from lecturemath_amd import device
    item_first, boxes, flat = flat_table(ages, images, bounds)
    return device.GroupImages.from_host(boxes, flat, w, h, lib), item_first


def assert_keyframes(frames, times, gold_frames, gold_times, what=None):
    kf = np.stack([np.asarray(f) for f in frames]) if len(frames) else np.zeros((0, 1, 1, 3), np.uint8)
    assert kf.dtype == np.uint8 and kf.shape[-1] == 3, what
    assert (kf[..., 0] == kf[..., 1]).all() and (kf[..., 0] == kf[..., 2]).all(), what
    assert ((kf == 0) | (kf == 255)).all(), what
    assert (np.packbits(kf[..., 0] == 255, axis=2) == gold_frames).all(), what
    if times is not None:
        flat = np.asarray([(sidx, *t) for sidx, lst in enumerate(times) for t in lst], np.float64).reshape(-1, 6)
        assert flat.shape == gold_times.shape and (flat == gold_times).all(), what


# ---- 1. G8 through host images ------------------------------------------------------------------------------------------------------
def check_g8_host(lib, name):
    dropin_checks.use_library(lib)
    KE = extractor()
    spec, ages, bounds, images = g4_structure(name)
    g = g8(name)
    n = int(g["n_frames"])
    times = [1000.0 * i for i in range(n)]
    gi, item_first = from_host(lib, ages, images, bounds, spec["w"], spec["h"])
    try:
        assert len(gi) == sum(len(v) for v in images.values())
        for k, segs in enumerate(g["segments"]):
            frames, cc_times = KE.GenerateFromGroupImages(gi, item_first, ages, bounds, times, spec["h"], spec["w"], segs, verbose=False)
            assert isinstance(frames, list) and len(frames) == len(segs) and frames[0].shape == (spec["h"], spec["w"], 3)
            assert_keyframes(frames, cc_times, g["keyframes_%d" % k], g["times_%d" % k], (name, k))
    finally:
        gi.close()


# ---- 2. G8 through the device view ---------------------------------------------------------------------------------------------------
def run_pipeline(lib, name, keyframes):
    from lecturemath_amd.pipeline import LecturePipeline
    _, spec, frames = lm_checks.load_stream(name)
    _, params = dropin_checks.g7(name)
    pipe = LecturePipeline(spec["w"], spec["h"], conf=dict(params[2], CC_STABILITY_MAX_GAP=spec["gap2"]), lib=lib)
    n = len(frames)
    pipe.add_binary_frames(np.stack(frames), [1000.0 * i for i in range(n)], list(range(n)))
    # the fixtures ran step 02 and step 03 with different CC_STABILITY_MAX_GAP values (dropin_checks.check_pipeline)
    pipe.configuration.data["CC_STABILITY_MAX_GAP"] = str(spec["gap3"])
    return pipe, pipe.finish(keyframes=keyframes)


@contextlib.contextmanager
def no_group_image_expansion():
    """Grouping.array raises when the uint8 group images (LM_G_GIMG) are asked for"""
    from lecturemath_amd import device
    original = device.Grouping.array

    def guarded(self, which):
        if which == "gimg" or which == device._G_NAMES.index("gimg"):
            raise AssertionError("the uint8 group images were requested")
        return original(self, which)

    device.Grouping.array = guarded
    try:
        yield
    finally:
        device.Grouping.array = original


def check_g8_view(lib, name, compare_images=False):
    from lecturemath_amd import device
    dropin_checks.use_library(lib)
    KE = extractor()
    g = g8(name)
    g7_, _ = dropin_checks.g7(name)
    with no_group_image_expansion():
        pipe, out = run_pipeline(lib, name, "device")
    intervals = [tuple(int(v) for v in iv) for iv in out["intervals"]]
    assert intervals == [tuple(int(v) for v in iv) for iv in g7_["intervals_2"]] and intervals == g["segments"][0]
    st3d = out["st3d"]
    assert_keyframes(out["keyframes"], None, g["keyframes_0"], None, name)       # (the step script keeps the CC times to itself)
    dev = pipe.be.to_host(out["keyframes_device"])
    assert dev.shape == (len(intervals), st3d.height, st3d.width, 3) and (dev == np.stack(out["keyframes"])).all()
    # the structure does not carry the handle into a pickle
    assert isinstance(st3d._device_images, device.GroupImages) and isinstance(st3d.cc_group_images, device.LazyGroupImages)
    blob = pickle.dumps(st3d, protocol=pickle.HIGHEST_PROTOCOL)
    back = pickle.loads(blob)
    assert not hasattr(back, "_device_images") and not hasattr(back, "_device_keyframes") and b"GroupImages" not in blob
    assert type(back.cc_group_images) is dict and list(back.cc_group_images) == list(range(len(st3d.cc_group_ages)))
    spec, ages, bounds, images = g4_structure(name)
    assert all(len(back.cc_group_images[k]) == len(images[k]) and all((a == b).all() for a, b in zip(back.cc_group_images[k], images[k]))
               for k in images)
    if compare_images:
        _, host = run_pipeline(lib, name, "host")
        assert host["keyframes_device"] is None and (np.stack(host["keyframes"]) == np.stack(out["keyframes"])).all()
        want = host["st3d"].cc_group_images
        assert len(st3d.cc_group_images) == len(want) and len(want) > 0
        for k in want:
            assert len(st3d.cc_group_images[k]) == len(want[k])
            for j in range(len(want[k])):
                got = st3d.cc_group_images[k][j]
                assert got.dtype == np.uint8 and got.shape == want[k][j].shape and (got == want[k][j]).all(), (k, j)
    # the other two segmentations through a second view of the same run
    est = pipe.estimator
    grouping = est._cur(est._thr)
    with no_group_image_expansion():
        view = device.GroupImages.from_grouping(grouping)
        for k in (1, 2):
            frames, cc_times = KE.GenerateFromGroupImages(view, view.item_first, st3d.cc_group_ages, st3d.cc_group_boundaries, st3d.frame_times,
                                                          st3d.height, st3d.width, g["segments"][k], verbose=False)
            assert_keyframes(frames, cc_times, g["keyframes_%d" % k], g["times_%d" % k], (name, k))
        dev, cc_times = KE.GenerateFromGroupImages(view, view.item_first, st3d.cc_group_ages, st3d.cc_group_boundaries, st3d.frame_times,
                                                   st3d.height, st3d.width, g["segments"][2], verbose=False, device_frames=True)
        assert_keyframes(list(pipe.be.to_host(dev)), cc_times, g["keyframes_2"], g["times_2"], name)
    # closing the run closes its views; a closed run gives no view
    grouping.close()
    assert view.handle is None and st3d._device_images.handle is None
    try:
        device.GroupImages.from_grouping(grouping)
    except ValueError:
        pass
    else:
        raise AssertionError("from_grouping on a closed Grouping did not raise")
    try:
        view.render([[0]])
    except ValueError:
        pass
    else:
        raise AssertionError("render on a closed view did not raise")


# ---- 3. G8b ties ----------------------------------------------------------------------------------------------------------------------
def check_ties(lib, case, want_crowded=False):
    dropin_checks.use_library(lib)
    KE = extractor()
    meta, ages, bounds, images, gold = g8b(case)
    n = meta["n"]
    times = [1000.0 * i for i in range(n)]
    gi, item_first = from_host(lib, ages, images, bounds, meta["w"], meta["h"])
    try:
        for k, segs in enumerate(meta["segs"]):
            frames, cc_times = KE.GenerateFromGroupImages(gi, item_first, ages, bounds, times, meta["h"], meta["w"], [tuple(sg) for sg in segs], verbose=False)
            assert_keyframes(frames, cc_times, gold["keyframes_%d_%d" % (case, k)], gold["times_%d_%d" % (case, k)], (case, k))
        crowded = gi.crowded_tiles()
    finally:
        gi.close()
    if want_crowded:
        assert crowded > 0, "no tile took the crowded-tile path"
    return crowded


# ---- 4. overlaps ---------------------------------------------------------------------------------------------------------------------
def random_structure(seed=3, n=60, side=96):
    """the generator idea of dropin_checks.check_image_pairs: boxes at arbitrary positions, widths around the 32-bit word
    boundaries, sparse and dense ink so that overlapping boxes often hold disjoint ink"""
    rng = np.random.default_rng(seed)
    boxes, images = [], []
    for k in range(n):
        w, h = int(rng.choice(WIDTHS)), int(rng.integers(1, 20))
        x0, y0 = int(rng.integers(0, side - 1)), int(rng.integers(0, side - 1))
        img = (rng.random((h, w)) < (0.15 if k % 3 else 0.6)).astype(np.uint8) * 255
        boxes.append((x0, x0 + w - 1, y0, y0 + h - 1))
        images.append(img)
    return boxes, images, side + 80


def dense_structure(n=80):
    """n boxes of 33 x 5 crowded into 40 x 10 pixels: every pair of boxes overlaps, ink alternates between two column parities"""
    rng = np.random.default_rng(11)
    boxes, images = [], []
    for k in range(n):
        x0, y0 = int(rng.integers(0, 7)), int(rng.integers(0, 5))
        img = np.zeros((5, 33), np.uint8)
        img[:, ((x0 + k) % 2)::2] = (rng.random((5, img[:, ((x0 + k) % 2)::2].shape[1])) < 0.3) * 255
        boxes.append((x0, x0 + 32, y0, y0 + 4))
        images.append(img)
    return boxes, images, 48


def canvases(boxes, images, side):
    out = np.zeros((len(boxes), side, side), bool)
    for c, (x0, x1, y0, y1), img in zip(out, boxes, images):
        c[y0:y1 + 1, x0:x1 + 1] = img > 0
    return out


def numpy_pairs(canvas, items):
    return [(i, j) for i in range(len(items)) for j in range(i + 1, len(items)) if (canvas[items[i]] & canvas[items[j]]).any()]


def box_pairs(boxes):
    b = np.asarray(boxes, np.int64)
    hit = (b[:, None, 0] <= b[None, :, 1]) & (b[None, :, 0] <= b[:, None, 1]) & (b[:, None, 2] <= b[None, :, 3]) & (b[None, :, 2] <= b[:, None, 3])
    return [(i, j) for i, j in zip(*np.nonzero(np.triu(hit, 1)))]


def segment_lists(n_items, n_lists, seed=5):
    """item lists: all items for one list; else an empty list, a one-item list whose item also sits in the next list, random subsets"""
    rng = np.random.default_rng(seed + n_lists)
    if n_lists == 1:
        return [list(range(n_items))]
    lists = [[], [7]]
    while len(lists) < n_lists:
        size = int(rng.integers(2, n_items))
        lists.append([int(v) for v in rng.permutation(n_items)[:size]])
    if 7 not in lists[2]:
        lists[2].append(7)
    return lists


def check_overlaps(lib, structure=None, list_counts=(1, 3, 17)):
    from lecturemath_amd import _lib, device
    boxes, images, side = structure or random_structure()
    canvas = canvases(boxes, images, side)
    gi = device.GroupImages.from_host(boxes, images, side, side, lib)
    try:
        for n_lists in list_counts:
            lists = segment_lists(len(boxes), n_lists)
            want = [numpy_pairs(canvas, items) for items in lists]
            got = gi.overlaps(lists)
            assert got == want, n_lists
            for items, pairs in zip(lists, want):
                assert device.image_pairs_overlap([boxes[i] for i in items], [images[i] for i in items], lib) == pairs
            total = sum(len(p) for p in want)
            assert total > 10
            # a deliberately small room: the true count comes back with LM_ERR_CAPACITY, nothing is written past the room
            off, flat = gi._csr(lists)
            triples = np.full((4, 3), -7, np.int32)
            found = np.zeros(1, np.int64)
            rc = lib.lm_kf_overlaps(gi.handle, off.ctypes.data, flat.ctypes.data, len(lists), triples.ctypes.data, 3, found.ctypes.data, gi.be.stream())
            assert rc == _lib.LM_ERR_CAPACITY and int(found[0]) == total and (triples[3] == -7).all() and "lm_kf_overlaps" in lib.last_error()
            triples = np.zeros((total, 3), np.int32)
            rc = lib.lm_kf_overlaps(gi.handle, off.ctypes.data, flat.ctypes.data, len(lists), triples.ctypes.data, total, found.ctypes.data, gi.be.stream())
            assert rc == _lib.LM_OK and int(found[0]) == total
            assert triples.tolist() == [[s, i, j] for s, pairs in enumerate(want) for i, j in pairs]
    finally:
        gi.close()


# ---- 5. render -----------------------------------------------------------------------------------------------------------------------
def render_table(w, h, n=320, seed=21):
    """boxes inside a w x h frame: the whole frame, bars along the four edges, one-pixel boxes in the corners and inside, two
    overlapping items with common ink, then random ones"""
    rng = np.random.default_rng(seed + w)
    boxes = [(0, w - 1, 0, h - 1), (0, w - 1, 0, 0), (0, w - 1, h - 1, h - 1), (0, 0, 0, h - 1), (w - 1, w - 1, 0, h - 1),
             (0, 0, 0, 0), (w - 1, w - 1, h - 1, h - 1), (w // 2, w // 2, h // 2, h // 2), (w - 1, w - 1, 0, 0)]
    images = [(rng.random((b[3] - b[2] + 1, b[1] - b[0] + 1)) < 0.08).astype(np.uint8) * 255 for b in boxes]
    for k in (5, 6, 7, 8):
        images[k][:] = 255
    a = (w // 4, min(w - 1, w // 4 + 40), 0, min(h - 1, 9))
    for _ in range(2):      # the same box twice, the same column of ink in both
        img = (rng.random((a[3] - a[2] + 1, a[1] - a[0] + 1)) < 0.2).astype(np.uint8) * 255
        img[:, 0] = 255
        boxes.append(a)
        images.append(img)
    while len(boxes) < n:
        bw, bh = min(w, int(rng.choice(WIDTHS))), min(h, int(rng.integers(1, 20)))
        x0, y0 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        boxes.append((x0, x0 + bw - 1, y0, y0 + bh - 1))
        images.append((rng.random((bh, bw)) < 0.3).astype(np.uint8) * 255)
    return boxes, images


def numpy_keyframes(boxes, images, draw_lists, w, h, channels):
    out = np.full((len(draw_lists), h, w, channels), 255, np.uint8)
    for frame, items in zip(out, draw_lists):
        mask = np.zeros((h, w), bool)
        for i in items:
            x0, x1, y0, y1 = boxes[i]
            mask[y0:y1 + 1, x0:x1 + 1] |= images[i] > 0
        frame[mask] = 0
    return out


def check_render(lib, w, h):
    """both channel counts; one keyframe of 300 items, then five keyframes of 0, 1, 300, 1 (the whole-frame item) and 12 items; the
    output sits between two guard rows of 0x5A.  300 items on at most eight tiles: the crowded-tile path runs (counter asserted)."""
    from lecturemath_amd import device
    boxes, images = render_table(w, h)
    n = len(boxes)
    rng = np.random.default_rng(2)
    many = [int(v) for v in rng.permutation(n)[:300]]
    calls = [[many], [[], [9], [int(v) for v in rng.permutation(n)[:300]], [0], list(range(1, 13))]]
    gi = device.GroupImages.from_host(boxes, images, w, h, lib)
    try:
        for channels in (1, 3):
            for draw_lists in calls:
                row = w * channels
                body = len(draw_lists) * h * row
                buf = gi.be.from_host(np.full(body + 2 * row, 0x5A, np.uint8))
                shape = (len(draw_lists), h, w, channels)
                out = buf[row:row + body].view(*shape) if gi.be.device else buf[row:row + body].reshape(shape)
                assert gi.render(draw_lists, channels=channels, out=out) is out
                got = gi.be.to_host(buf)
                assert (got[:row] == 0x5A).all() and (got[row + body:] == 0x5A).all(), (w, h, channels)
                assert (got[row:row + body].reshape(shape) == numpy_keyframes(boxes, images, draw_lists, w, h, channels)).all(), (w, h, channels)
            fresh = gi.be.to_host(gi.render(calls[1], channels=channels))
            assert fresh.shape == (5, h, w, channels) and (fresh == numpy_keyframes(boxes, images, calls[1], w, h, channels)).all()
            assert (fresh[0] == 255).all()
        assert gi.crowded_tiles() > 0
        for k in (0, 5, 9, n - 1):
            assert (gi.image(k) == images[k]).all() and gi.image(k).dtype == np.uint8
    finally:
        gi.close()


# ---- 6. LM_KEYFRAMES ------------------------------------------------------------------------------------------------------------------
def check_env_switch(lib, monkeypatch, name="short_gap_jitter"):
    from lecturemath_amd import device
    dropin_checks.use_library(lib)
    KE = extractor()
    from AccessMath.data.space_time_struct import SpaceTimeStruct
    spec, ages, bounds, images = g4_structure(name)
    g = g8(name)
    n = int(g["n_frames"])
    st3d = SpaceTimeStruct([1000.0 * i for i in range(n)], list(range(n)), spec["h"], spec["w"], ages, images, bounds)
    monkeypatch.delenv("LM_KEYFRAMES", raising=False)
    before = device.GroupImages.created
    frames, cc_times = KE.GenerateFromST3DForIntervals(st3d, g["segments"][0], False)
    assert device.GroupImages.created == before, "the host route built a GroupImages"
    assert_keyframes(frames, cc_times, g["keyframes_0"], g["times_0"])
    monkeypatch.setenv("LM_KEYFRAMES", "device")
    for k, segs in enumerate(g["segments"]):
        frames, cc_times = KE.GenerateFromST3DForIntervals(st3d, segs, False)
        assert device.GroupImages.created == before + k + 1
        assert_keyframes(frames, cc_times, g["keyframes_%d" % k], g["times_%d" % k], k)
    monkeypatch.setenv("LM_KEYFRAMES", "host")
    KE.GenerateFromST3DForIntervals(st3d, g["segments"][1], False)
    assert device.GroupImages.created == before + 3


# ---- 7. argument checks ---------------------------------------------------------------------------------------------------------------
def check_argument_errors(lib):
    from lecturemath_amd import _lib, device
    ARG = _lib.LM_ERR_ARG
    boxes = np.asarray([[0, 3, 0, 1], [2, 5, 1, 2]], np.int32)
    img = np.full(16, 255, np.uint8)
    off = np.asarray([0, 8, 16], np.int64)
    st = device.Backend(lib).stream()

    def create(b=boxes, i=img, o=off, n=2, w=8, h=4):
        return lib.lm_kf_create_from_images(b.ctypes.data if b is not None else None, i.ctypes.data if i is not None else None,
                                            o.ctypes.data if o is not None else None, n, w, h, st)

    def refused(handle, who):
        assert not handle and who in lib.last_error(), (handle, lib.last_error())

    refused(create(b=None), "lm_kf_create_from_images")
    refused(create(i=None), "lm_kf_create_from_images")
    refused(create(o=None), "lm_kf_create_from_images")
    refused(create(n=-1), "lm_kf_create_from_images")
    refused(create(w=0), "lm_kf_create_from_images")
    refused(create(w=5), "lm_kf_create_from_images")                                       # box 1 ends at x = 5: outside a 5-wide frame
    refused(create(h=2), "lm_kf_create_from_images")
    refused(create(b=np.asarray([[-1, 2, 0, 1], [2, 5, 1, 2]], np.int32)), "lm_kf_create_from_images")
    refused(create(b=np.asarray([[3, 0, 0, 1], [2, 5, 1, 2]], np.int32)), "lm_kf_create_from_images")
    refused(create(o=np.asarray([0, 7, 16], np.int64)), "lm_kf_create_from_images")       # size mismatch
    refused(lib.lm_kf_create_from_group(None), "lm_kf_create_from_group")
    assert lib.lm_kf_count(None) == -1
    lib.lm_kf_destroy(None)
    kf = create()
    assert kf and lib.lm_kf_count(kf) == 2
    try:
        seg = np.asarray([0, 2], np.int64)
        items = np.asarray([0, 1], np.int32)
        tri = np.zeros((4, 3), np.int32)
        found = np.zeros(1, np.int64)

        def overlaps(k=kf, s=seg, it=items, n=1, t=tri, cap=4, f=found):
            return lib.lm_kf_overlaps(k, s.ctypes.data if s is not None else None, it.ctypes.data if it is not None else None, n,
                                      t.ctypes.data if t is not None else None, cap, f.ctypes.data if f is not None else None, st)

        assert overlaps() == _lib.LM_OK and int(found[0]) == 1 and tri[0].tolist() == [0, 0, 1]
        bad = [dict(k=None), dict(s=None), dict(it=None), dict(f=None), dict(t=None), dict(cap=-1), dict(n=-1),
               dict(s=np.asarray([0, 2, 1], np.int64), n=2), dict(s=np.asarray([1, 2], np.int64)),
               dict(it=np.asarray([0, 2], np.int32)), dict(it=np.asarray([-1, 1], np.int32))]
        for kw in bad:
            assert overlaps(**kw) == ARG and "lm_kf_overlaps" in lib.last_error(), kw
        be = device.Backend(lib)
        out = be.from_host(np.zeros(8 * 4 * 3, np.uint8))

        def render(k=kf, s=seg, it=items, n=1, ch=3, o=out):
            return lib.lm_kf_render(k, s.ctypes.data if s is not None else None, it.ctypes.data if it is not None else None, n, ch, _lib.ptr(o), st)

        assert render() == _lib.LM_OK
        be.synchronize()
        bad = [dict(k=None), dict(s=None), dict(it=None), dict(o=None), dict(n=-1), dict(ch=2), dict(ch=0), dict(ch=4),
               dict(s=np.asarray([0, 2, 1], np.int64), n=2), dict(s=np.asarray([1, 2], np.int64)),
               dict(it=np.asarray([0, 2], np.int32)), dict(it=np.asarray([-1, 1], np.int32))]
        for kw in bad:
            assert render(**kw) == ARG and "lm_kf_render" in lib.last_error(), kw
        one = np.zeros(8, np.uint8)
        assert lib.lm_kf_image(kf, 1, one.ctypes.data, 8, st) == _lib.LM_OK and (one == 255).all()
        for args in ((None, 1, one.ctypes.data, 8), (kf, 2, one.ctypes.data, 8), (kf, -1, one.ctypes.data, 8), (kf, 1, None, 8), (kf, 1, one.ctypes.data, 7)):
            assert lib.lm_kf_image(*args, st) == ARG and "lm_kf_image" in lib.last_error(), args
        assert lib.lm_kf_crowded_tiles(kf, None, st) == ARG and lib.lm_kf_crowded_tiles(None, found.ctypes.data, st) == ARG
    finally:
        lib.lm_kf_destroy(kf)
    # the Python layer
    for call in (lambda: device.GroupImages.from_grouping(types.SimpleNamespace(handle=None)),
                 lambda: device.GroupImages.from_host([(0, 8, 0, 1)], [np.zeros((2, 9), np.uint8)], 8, 4, lib)):
        try:
            call()
        except (ValueError, _lib.LecturemathError):
            pass
        else:
            raise AssertionError("no exception")
    gi = device.GroupImages.from_host([], [], 16, 2, lib)      # an empty table renders white keyframes
    assert len(gi) == 0 and gi.overlaps([[], []]) == [[], []] and (gi.be.to_host(gi.render([[]], channels=1)) == 255).all()
    gi.close()
    for call in (lambda: gi.overlaps([[0]]), lambda: gi.image(0), lambda: pickle.dumps(gi)):
        try:
            call()
        except (ValueError, TypeError):
            pass
        else:
            raise AssertionError("no exception")
    # a group without a segment image raises IndexError like the reference and the host route
    gi, item_first = from_host(lib, {0: [0, 5]}, {0: [np.full((2, 2), 255, np.uint8)]}, {0: (0, 1, 0, 1)}, 8, 4)
    try:
        extractor().GenerateFromGroupImages(gi, {0: 0, 1: 1}, {0: [0, 5], 1: [3]}, {0: (0, 1, 0, 1), 1: (0, 1, 0, 1)}, [0.0] * 6, 4, 8, [(0, 5)], False)
    except IndexError:
        pass
    else:
        raise AssertionError("no IndexError")
    finally:
        gi.close()


# ---- 8. vacuity guard (CPU, no library) ---------------------------------------------------------------------------------------------
def host_pairs(boxes, images):
    """pairs (i < j) that share an ink pixel, by numpy on the box intersections"""
    out = []
    for i, j in box_pairs(boxes):
        a, b = boxes[i], boxes[j]
        x0, x1, y0, y1 = max(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), min(a[3], b[3])
        if ((images[i][y0 - a[2]:y1 - a[2] + 1, x0 - a[0]:x1 - a[0] + 1] > 0) & (images[j][y0 - b[2]:y1 - b[2] + 1, x0 - b[0]:x1 - b[0] + 1] > 0)).any():
            out.append((int(i), int(j)))
    return out


def vacuity_counts():
    KE = extractor()
    counts = {"g8": {}, "g8b": {}}
    for name in lm_checks.STREAMS:
        _, ages, _, _ = g4_structure(name)
        g = g8(name)
        per = []
        for k, segs in enumerate(g["segments"]):
            _, _, selection = KE._segment_selection(ages, segs)
            per.append((sum(len(alive) for alive, _ in selection), len(g["times_%d" % k]),
                        any(len(alive) > int((g["times_%d" % k][:, 0] == s).sum()) for s, (alive, _) in enumerate(selection))))
        counts["g8"][name] = per
    for case in range(3):
        meta, ages, bounds, images, _ = g8b(case)
        best = 0
        for segs in meta["segs"]:
            group_ids, first, selection = KE._segment_selection(ages, [tuple(sg) for sg in segs])
            for alive, ks in selection:
                bx = [bounds[group_ids[a]] for a in alive]
                im = [images[group_ids[a]][k] for a, k in zip(alive, ks)]
                components, _ = KE._component_member_order(len(bx), host_pairs(bx, im))
                for comp in components:
                    starts = first[alive[np.asarray(comp)]]
                    best = max(best, int(np.bincount(starts - starts.min()).max()))
        counts["g8b"][case] = best
    boxes, images, _ = random_structure()
    bp, ink = box_pairs(boxes), host_pairs(boxes, images)
    counts["random"] = (len(bp), len(ink), len(bp) - len(ink))
    counts["dense"] = len(box_pairs(dense_structure()[0]))
    return counts


def check_not_vacuous():
    c = vacuity_counts()
    for name, per in c["g8"].items():
        assert any(flag for _, _, flag in per), (name, per)
    assert max(c["g8b"].values()) >= 3, c["g8b"]
    n_box, n_ink, n_dry = c["random"]
    assert n_ink > 10 and n_dry > 10, c["random"]
    n = len(dense_structure()[0])
    assert c["dense"] == n * (n - 1) // 2 > 8 * n + 64
    return c
