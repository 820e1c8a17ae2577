"""Checks of the pixel history on the device (lm_hist_* / device.FrameHistory / CCStabilityEstimator.
compute_group_images_from_raw_binary / KeyframeExtractor.extract) shared by the CPU tests (emulated library) and the GPU tests.
Everything is compared bit for bit, there are no tolerances.

Fixtures (tests/golden/make_golden_history.py ran the reference itself, cc_stability_estimator.py:502-573 and
keyframe_extractor.py:146-222):
  g23_history_<stream>.npz     the three golden streams: the reference's groups, ages and the unique CCs they name; its raw-binary
                               group images at thresholds 0, 127, 127.5, 254, 255 and -1; extract() on three segment sets at
                               treshold_length 1, 4.5 and n + 1; the reference's step-05 keyframes from the threshold-127 images
  g23_history_synthetic.npz    "long" (24 x 70, 300 frames, segments [0, 256] and [257, 299]: counts cross 255 / 256), "wide"
                               (40 x 1100, W % 32 == 12: a group box x 13..1067 of overlapping members, boxes of width 1, 2 and 33
                               that start at x % 32 == 31, a box touching the right and bottom edges, a member that leaves its
                               group before the second age segment), "stranger" (all-zero frames: maximum 0, thresholds 0 and -1)
The reference does not return an image's maximum count; the stored maxima are those of numpy_raw_images below, which the generator
asserted equal to the reference image by image before it stored anything.

numpy_raw_images / numpy_extract restate both methods in numpy.  check_restatement asserts them equal to every fixture (CPU, no
library); the random cases of both builds compare against them, the reference not being where the GPU tests run.

What the data exercises (check_not_vacuous asserts the inequalities; the figures are the reference's own):
  * raw-binary images at threshold 127 that differ from compute_group_images(..., 0.5) (the G4 fixture): accumulate_erase 113 of
    345, occluder_return 187 of 446, short_gap_jitter 25 of 77; at least 100 / 150 / 20 are asked for
  * at threshold 255 every image is empty; the maximum of the "long" case is 257 > 255"""
import json
import os
import pickle
import sys
import types

import numpy as np

import dropin_checks
import keyframe_checks
import lm_checks

THRESHOLDS = [0, 127, 127.5, 254, 255, -1]
TRESHOLD_LENGTHS = ["1", "4.5", "n+1"]
MIN_DIFFERENT = {"accumulate_erase": 100, "occluder_return": 150, "short_gap_jitter": 20}
SYNTHETIC = ["long", "wide", "stranger"]


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------
def numpy_raw_images(cc_boxes, cc_images, cc_life, cc_groups, group_ages, frames, threshold):
    """compute_group_images_from_raw_binary: ({group: [uint8 image per age segment]}, {group: box}, {group: [maximum count]})"""
    ink = np.asarray(frames) == 255
    images, bounds, maxima = {}, {}, {}
    for g, group in enumerate(cc_groups):
        if len(group) == 0:
            continue
        b = np.asarray([cc_boxes[c] for c in group], np.int64)
        x0, x1, y0, y1 = int(b[:, 0].min()), int(b[:, 1].max()), int(b[:, 2].min()), int(b[:, 3].max())
        bounds[g] = (x0, x1, y0, y1)
        images[g], maxima[g] = [], []
        ages = group_ages[g]
        for k in range(len(ages) - 1):
            t0, t1 = int(ages[k]), int(ages[k + 1])
            mask = np.zeros((y1 - y0 + 1, x1 - x0 + 1), bool)
            for c in group:
                if cc_life[c][0] <= t1 and t0 <= cc_life[c][1]:
                    cx0, cx1, cy0, cy1 = cc_boxes[c]
                    mask[cy0 - y0:cy1 - y0 + 1, cx0 - x0:cx1 - x0 + 1] |= np.asarray(cc_images[c]) > 0
            count = (ink[t0:t1 + 1, y0:y1 + 1, x0:x1 + 1] & mask).sum(axis=0, dtype=np.int64)
            m = int(count.max())
            scaled = (count * 255) // m if m > 0 else np.zeros_like(count)       # numpy's int32 // 0 yields 0
            images[g].append((scaled > threshold).astype(np.uint8) * 255)
            maxima[g].append(m)
    return images, bounds, maxima


def numpy_extract(frames, video_segments, treshold_length):
    """KeyframeExtractor.extract with "local_max" as the frame's index"""
    ink = np.asarray(frames) == 255
    per_frame = ink.reshape(len(ink), -1).sum(axis=1)
    out = []
    for s, e in video_segments:
        part = ink[s:e + 1]
        total = part.sum(axis=0, dtype=np.int64).astype(np.float32)
        age = np.where(part.any(axis=0), s + part.argmax(axis=0), 0).astype(np.float32)
        out.append({"start": s, "end": e, "sum": total, "age": age, "filtered": (total >= treshold_length).astype(np.uint8) * 255,
                    "local_max": s + int(np.argmax(per_frame[s:e + 1]))})
    return out


# ---- fixtures (loaded once, never modified) ---------------------------------------------------------------------------------------
_cache = {}


def _unpack_images(packed, shapes):
    bits = np.unpackbits(packed)
    out, pos = [], 0
    for h, w in shapes:
        out.append((bits[pos:pos + h * w].reshape(h, w) * 255).astype(np.uint8))
        pos += h * w
    return out


def _case(g, prefix):
    """the inputs and the reference's images of one case stored under `prefix` in the npz `g`"""
    meta = json.loads(bytes(g[prefix + "meta"]).decode())
    cc_boxes = [tuple(int(v) for v in b) for b in g[prefix + "cc_boxes"]]
    cc_images = _unpack_images(g[prefix + "cc_images"], [(b[3] - b[2] + 1, b[1] - b[0] + 1) for b in cc_boxes])
    cc_life = [tuple(int(v) for v in b) for b in g[prefix + "cc_life"]]
    goff, aoff = g[prefix + "groups_off"], g[prefix + "ages_off"]
    groups = [[int(c) for c in g[prefix + "groups"][goff[k]:goff[k + 1]]] for k in range(len(goff) - 1)]
    ages = {k: [int(a) for a in g[prefix + "ages"][aoff[k]:aoff[k + 1]]] for k in range(len(aoff) - 1)}
    bounds = {int(k): tuple(int(v) for v in b) for k, b in zip(g[prefix + "bound_groups"], g[prefix + "bounds"])}
    shapes = [(bounds[k][3] - bounds[k][2] + 1, bounds[k][1] - bounds[k][0] + 1) for k in bounds for _ in range(len(ages[k]) - 1)]
    raw = {}
    for ti, thr in enumerate(meta["thresholds"]):
        flat, pos = _unpack_images(g[prefix + "raw_%d" % ti], shapes), 0
        raw[thr] = {}
        for k in bounds:
            raw[thr][k] = flat[pos:pos + len(ages[k]) - 1]
            pos += len(ages[k]) - 1
    maxima, pos = {}, 0
    for k in bounds:
        maxima[k] = [int(v) for v in g[prefix + "raw_max"][pos:pos + len(ages[k]) - 1]]
        pos += len(ages[k]) - 1
    return {"meta": meta, "cc_boxes": cc_boxes, "cc_images": cc_images, "cc_life": cc_life, "groups": groups, "ages": ages, "bounds": bounds,
            "raw": raw, "maxima": maxima}


def _extract_gold(g, prefix, meta):
    out = []
    for si, segs in enumerate(meta["segment_sets"]):
        per_thr = {}
        for li, name in enumerate(meta["treshold_lengths"]):
            per_thr[name] = {"filtered": (np.unpackbits(g[prefix + "filtered_%d_%d" % (si, li)], axis=2)[:, :, :meta["w"]] * 255).astype(np.uint8),
                             "local_max": [int(v) for v in g[prefix + "local_max_%d_%d" % (si, li)]]}
        out.append({"segments": [tuple(sg) for sg in segs], "sum": g[prefix + "sum_%d" % si].astype(np.float32),
                    "age": g[prefix + "age_%d" % si].astype(np.float32), "by_length": per_thr})
    return out


def stream_case(name):
    if name not in _cache:
        g = np.load(os.path.join(lm_checks.GOLD, "g23_history_%s.npz" % name))
        c = _case(g, "")
        c["frames"] = lm_checks.load_stream(name)[2]
        c["extract"] = _extract_gold(g, "x_", c["meta"])
        c["segments05"] = [tuple(sg) for sg in c["meta"]["segments05"]]
        c["keyframes05"], c["times05"] = g["keyframes05"], g["times05"]
        _cache[name] = c
    return _cache[name]


def synthetic_case(name):
    if name not in _cache:
        g = np.load(os.path.join(lm_checks.GOLD, "g23_history_synthetic.npz"))
        c = _case(g, name + "_")
        m = c["meta"]
        c["frames"] = (np.unpackbits(g[name + "_frames"], axis=2)[:, :, :m["w"]] * 255).astype(np.uint8)
        c["extract"] = _extract_gold(g, name + "_x_", m) if m.get("segment_sets") else []
        _cache[name] = c
    return _cache[name]


def any_case(name):
    return synthetic_case(name) if name in SYNTHETIC else stream_case(name)


def length_value(name, n):
    return {"1": 1, "4.5": 4.5, "n+1": n + 1}[name] if isinstance(name, str) and name in ("1", "4.5", "n+1") else float(name)


# ---- 1. the restatement against every fixture (CPU, no library) ------------------------------------------------------------------
def check_restatement(name):
    c = any_case(name)
    for thr in c["meta"]["thresholds"]:
        images, bounds, maxima = numpy_raw_images(c["cc_boxes"], c["cc_images"], c["cc_life"], c["groups"], c["ages"], c["frames"], thr)
        assert bounds == c["bounds"] and maxima == c["maxima"], (name, thr)
        assert list(images) == list(c["raw"][thr])
        for k in images:
            assert len(images[k]) == len(c["raw"][thr][k])
            for a, b in zip(images[k], c["raw"][thr][k]):
                assert a.shape == b.shape and (a == b).all(), (name, thr, k)
    n = len(c["frames"])
    for gold in c["extract"]:
        for lname, per in gold["by_length"].items():
            got = numpy_extract(c["frames"], gold["segments"], length_value(lname, n))
            assert_extract(got, gold, per, c["frames"], (name, lname))


def assert_extract(got, gold, per, frames, what, local_max_is=None):
    assert len(got) == len(gold["segments"]), what
    for i, (seg, (s, e)) in enumerate(zip(got, gold["segments"])):
        assert (seg["start"], seg["end"]) == (s, e), what
        assert seg["sum"].dtype == np.float32 and seg["age"].dtype == np.float32 and seg["filtered"].dtype == np.uint8, what
        assert (np.asarray(seg["sum"]) == gold["sum"][i]).all() and (np.asarray(seg["age"]) == gold["age"][i]).all(), what
        assert (seg["filtered"] == per["filtered"][i]).all(), what
        if isinstance(seg["local_max"], (int, np.integer)):
            assert seg["local_max"] == per["local_max"][i], what
        else:
            lm = np.asarray(seg["local_max"])
            assert lm.dtype == np.uint8 and (lm == frames[per["local_max"][i]]).all(), what
            if local_max_is is not None:
                assert seg["local_max"] is local_max_is[per["local_max"][i]], what


# ---- 2. vacuity guard (CPU, no library) -------------------------------------------------------------------------------------------
def different_from_crop_voting(name):
    """(images of the reference's raw-binary voting at threshold 127 that differ from its compute_group_images(..., 0.5), images)"""
    c = stream_case(name)
    _, _, _, crop_images = keyframe_checks.g4_structure(name)
    differ = total = 0
    for k in c["raw"][127]:
        assert len(c["raw"][127][k]) == len(crop_images[k])
        for a, b in zip(c["raw"][127][k], crop_images[k]):
            total += 1
            differ += int(a.shape != b.shape or (a != b).any())
    return differ, total


def check_not_vacuous():
    for name in lm_checks.STREAMS:
        differ, total = different_from_crop_voting(name)
        assert differ >= MIN_DIFFERENT[name], (name, differ, total)
        assert all(not im.any() for lst in stream_case(name)["raw"][255].values() for im in lst), name
        assert any(im.any() for lst in stream_case(name)["raw"][254].values() for im in lst), name
    assert max(m for lst in synthetic_case("long")["maxima"].values() for m in lst) > 255
    assert all(m == 0 for lst in synthetic_case("stranger")["maxima"].values() for m in lst)
    assert all(im.all() for lst in synthetic_case("stranger")["raw"][-1].values() for im in lst)
    assert synthetic_case("wide")["meta"]["w"] % 32 == 12
    assert any(b[1] == synthetic_case("wide")["meta"]["w"] - 1 and b[3] == synthetic_case("wide")["meta"]["h"] - 1
               for b in synthetic_case("wide")["bounds"].values())


# ---- the overlay on a fixture's inputs ---------------------------------------------------------------------------------------------
def estimator_class():
    if dropin_checks.DROPIN not in sys.path:
        sys.path.insert(0, dropin_checks.DROPIN)
    from AccessMath.preprocessing.content.cc_stability_estimator import CCStabilityEstimator
    return CCStabilityEstimator


def bare_estimator(c):
    """the overlay's estimator with hand-set unique_cc_objects / unique_cc_frames, as the generator drove the reference's"""
    est = estimator_class().__new__(estimator_class())
    est.unique_cc_objects = [types.SimpleNamespace(min_x=b[0], max_x=b[1], min_y=b[2], max_y=b[3], img=im) for b, im in zip(c["cc_boxes"], c["cc_images"])]
    est.unique_cc_frames = [[(first, 1), (last, 1)] for first, last in c["cc_life"]]
    return est


def assert_raw_images(images, bounds, c, thr, what):
    assert list(images.keys()) == list(c["raw"][thr]) and len(images) == len(c["raw"][thr]), what
    assert {k: tuple(int(v) for v in b) for k, b in bounds.items()} == c["bounds"], what
    for k in c["raw"][thr]:
        assert len(images[k]) == len(c["raw"][thr][k]), (what, k)
        for j, want in enumerate(c["raw"][thr][k]):
            got = images[k][j]
            assert got.dtype == np.uint8 and got.shape == want.shape and (got == want).all(), (what, k, j)


# ---- 3. raw-binary images against the reference ------------------------------------------------------------------------------------
def check_raw_images(lib, name, thresholds=None):
    from lecturemath_amd import device
    dropin_checks.use_library(lib)
    c = any_case(name)
    est = bare_estimator(c)
    m = c["meta"]
    hist = device.FrameHistory.from_frames(c["frames"], lib)
    try:
        for thr in (thresholds if thresholds is not None else m["thresholds"]):
            images, bounds = est.compute_group_images_from_raw_binary(c["groups"], c["ages"], hist, thr)
            assert isinstance(images, device.LazyGroupImages)
            assert_raw_images(images, bounds, c, thr, (name, thr))
            gi = images.device_images
            assert all(gi.item_first[k] == sum(len(c["ages"][q]) - 1 for q in c["bounds"] if q < k) for k in c["bounds"])
            gi.close()
        assert hist.appends == 1 and len(hist) == len(c["frames"])
        # the maxima, straight from the device layer
        keys = list(c["bounds"])
        masks = device.GroupImages.from_host(c["cc_boxes"], c["cc_images"], m["w"], m["h"], lib)
        boxes = [c["bounds"][k] for k in keys for _ in range(len(c["ages"][k]) - 1)]
        ranges = [(c["ages"][k][j], c["ages"][k][j + 1]) for k in keys for j in range(len(c["ages"][k]) - 1)]
        lists = [[q for q in c["groups"][k] if c["cc_life"][q][0] <= t1 and t0 <= c["cc_life"][q][1]]
                 for k in keys for t0, t1 in zip(c["ages"][k][:-1], c["ages"][k][1:])]
        gi, maxima = hist.masked_images(masks, boxes, ranges, lists, 127)
        assert maxima.dtype == np.int64 and maxima.tolist() == [v for k in keys for v in c["maxima"][k]], name
        flat = [im for k in keys for im in c["raw"][127][k]] if 127 in c["raw"] else None
        if flat is not None:
            assert len(gi) == len(flat) and all((gi.image(i) == flat[i]).all() for i in range(0, len(flat), 7))
        gi.close()
        masks.close()
    finally:
        hist.close()


def check_raw_images_from_a_list(lib, name="short_gap_jitter"):
    """a plain list of frames (the reference's own argument) and, on the GPU, a device tensor give the same images"""
    from lecturemath_amd import device
    dropin_checks.use_library(lib)
    c = stream_case(name)
    est = bare_estimator(c)
    before = device.GroupImages.created
    images, bounds = est.compute_group_images_from_raw_binary(c["groups"], c["ages"], list(c["frames"]), 127.5)
    assert_raw_images(images, bounds, c, 127.5, name)
    assert device.GroupImages.created == before + 2            # the mask table and the images
    be = device.Backend(lib)
    images, bounds = est.compute_group_images_from_raw_binary(c["groups"], c["ages"], be.from_host(c["frames"]), 0)
    assert_raw_images(images, bounds, c, 0, name)
    # empty groups are skipped, like the reference does; the cached grouping is not consulted (a bare estimator has none)
    groups = [[]] + c["groups"]
    ages = {0: [0, 1]}
    ages.update({k + 1: v for k, v in c["ages"].items()})
    images, bounds = est.compute_group_images_from_raw_binary(groups, ages, list(c["frames"]), 127)
    assert 0 not in images and 0 not in bounds and list(images.keys()) == [k + 1 for k in c["bounds"]]
    assert all((images[k + 1][0] == c["raw"][127][k][0]).all() for k in c["bounds"] if c["raw"][127][k])
    blob = pickle.dumps(images, protocol=pickle.HIGHEST_PROTOCOL)
    back = pickle.loads(blob)
    assert type(back) is dict and list(back) == list(images.keys()) and b"GroupImages" not in blob


def check_after_steps_02_03(lib, name="short_gap_jitter"):
    """the overlay's own steps 02-03, then the raw-binary images: the unique CCs come from the device without the estimator's
    attributes being materialised, and from the attributes once they are; a grouping other than the cached one is honoured"""
    import contextlib
    import io
    dropin_checks.use_library(lib)
    c = stream_case(name)
    spec = lm_checks.load_stream(name)[1]
    est = estimator_class()(spec["w"], spec["h"], 0.85, 0.85, spec["gap2"], False)
    for f in c["frames"]:
        est.add_frame(f, True)
    with contextlib.redirect_stdout(io.StringIO()):
        est.split_stable_cc_by_gaps(spec["gap3"], 3)
        stable = est.get_stable_cc_idxs(3)
        time_ov, _, _ = est.compute_overlapping_stable_cc(stable, 5)
        groups, _ = est.compute_groups(stable, time_ov, 0.5, None, None)
        ages, _ = est.compute_groups_temporal_information(groups)
    assert {k: [int(a) for a in v] for k, v in ages.items()} == c["ages"]
    images, bounds = est.compute_group_images_from_raw_binary(groups, ages, list(c["frames"]), 127)
    assert est._host is None, "the estimator's attributes were materialised"
    assert_raw_images(images, bounds, c, 127, name)
    assert all(isinstance(v, np.int32) for b in bounds.values() for v in b)
    # another grouping than the cached one: the first two groups as one, its ages the union of theirs
    used = sorted({int(u) for group in groups for u in group})
    slot = {u: i for i, u in enumerate(used)}
    assert [[slot[int(u)] for u in group] for group in groups] == c["groups"]
    merged = [list(groups[0]) + list(groups[1])] + [list(group) for group in groups[2:]]
    merged_ages = {0: sorted(set(ages[0]) | set(ages[1]))}
    merged_ages.update({k - 1: list(ages[k]) for k in range(2, len(groups))})
    want, wbounds, _ = numpy_raw_images(c["cc_boxes"], c["cc_images"], c["cc_life"], [[slot[int(u)] for u in group] for group in merged], merged_ages,
                                        c["frames"], 127)
    est.unique_cc_objects                       # materialised from here on
    assert est._host is not None
    images, bounds = est.compute_group_images_from_raw_binary(merged, merged_ages, list(c["frames"]), 127)
    assert list(images.keys()) == list(want) and {k: tuple(int(v) for v in b) for k, b in bounds.items()} == wbounds
    assert all(len(images[k]) == len(want[k]) and all((images[k][j] == want[k][j]).all() for j in range(len(want[k]))) for k in want)
    assert all(isinstance(v, np.int32) for b in bounds.values() for v in b)


# ---- 4. step 05 from the raw-binary images ------------------------------------------------------------------------------------------
def check_step05(lib, name):
    """the reference's keyframes from ITS threshold-127 raw-binary images, by the host route (the images expanded to uint8) and by
    the device route (the bit rows as they are)"""
    from lecturemath_amd import device
    dropin_checks.use_library(lib)
    KE = keyframe_checks.extractor()
    from AccessMath.data.space_time_struct import SpaceTimeStruct
    c = stream_case(name)
    m = c["meta"]
    n = len(c["frames"])
    times = [1000.0 * i for i in range(n)]
    images, bounds = bare_estimator(c).compute_group_images_from_raw_binary(c["groups"], c["ages"], c["frames"], 127)
    gi = images.device_images
    frames, cc_times = KE.GenerateFromGroupImages(gi, gi.item_first, c["ages"], bounds, times, m["h"], m["w"], c["segments05"], verbose=False)
    keyframe_checks.assert_keyframes(frames, cc_times, c["keyframes05"], c["times05"], (name, "device"))
    host_images = {k: list(images[k]) for k in images}
    st3d = SpaceTimeStruct(times, list(range(n)), m["h"], m["w"], c["ages"], host_images, bounds)
    os.environ.pop("LM_KEYFRAMES", None)
    before = device.GroupImages.created
    frames, cc_times = KE.GenerateFromST3DForIntervals(st3d, c["segments05"], False)
    assert device.GroupImages.created == before, "the host route built a GroupImages"
    keyframe_checks.assert_keyframes(frames, cc_times, c["keyframes05"], c["times05"], (name, "host"))
    gi.close()


# ---- 5. extract against the reference ----------------------------------------------------------------------------------------------
def check_extract(lib, name):
    from lecturemath_amd import device
    dropin_checks.use_library(lib)
    KE = keyframe_checks.extractor()
    c = any_case(name)
    n = len(c["frames"])
    as_list = list(c["frames"])
    hist = device.FrameHistory.from_frames(c["frames"], lib)
    try:
        assert (hist.ink_counts() == (c["frames"] == 255).reshape(n, -1).sum(axis=1)).all()
        for si, gold in enumerate(c["extract"]):
            for lname, per in gold["by_length"].items():
                source, same = (as_list, as_list) if (si + len(lname)) % 2 else (hist, None)
                got = KE.extract(source, gold["segments"], length_value(lname, n))
                assert_extract(got, gold, per, c["frames"], (name, si, lname), local_max_is=same)
        assert hist.appends == 1
    finally:
        hist.close()


def check_extract_inputs(lib, tmp_path, name="short_gap_jitter"):
    """device tensor input; the saved PNG; a history shared by both methods uploads once"""
    from lecturemath_amd import device, png
    dropin_checks.use_library(lib)
    KE = keyframe_checks.extractor()
    c = stream_case(name)
    n = len(c["frames"])
    gold = c["extract"][1]
    be = device.Backend(lib)
    prefix = os.path.join(str(tmp_path), "kf")
    got = KE.extract(be.from_host(c["frames"]), gold["segments"], 4.5, save_prefix=prefix)
    assert_extract(got, gold, gold["by_length"]["4.5"], c["frames"], name)
    for i in range(len(gold["segments"])):
        data = np.fromfile("%s_filt_seg_%d.png" % (prefix, i + 1), np.uint8)
        assert (png.decode_gray8(data) == gold["by_length"]["4.5"]["filtered"][i]).all()
    hist = device.FrameHistory(c["meta"]["w"], c["meta"]["h"], n, lib)
    try:
        hist.append(c["frames"])
        images, bounds = bare_estimator(c).compute_group_images_from_raw_binary(c["groups"], c["ages"], hist, 254)
        assert_raw_images(images, bounds, c, 254, name)
        got = KE.extract(hist, gold["segments"], 1)
        assert_extract(got, gold, gold["by_length"]["1"], c["frames"], name)
        assert hist.appends == 1 and len(hist) == n
    finally:
        hist.close()


# ---- 6. appending ------------------------------------------------------------------------------------------------------------------
def random_frames(n, h, w, seed, p=0.3):
    rng = np.random.default_rng(seed)
    return ((rng.random((n, h, w)) < p) * 255).astype(np.uint8)


def check_append_batches(lib, h=19, w=77):
    """7 + 1 + rest equals one batch; W % 16 != 0 and W % 16 == 0 (the vector loads of the packing); device input equals host input"""
    from lecturemath_amd import device
    be = device.Backend(lib)
    for width in (w, 96, 48):
        frames = random_frames(23, h, width, 5 + width)
        one = device.FrameHistory(width, h, 23, lib)
        parts = device.FrameHistory(width, h, 40, lib)
        dev = device.FrameHistory(width, h, 23, lib)
        try:
            one.append(frames)
            parts.append(frames[:7])
            parts.append([frames[7]])
            parts.append(list(frames[8:]))
            dev.append(be.from_host(frames))
            assert len(one) == len(parts) == len(dev) == 23 and parts.appends == 3
            want = numpy_extract(frames, [(0, 22), (3, 9), (22, 22)], 2)
            for hist in (one, parts, dev):
                assert (hist.ink_counts() == (frames == 255).reshape(23, -1).sum(axis=1)).all()
                assert (hist.ink_counts(5, 3) == (frames[5:8] == 255).reshape(3, -1).sum(axis=1)).all()
                for seg in want:
                    total, age = hist.segment_stats(seg["start"], seg["end"], host=True)
                    assert total.dtype == np.float32 and (total == seg["sum"]).all() and (age == seg["age"]).all()
                for t in (0, 7, 8, 22):
                    assert (hist.frame(t) == frames[t]).all()
            total, age = one.segment_stats(0, 22)
            assert (be.to_host(total) == want[0]["sum"]).all() and (be.to_host(age) == want[0]["age"]).all()
        finally:
            one.close()
            parts.close()
            dev.close()


# ---- 7. random jobs against the restatement ------------------------------------------------------------------------------------------
def check_random_jobs(lib, h=45, w=140, n=40, seed=9):
    """boxes at arbitrary positions with widths around the word boundaries, overlapping masks, frame ranges of every length up to
    n (the unrolled frame loop's remainders), every threshold: against numpy_raw_images, each job as a group of its own"""
    from lecturemath_amd import device
    rng = np.random.default_rng(seed)
    frames = random_frames(n, h, w, seed + 1, p=0.6)
    cc_boxes, cc_images, cc_life, groups, ages = [], [], [], [], {}
    for g in range(60):
        bw, bh = min(w, int(rng.choice(keyframe_checks.WIDTHS + [100, w]))), int(rng.integers(1, 18))
        x0, y0 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        members = []
        for _ in range(int(rng.integers(1, 4))):
            mw, mh = int(rng.integers(1, bw + 1)), int(rng.integers(1, bh + 1))
            mx, my = x0 + int(rng.integers(0, bw - mw + 1)), y0 + int(rng.integers(0, bh - mh + 1))
            members.append(len(cc_boxes))
            cc_boxes.append((mx, mx + mw - 1, my, my + mh - 1))
            cc_images.append(((rng.random((mh, mw)) < 0.7) * 255).astype(np.uint8))
            first = int(rng.integers(0, n))
            cc_life.append((first, int(rng.integers(first, n))))
        groups.append(members)
        t0 = int(rng.integers(0, n))
        ages[g] = sorted({t0, int(rng.integers(t0, n)), int(rng.integers(t0, n))}) if g % 5 else [0, n - 1]
    hist = device.FrameHistory.from_frames(frames, lib)
    masks = device.GroupImages.from_host(cc_boxes, cc_images, w, h, lib)
    try:
        for thr in THRESHOLDS + [30.2]:
            want, bounds, maxima = numpy_raw_images(cc_boxes, cc_images, cc_life, groups, ages, frames, thr)
            boxes = [bounds[g] for g in want for _ in want[g]]
            ranges = [(ages[g][k], ages[g][k + 1]) for g in want for k in range(len(want[g]))]
            lists = [[c for c in groups[g] if cc_life[c][0] <= t1 and t0 <= cc_life[c][1]] for g in want for t0, t1 in zip(ages[g][:-1], ages[g][1:])]
            gi, got_max = hist.masked_images(masks, boxes, ranges, lists, thr)
            flat = [im for g in want for im in want[g]]
            assert len(gi) == len(flat) > 60 and got_max.tolist() == [m for g in want for m in maxima[g]]
            assert any(len(lst) == 0 for lst in lists) and any(len(lst) > 1 for lst in lists)
            for i, im in enumerate(flat):
                assert (gi.image(i) == im).all(), (thr, i)
            gi.close()
        # mask items that reach beyond the job's box on every side are clipped to it
        big_boxes = [(0, w - 1, 0, h - 1), (30, 100, 3, 30)]
        big_images = [((rng.random((h, w)) < 0.5) * 255).astype(np.uint8), ((rng.random((28, 71)) < 0.5) * 255).astype(np.uint8)]
        canvas = big_images[0] > 0
        canvas[3:31, 30:101] |= big_images[1] > 0
        big = device.GroupImages.from_host(big_boxes, big_images, w, h, lib)
        boxes = [(31, 31, 5, 5), (33, 97, 4, 29), (5, 70, 0, h - 1), (64, 95, 10, 12), (0, w - 1, 0, h - 1), (95, w - 1, 29, h - 1)]
        gi, got_max = hist.masked_images(big, boxes, [(2, 30)] * len(boxes), [[0, 1]] * len(boxes), 100)
        for i, (x0, x1, y0, y1) in enumerate(boxes):
            count = ((frames[2:31, y0:y1 + 1, x0:x1 + 1] == 255) & canvas[y0:y1 + 1, x0:x1 + 1]).sum(axis=0, dtype=np.int64)
            assert int(got_max[i]) == int(count.max()) > 0
            assert (gi.image(i) == (((count * 255) // count.max()) > 100) * 255).all(), i
        gi.close()
        big.close()
    finally:
        masks.close()
        hist.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    from lecturemath_amd import _lib, device
    h, w, n = 10, 50, 12
    frames = random_frames(n, h, w, 3)
    hist = device.FrameHistory(w, h, n + 2, lib)
    masks = device.GroupImages.from_host([(0, 3, 0, 1)], [np.full((2, 4), 255, np.uint8)], w, h, lib)

    def refused(call, *args, **kw):
        try:
            call(*args, **kw)
        except ValueError:
            pass
        else:
            raise AssertionError("no ValueError")
        assert len(hist) == n

    def usable():
        total, age = hist.segment_stats(0, n - 1, host=True)
        assert (total == numpy_extract(frames, [(0, n - 1)], 1)[0]["sum"]).all()
        gi, maxima = hist.masked_images(masks, [(0, 3, 0, 1)], [(0, n - 1)], [[0]], 0)
        assert maxima.tolist() == [int((frames[:, 0:2, 0:4] == 255).sum(axis=0).max())]
        gi.close()

    try:
        hist.append(frames)
        usable()
        bad = frames[:2].copy()
        bad[1, 9, 49] = 7
        refused(hist.append, bad)                                           # a byte that is neither 0 nor 255
        refused(hist.append, [bad[0], bad[1]])
        refused(hist.append, np.zeros((1, h, w + 1), np.uint8))             # wrong shapes
        refused(hist.append, np.zeros((h, w), np.uint8))
        refused(hist.append, [np.zeros((h + 1, w), np.uint8)])
        refused(hist.append, np.zeros((3, h, w), np.uint8))                 # past capacity (12 + 3 > 14)
        refused(hist.segment_stats, 0, n)                                   # t1 >= len
        refused(hist.segment_stats, 5, 4)                                   # t0 > t1
        refused(hist.segment_stats, -1, 4)
        refused(hist.segment_stats, 0, 65535)                               # 65,536 frames against a short history: the length check fires
        refused(hist.masked_images, masks, [(0, 3, 0, 1)], [(0, n)], [[0]], 0)
        refused(hist.masked_images, masks, [(0, 3, 0, 1)], [(3, 2)], [[0]], 0)
        refused(hist.masked_images, masks, [(0, 3, 0, 1)], [(0, 65535)], [[0]], 0)
        refused(hist.masked_images, masks, [(0, w, 0, 1)], [(0, 1)], [[0]], 0)      # boxes outside the frame
        refused(hist.masked_images, masks, [(0, 3, 0, h)], [(0, 1)], [[0]], 0)
        refused(hist.masked_images, masks, [(-1, 3, 0, 1)], [(0, 1)], [[0]], 0)
        refused(hist.masked_images, masks, [(4, 3, 0, 1)], [(0, 1)], [[0]], 0)
        refused(hist.masked_images, masks, [(0, 3, 0, 1)], [(0, 1)], [[1]], 0)      # a mask item outside the table
        refused(hist.masked_images, masks, [(0, 3, 0, 1)], [(0, 1)], [[0]], float("nan"))
        usable()
        # the C ABI itself answers the same way
        st = hist.be.stream()
        box, rng_, off, item = np.asarray([0, 3, 0, 1], np.int32), np.asarray([0, n], np.int32), np.asarray([0, 1], np.int64), np.asarray([0], np.int32)
        assert not lib.lm_hist_masked_images(hist.handle, masks.handle, box.ctypes.data, rng_.ctypes.data, off.ctypes.data, item.ctypes.data, 1, 0.0, None, st)
        assert "lm_hist_masked_images" in lib.last_error()
        dev = hist.be.from_host(np.zeros((3, h, w), np.uint8))
        assert lib.lm_hist_append(hist.handle, _lib.ptr(dev), 3, st) == _lib.LM_ERR_CAPACITY
        both = hist.be.empty((2, h, w), np.float32)
        assert lib.lm_hist_segment_stats(hist.handle, 0, n, _lib.ptr(both[0]), _lib.ptr(both[1]), st) == _lib.LM_ERR_ARG
        assert lib.lm_hist_count(None) == -1 and lib.lm_hist_truncate(hist.handle, n + 1) == _lib.LM_ERR_ARG
        lib.lm_hist_destroy(None)
        hist.append(frames[:2])                                             # room for two more
        assert len(hist) == n + 2 and (hist.frame(n + 1) == frames[1]).all()
    finally:
        hist.close()
        masks.close()
    for call in (lambda: len(hist), lambda: hist.segment_stats(0, 1), lambda: pickle.dumps(hist)):
        try:
            call()
        except (ValueError, TypeError):
            pass
        else:
            raise AssertionError("no exception")
    for args in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (40000, 4, 1)):
        try:
            device.FrameHistory(*args, lib=lib)
        except (_lib.LecturemathError, ValueError):
            pass
        else:
            raise AssertionError("no exception")
