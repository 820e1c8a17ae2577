#!/usr/bin/env python3
"""G23: the pixel-history methods of the reference, run unmodified in THIS container:
CCStabilityEstimator.compute_group_images_from_raw_binary (cc_stability_estimator.py:502-573) and KeyframeExtractor.extract
(keyframe_extractor.py:146-222), on the three golden streams and on three synthetic cases driven through a bare estimator
(CCStabilityEstimator.__new__ with hand-set unique_cc_objects / unique_cc_frames).  tests/history_checks.py documents the layout.
numpy >= 1.24 lacks np.bool, which the reference still uses: aliased to bool here (environment stand-in).  The reference does not
return an image's maximum count: the stored maxima are those of history_checks.numpy_raw_images, asserted equal to the reference
image by image first."""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_env  # noqa: E402
import history_checks as hc  # noqa: E402
from lecturemath_amd import synth  # noqa: E402

ref_env.enter()
if not hasattr(np, "bool"):
    np.bool = bool
from AccessMath.preprocessing.content.cc_stability_estimator import CCStabilityEstimator  # noqa: E402
from AccessMath.preprocessing.content.keyframe_extractor import KeyframeExtractor  # noqa: E402
from AccessMath.data.space_time_struct import SpaceTimeStruct  # noqa: E402


class BareCC:
    """what compute_group_images_from_raw_binary reads of a ConnectedComponent"""

    def __init__(self, box, img):
        self.min_x, self.max_x, self.min_y, self.max_y = box
        self.img = img

    def getWidth(self):
        return self.max_x - self.min_x + 1

    def getHeight(self):
        return self.max_y - self.min_y + 1


def pack_images(images):
    return np.packbits(np.concatenate([np.asarray(im).ravel() > 0 for im in images])) if images else np.zeros(0, np.uint8)


def store_case(out, prefix, est, groups, ages, frames, thresholds, meta):
    """runs the reference method at every threshold and stores inputs and results; groups name unique CCs of `est`"""
    used = sorted({int(c) for group in groups for c in group})
    slot = {c: i for i, c in enumerate(used)}
    cc_boxes = [(int(est.unique_cc_objects[c].min_x), int(est.unique_cc_objects[c].max_x), int(est.unique_cc_objects[c].min_y),
                 int(est.unique_cc_objects[c].max_y)) for c in used]
    cc_images = [np.asarray(est.unique_cc_objects[c].img) for c in used]
    assert all(set(np.unique(im)) <= {0, 255} for im in cc_images)
    cc_life = [(int(est.unique_cc_frames[c][0][0]), int(est.unique_cc_frames[c][-1][0])) for c in used]
    compact = [[slot[int(c)] for c in group] for group in groups]
    ages = {k: [int(a) for a in ages[k]] for k in range(len(groups))}
    out[prefix + "cc_boxes"] = np.asarray(cc_boxes, np.int32).reshape(-1, 4)
    out[prefix + "cc_images"] = pack_images(cc_images)
    out[prefix + "cc_life"] = np.asarray(cc_life, np.int32).reshape(-1, 2)
    out[prefix + "groups"] = np.asarray([c for group in compact for c in group], np.int32)
    out[prefix + "groups_off"] = np.cumsum([0] + [len(group) for group in compact]).astype(np.int64)
    out[prefix + "ages"] = np.asarray([a for k in ages for a in ages[k]], np.int32)
    out[prefix + "ages_off"] = np.cumsum([0] + [len(ages[k]) for k in ages]).astype(np.int64)
    keys = None
    for ti, thr in enumerate(thresholds):
        with np.errstate(all="ignore"):
            images, bounds = est.compute_group_images_from_raw_binary(groups, ages, frames, thr)
        want, wbounds, maxima = hc.numpy_raw_images(cc_boxes, cc_images, cc_life, compact, ages, frames, thr)
        assert list(images) == list(want) and {k: tuple(int(v) for v in b) for k, b in bounds.items()} == wbounds
        for k in images:
            assert len(images[k]) == len(want[k]) == len(ages[k]) - 1
            assert all(a.dtype == np.uint8 and a.shape == b.shape and (a == b).all() for a, b in zip(images[k], want[k])), (prefix, thr, k)
        keys = list(images)
        out[prefix + "raw_%d" % ti] = pack_images([im for k in keys for im in images[k]])
        out[prefix + "raw_max"] = np.asarray([m for k in keys for m in maxima[k]], np.int64)
        out[prefix + "bound_groups"] = np.asarray(keys, np.int32)
        out[prefix + "bounds"] = np.asarray([wbounds[k] for k in keys], np.int32).reshape(-1, 4)
        print(prefix or meta["name"], "threshold", thr, "images", sum(len(v) for v in images.values()), "non-empty",
              sum(int(im.any()) for v in images.values() for im in v), "largest maximum", max(m for k in keys for m in maxima[k]))
    meta = dict(meta, thresholds=thresholds)
    return meta, images


def store_extract(out, prefix, frames, segment_sets, lengths, meta):
    n, w = len(frames), frames[0].shape[1]
    as_list = list(frames)
    for si, segs in enumerate(segment_sets):
        for li, lname in enumerate(lengths):
            res = KeyframeExtractor.extract(as_list, segs, hc.length_value(lname, n))
            assert [(r["start"], r["end"]) for r in res] == [tuple(sg) for sg in segs]
            total, age = np.stack([r["sum"] for r in res]), np.stack([r["age"] for r in res])
            assert total.dtype == np.float32 and age.dtype == np.float32 and (total == np.round(total)).all() and total.max() < 65536
            if li == 0:
                out[prefix + "sum_%d" % si] = total.astype(np.uint16)
                out[prefix + "age_%d" % si] = age.astype(np.int32)
                assert (out[prefix + "age_%d" % si] == age).all()
            else:
                assert (out[prefix + "sum_%d" % si] == total).all() and (out[prefix + "age_%d" % si] == age).all()
            out[prefix + "filtered_%d_%d" % (si, li)] = np.packbits(np.stack([r["filtered"] for r in res]) == 255, axis=2)
            out[prefix + "local_max_%d_%d" % (si, li)] = np.asarray([[i for i, f in enumerate(as_list) if f is r["local_max"]][0] for r in res], np.int32)
            want = hc.numpy_extract(frames, segs, hc.length_value(lname, n))
            assert all((a["sum"] == b["sum"]).all() and (a["age"] == b["age"]).all() and (a["filtered"] == b["filtered"]).all() and
                       as_list[b["local_max"]] is a["local_max"] for a, b in zip(res, want))
    return dict(meta, segment_sets=[[list(sg) for sg in segs] for segs in segment_sets], treshold_lengths=lengths, w=w)


def make_stream(name):
    g = np.load(os.path.join(HERE, "g3_stream_%s.npz" % name))
    g7 = np.load(os.path.join(HERE, "g7_step04_%s.npz" % name))
    spec = json.loads(bytes(g["spec"]).decode())
    h, w = spec["h"], spec["w"]
    frames = np.stack(list(synth.binary_stream(spec["n"], h, w, **spec["gen"])))
    est = CCStabilityEstimator(w, h, 0.85, 0.85, spec["gap2"], False)
    for f in frames:
        est.add_frame(f, True)
    with contextlib.redirect_stdout(io.StringIO()):
        est.split_stable_cc_by_gaps(spec["gap3"], 3)
        stable = est.get_stable_cc_idxs(3)
        tov, total, aov = est.compute_overlapping_stable_cc(stable, 5)
        groups, gid = est.compute_groups(stable, tov, 0.5, None, None)
        ages, gpf = est.compute_groups_temporal_information(groups)
        crop_images, _ = est.compute_group_images(groups, ages, 0.5)
    n = len(frames)
    out = {}
    meta, _ = store_case(out, "", est, groups, ages, list(frames), hc.THRESHOLDS, {"name": name, "h": h, "w": w, "n": n})
    with np.errstate(all="ignore"):
        images, bounds = est.compute_group_images_from_raw_binary(groups, ages, list(frames), 127)
    differ = sum(int((a != b).any()) for k in images for a, b in zip(images[k], crop_images[k]))
    print(name, "raw-binary images at 127 that differ from compute_group_images(0.5):", differ, "of", sum(len(v) for v in images.values()))
    meta = store_extract(out, "x_", frames, [[(0, n - 1)], [(0, n // 3), (n // 3 + 1, n - 1)], [(n // 2, n // 2)]], hc.TRESHOLD_LENGTHS, meta)
    segs = [tuple(int(v) for v in iv) for iv in g7["intervals_2"]]
    st3d = SpaceTimeStruct([1000.0 * i for i in range(n)], list(range(n)), est.height, est.width, ages, images, bounds)
    with contextlib.redirect_stdout(io.StringIO()):
        keyframes, cc_times = KeyframeExtractor.GenerateFromST3DForIntervals(st3d, segs, False)
    kf = np.stack(keyframes)
    assert set(np.unique(kf)) <= {0, 255} and (kf[..., 0] == kf[..., 1]).all() and (kf[..., 0] == kf[..., 2]).all()
    out["keyframes05"] = np.packbits(kf[..., 0] == 255, axis=2)
    out["times05"] = np.asarray([(s, *t) for s, lst in enumerate(cc_times) for t in lst], np.float64).reshape(-1, 6)
    meta["segments05"] = [list(sg) for sg in segs]
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(os.path.join(HERE, "g23_history_%s.npz" % name), **out)


def bare(ccs, lives):
    est = CCStabilityEstimator.__new__(CCStabilityEstimator)
    est.unique_cc_objects = [BareCC(box, img) for box, img in ccs]
    est.unique_cc_frames = [[(first, 1), (last, 1)] for first, last in lives]
    return est


def random_cc(rng, box, p=0.7):
    return box, ((rng.random((box[3] - box[2] + 1, box[1] - box[0] + 1)) < p) * 255).astype(np.uint8)


def make_synthetic():
    out = {}
    rng = np.random.default_rng(23)
    # long: counts cross 255 / 256
    h, w, n = 24, 70, 300
    frames = ((rng.random((n, h, w)) < 0.9) * 255).astype(np.uint8)
    frames[:, 3, 30:36] = 255
    ccs = [random_cc(rng, (2, 66, 1, 20)), random_cc(rng, (40, 69, 10, 23)), random_cc(rng, (0, 33, 0, 23), 0.9)]
    lives = [(0, 299), (0, 299), (0, 299)]
    meta, _ = store_case(out, "long_", bare(ccs, lives), [[0, 1], [2]], {0: [0, 256], 1: [257, 299]}, list(frames), hc.THRESHOLDS,
                         {"name": "long", "h": h, "w": w, "n": n})
    meta = store_extract(out, "long_x_", frames, [[(0, 256), (257, 299)]], ["1", "256", "n+1"], meta)
    out["long_frames"] = np.packbits(frames == 255, axis=2)
    out["long_meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    # wide: W % 32 == 12, boxes around the word boundaries and at the frame's edges
    h, w, n = 40, 1100, 12
    frames = ((rng.random((n, h, w)) < 0.5) * 255).astype(np.uint8)
    ccs = [random_cc(rng, (13, 600, 2, 30)), random_cc(rng, (500, 1067, 5, 37)), random_cc(rng, (550, 560, 0, 39), 1.0),
           random_cc(rng, (31, 31, 0, 5), 1.0), random_cc(rng, (63, 64, 7, 9), 1.0), random_cc(rng, (95, 127, 11, 12)),
           random_cc(rng, (1080, 1099, 30, 39)), random_cc(rng, (1090, 1099, 35, 39), 0.5), random_cc(rng, (0, 1099, 20, 20))]
    lives = [(0, 4), (3, 11), (0, 11), (0, 11), (0, 11), (2, 9), (0, 11), (6, 11), (0, 11)]
    groups = [[0, 1, 2], [3], [4], [5], [6, 7], [8]]
    ages = {0: [0, 5, 11], 1: [0, 11], 2: [1, 2, 10], 3: [2, 9], 4: [0, 5, 6, 11], 5: [4, 4]}
    meta, _ = store_case(out, "wide_", bare(ccs, lives), groups, ages, list(frames), hc.THRESHOLDS, {"name": "wide", "h": h, "w": w, "n": n})
    out["wide_frames"] = np.packbits(frames == 255, axis=2)
    out["wide_meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    # stranger: nothing is ever ink
    h, w, n = 16, 40, 5
    frames = np.zeros((n, h, w), np.uint8)
    ccs = [random_cc(rng, (3, 37, 2, 12))]
    meta, _ = store_case(out, "stranger_", bare(ccs, [(0, 4)]), [[0]], {0: [0, 2, 4]}, list(frames), [0, -1], {"name": "stranger", "h": h, "w": w, "n": n})
    out["stranger_frames"] = np.packbits(frames == 255, axis=2)
    out["stranger_meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(os.path.join(HERE, "g23_history_synthetic.npz"), **out)


if __name__ == "__main__":
    make_synthetic()
    for nm in ("accumulate_erase", "occluder_return", "short_gap_jitter"):
        make_stream(nm)
