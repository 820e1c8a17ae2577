#!/usr/bin/env python3
"""G20 (g20_step04_sums.npz): step 04 with VIDEO_SEGMENTATION_METHOD = 1 (sums + regression tree) of the reference, run in THIS
container.  The tree is sklearn's: the fixture was recorded with scikit-learn 1.7.2 (numpy 1.x float64), which is what
DecisionTreeRegressor(max_depth=None, min_samples_leaf=leaf_min) on x = arange(n) runs as here; the version that wrote the file is
stored in it (`sklearn_version`).

(a) The three golden streams: the reference's own step-03 calls reconstruct the frames (PNG files, as in make_golden_step04.py), then
    the reference's pre_ST3D_v3.0_04_vid_segmentation.process_input runs unmodified (matplotlib is a no-op stand-in) with the input
    of method 1, the (frame_times, frame_indices, compressed_frames) triple itself, for the parameter sets PARAM_SETS -- minimum
    segments small enough that every stream splits.  Stored per stream and set: the sums, everything printed, the returned intervals.
(b) 400 random signals, 100 of each of four kinds (integer sums; integer ramps with erasures; S / 255 with S no multiple of 255;
    plateaus of 20 equal values), n in 5 .. 600, leaf_min in 1 .. 40, several min_erase, through the reference's
    VideoSegmenter.video_segments_from_sums and get_tree_decision_boundaries.  Stored per case: the signal as the integers S with
    y = S / divisor (divisor 1 or 255: the float64 division is the one the test repeats), the parameters, interval_idxs,
    interval_vals (bit patterns) and the segments; and, read off sklearn's fitted tree, what keeps the fixture from being vacuous:
      short_node   a node with leaf_min > m - leaf_min (m its samples)
      backward     a split node whose winning left part is longer than its right part: the left sum of the winning split is taken
                   from the far end, over the rotated right part
      rot_leaf     a right child that is a leaf of three or more samples with non-integer values
      rot_shows    ... whose prediction differs in bits from the sum of its samples in frame order divided by their number
"""
import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_env  # noqa: E402
from lecturemath_amd import synth  # noqa: E402

ref_env.enter()
import sklearn  # noqa: E402
from AccessMath.preprocessing.content.cc_stability_estimator import CCStabilityEstimator  # noqa: E402
from AccessMath.preprocessing.content.video_segmenter import VideoSegmenter  # noqa: E402

spec04 = importlib.util.spec_from_file_location("ref_step04", os.path.join(ref_env.REF_ROOT, "pre_ST3D_v3.0_04_vid_segmentation.py"))
ref_step04 = importlib.util.module_from_spec(spec04)
spec04.loader.exec_module(ref_step04)

K = "VIDEO_SEGMENTATION_SUM_"
PARAM_SETS = [
    {"SAMPLING_FPS": 1.0, K + "MIN_SEGMENT": 3, K + "MIN_ERASE_RATIO": 0.05},
    {"SAMPLING_FPS": 0.5, K + "MIN_SEGMENT": 3, K + "MIN_ERASE_RATIO": 0.0},         # leaf_min = ceil(1.5) = 2
    {"SAMPLING_FPS": 2.0, K + "MIN_SEGMENT": 3, K + "MIN_ERASE_RATIO": 0.2},
]
STREAMS = ("accumulate_erase", "occluder_return", "short_gap_jitter")
KINDS = ("integer sums", "integer ramps with erasures", "S / 255", "plateaus of 20")
CASES_PER_KIND = 100


class _Conf:
    def __init__(self, values):
        self.values = dict(values, VIDEO_SEGMENTATION_METHOD=1)

    def get_int(self, key, default=None):
        return int(self.values.get(key, default))

    def get_float(self, key, default=None):
        return float(self.values.get(key, default))

    def get(self, key, default=None):
        return self.values.get(key, default)


class _Lecture:
    title = "golden"


class _Process:
    def __init__(self, values):
        self.configuration = _Conf(values)
        self.img_dir = "."
        self.current_lecture = _Lecture()
        self.params = {}


def bits(values):
    return np.asarray(values, np.float64).view(np.int64)


def make_stream(name, out):
    g = np.load(os.path.join(HERE, "g3_stream_%s.npz" % name))
    spec = json.loads(bytes(g["spec"]).decode())
    h, w = spec["h"], spec["w"]
    frames = list(synth.binary_stream(spec["n"], h, w, **spec["gen"]))
    est = CCStabilityEstimator(w, h, 0.85, 0.85, spec["gap2"], False)
    for f in frames:
        est.add_frame(f, True)
    with contextlib.redirect_stdout(io.StringIO()):
        est.split_stable_cc_by_gaps(spec["gap3"], 3)
        stable = est.get_stable_cc_idxs(3)
        tov, total, aov = est.compute_overlapping_stable_cc(stable, 5)
        groups, gid = est.compute_groups(stable, tov, 0.5, None, None)
        ages, gpf = est.compute_groups_temporal_information(groups)
        gimg, gb = est.compute_group_images(groups, ages, 0.5)
        clean = est.frames_from_groups(groups, gb, gpf, ages, gimg, None, 3, True)
    n = len(frames)
    frame_times, frame_indices = [float(i) for i in range(n)], list(range(n))
    from AccessMath.preprocessing.content.helper import Helper
    sums = VideoSegmenter.compute_binary_sums(Helper.decompress_binary_images(clean))
    out["%s.sums" % name] = bits(sums)
    for k, values in enumerate(PARAM_SETS):
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            intervals = ref_step04.process_input(_Process(values), (frame_times, frame_indices, clean))
        out["%s.intervals_%d" % (name, k)] = np.asarray(intervals, np.int64).reshape(-1, 2)
        out["%s.printed_%d" % (name, k)] = np.frombuffer(text.getvalue().encode(), np.uint8)
        print(name, "params", k, "->", [tuple(int(v) for v in iv) for iv in intervals])


# ---- (b) random signals --------------------------------------------------------------------------------------------------------
def random_signal(rng, kind):
    """-> (S int64 [n], divisor): a board that fills and is erased now and then"""
    n = int(rng.integers(5, 601))
    level, values = int(rng.integers(0, 40000)), []
    while len(values) < n:
        length = int(rng.integers(3, 160))
        step = int(rng.integers(0, 900))
        for _ in range(length):
            level += int(rng.integers(0, step + 1))
            values.append(level)
        if rng.random() < 0.8:
            level = int(level * rng.choice([0.0, 0.1, 0.5, 0.9, 0.97]))           # an erasure, from complete to hardly any
    S = np.asarray(values[:n], np.int64)
    if kind == 0:                   # integer sums: ink counts with the frame-to-frame noise of a binarizer
        return np.maximum(S + rng.integers(-300, 301, n), 0), 1
    if kind == 1:                   # integer ramps with erasures, clean
        return S, 1
    if kind == 2:                   # sums of frames that hold other values than 0 and 255 (images added on top of each other)
        S = S * 255 + rng.integers(1, 255, n)
        return S, 255
    S = np.repeat(S[::20] * 255 + rng.integers(1, 255, len(S[::20])), 20)[:n]        # plateaus of 20 equal, non-integer values
    return S, 255


def tree_facts(tree, y, leaf_min):
    t = tree.tree_
    left, right, m = t.children_left, t.children_right, t.n_node_samples
    short_node = bool((leaf_min > m - leaf_min).any())
    split = np.flatnonzero(left >= 0)
    backward = bool((m[left[split]] > m[right[split]]).any())
    rot_leaf = rot_shows = False
    # first frame of every node: the root starts at 0, a left child where its parent does, a right child behind the left one
    start = np.zeros(len(m), np.int64)
    for node in split:              # parents come before their children (depth-first numbering)
        start[left[node]] = start[node]
        start[right[node]] = start[node] + m[left[node]]
    for node in split:
        r = right[node]
        if left[r] < 0 and m[r] >= 3:
            ys = y[start[r]:start[r] + m[r]]
            if (ys != np.floor(ys)).any():
                rot_leaf = True
                if np.float64(np.cumsum(ys)[-1] / m[r]).view(np.int64) != np.float64(t.value[r, 0, 0]).view(np.int64):
                    rot_shows = True
    return short_node, backward, rot_leaf, rot_shows


def make_cases(out):
    rng = np.random.default_rng(2004)
    acc = {k: [] for k in ("kind", "n", "divisor", "leaf_min", "min_erase", "S", "idx_off", "interval_idxs", "interval_vals", "seg_off",
                           "segments", "short_node", "backward", "rot_leaf", "rot_shows")}
    for case in range(CASES_PER_KIND * len(KINDS)):
        kind = case % len(KINDS)
        S, divisor = random_signal(rng, kind)
        y = S / divisor if divisor != 1 else S.astype(np.float64)
        leaf_min = int(rng.integers(1, 41))
        min_erase = float(rng.choice([0.0, 0.01, 0.05, 0.2]))
        all_sums = list(y)
        with np.errstate(all="ignore"):
            segments = VideoSegmenter.video_segments_from_sums(all_sums, leaf_min, min_erase)
        tree = VideoSegmenter.create_regresor_from_sums(all_sums, leaf_min)
        interval_idxs, interval_vals = VideoSegmenter.get_tree_decision_boundaries(tree, len(all_sums))
        facts = tree_facts(tree, y, leaf_min)
        acc["kind"].append(kind)
        acc["n"].append(len(S))
        acc["divisor"].append(divisor)
        acc["leaf_min"].append(leaf_min)
        acc["min_erase"].append(min_erase)
        acc["S"].extend(S.tolist())
        acc["idx_off"].append(len(interval_idxs))
        acc["interval_idxs"].extend(interval_idxs)
        acc["interval_vals"].extend(bits(interval_vals).tolist())
        acc["seg_off"].append(len(segments))
        acc["segments"].extend(segments)
        for key, v in zip(("short_node", "backward", "rot_leaf", "rot_shows"), facts):
            acc[key].append(v)
    out.update({"n_cases": np.int64(len(acc["n"])), "kind": np.asarray(acc["kind"], np.int8), "n": np.asarray(acc["n"], np.int32),
                "divisor": np.asarray(acc["divisor"], np.int32), "leaf_min": np.asarray(acc["leaf_min"], np.int32),
                "min_erase": np.asarray(acc["min_erase"], np.float64), "S": np.asarray(acc["S"], np.int64),
                "interval_idxs": np.asarray(acc["interval_idxs"], np.int32), "interval_vals": np.asarray(acc["interval_vals"], np.int64),
                "segments": np.asarray(acc["segments"], np.int32).reshape(-1, 2)})
    for key in ("short_node", "backward", "rot_leaf", "rot_shows"):
        out[key] = np.asarray(acc[key], np.bool_)
    out["y_off"] = np.concatenate([[0], np.cumsum(acc["n"])]).astype(np.int64)
    for key in ("idx_off", "seg_off"):
        out[key] = np.concatenate([[0], np.cumsum(acc[key])]).astype(np.int64)
    check_not_vacuous(out)


def check_not_vacuous(g):
    """The conditions that keep the fixture from being vacuous (tests/test_step04_sums_emulated.py re-asserts them)."""
    n = int(g["n_cases"])
    n_seg = np.diff(g["seg_off"])
    print("g20: %d cases; %.0f %% give two or more segments; short node %d, backward %d, rotated leaf %d (shows in %d)" % (
        n, 100 * (n_seg >= 2).mean(), g["short_node"].sum(), g["backward"].sum(), g["rot_leaf"].sum(), g["rot_shows"].sum()))
    assert n >= 300 and all((g["kind"] == k).sum() >= 50 for k in range(len(KINDS)))
    assert (n_seg >= 2).mean() >= 0.5
    assert g["short_node"].sum() >= 20 and g["backward"].sum() >= 20
    assert g["rot_leaf"].sum() >= 20 and g["rot_shows"].sum() >= 20


if __name__ == "__main__":
    out = {"sklearn_version": np.frombuffer(sklearn.__version__.encode(), np.uint8),
           "params": np.frombuffer(json.dumps(PARAM_SETS).encode(), np.uint8)}
    for nm in STREAMS:
        make_stream(nm, out)
    make_cases(out)
    path = os.path.join(HERE, "g20_step04_sums.npz")
    np.savez_compressed(path, **out)
    print("g20:", os.path.getsize(path), "bytes")
