#!/usr/bin/env python3
"""G17 / G18: step 04 with VIDEO_SEGMENTATION_METHOD = 2 (conflict minimisation) of the reference, run in THIS container.

G17 (g17_step04_conflicts_<stream>.npz), for the three golden streams: the reference's own step-03 calls build (group_ages,
conflicts) as in make_golden_step04.py, then the reference's pre_ST3D_v3.0_04_vid_segmentation.process_input runs unmodified
(matplotlib is a no-op stand-in) for six parameter sets: the script's defaults, the shipped configuration and four sensitive sets
with small minimum lengths that use every weight constant once.  Stored per set: intervals, everything printed, the conflict
signal of the whole stream (depth 0) as int64 bit patterns, and what from_group_conflicts_with_presegments returns for the
pre-segments method 3 found (G7, parameter set 2).

G18 (g18_conflict_cases.npz): 960 random (n_frames, group_ages, conflicts) structures, each run through the reference's
VideoSegmenter.split_video_from_group_conflicts with one parameter tuple, 20 per combination of the 4 x 4 x 3 weight modes.  Stored
per case: the inputs with the insertion orders of the dicts as explicit lists (`group_order`: the keys of group_ages; `rows`: (group,
other) of every inner-dict entry in insertion order, its four numbers in `pairs` [6][n] = group < other, matched, unmatched, area_union,
area_intersection), intervals, printed text, split_data, the depth-0
signal as int64 bit patterns and whether that signal changes when the inner dicts are re-sorted.
"""
import contextlib
import copy
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
import cv2  # noqa: E402  (the stand-in)
from AccessMath.preprocessing.content.cc_stability_estimator import CCStabilityEstimator  # noqa: E402
from AccessMath.preprocessing.content.video_segmenter import VideoSegmenter  # noqa: E402

spec04 = importlib.util.spec_from_file_location("ref_step04", os.path.join(ref_env.REF_ROOT, "pre_ST3D_v3.0_04_vid_segmentation.py"))
ref_step04 = importlib.util.module_from_spec(spec04)
spec04.loader.exec_module(ref_step04)

K = "VIDEO_SEGMENTATION_CONFLICTS_"


def params(w, p, t, min_conflicts, min_split, min_len):
    return {K + "WEIGHTS": w, K + "WEIGHTS_PIXELS": p, K + "WEIGHTS_TIME": t, K + "MIN_CONFLICTS": min_conflicts,
            K + "MIN_SPLIT": min_split, K + "MIN_LENGTH": min_len}


PARAM_SETS = [
    params(0, 0, 0, 3.0, 50, 25),           # the script's defaults (04_vid_segmentation.py:122-136)
    params(3, 3, 1, 0.03, 20, 15),          # configs/FCN_LectureNet.conf:189-210
    params(4, 1, 2, 0.0, 6, 3),             # four sensitive sets: every area / pixel / time constant once
    params(5, 2, 1, 0.01, 4, 2),
    params(0, 3, 0, 0.5, 6, 3),
    params(3, 0, 2, 0.0, 2, 1),
]


class _Conf:
    def __init__(self, values):
        self.values = dict(values, VIDEO_SEGMENTATION_METHOD=2)

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


def root_signal(n_frames, ages, conf, w, p, t):
    """conflicts_per_frame of the whole stream: the reference's function with a minimum length no split can meet"""
    graph = []
    with contextlib.redirect_stdout(io.StringIO()):
        VideoSegmenter.split_video_from_group_conflicts(0, n_frames - 1, ages, conf, 0.0, 0, n_frames + 1, w, p, t, 0, graph, [], n_frames)
    return bits([graph[0][1][f] for f in range(n_frames)])


def make_stream(name):
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
        conf = est.compute_conflicting_groups(stable, aov, len(groups), gid)
        gimg, gb = est.compute_group_images(groups, ages, 0.5)
        clean = est.frames_from_groups(groups, gb, gpf, ages, gimg, None, 3, True)
    n = len(frames)
    frame_times, frame_indices = [float(i) for i in range(n)], list(range(n))
    pre_segments = [tuple(int(v) for v in iv) for iv in np.load(os.path.join(HERE, "g7_step04_%s.npz" % name))["intervals_2"]]
    out = {"name": np.frombuffer(name.encode(), np.uint8), "n_frames": np.int64(n),
           "params": np.frombuffer(json.dumps(PARAM_SETS).encode(), np.uint8), "pre_segments": np.asarray(pre_segments, np.int64).reshape(-1, 2)}
    for k, values in enumerate(PARAM_SETS):
        mine = copy.deepcopy(conf)                      # the reference normalises the areas in place
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            intervals = ref_step04.process_input(_Process(values), [(frame_times, frame_indices, clean), (ages, mine)])
        out["intervals_%d" % k] = np.asarray(intervals, np.int64).reshape(-1, 2)
        out["printed_%d" % k] = np.frombuffer(text.getvalue().encode(), np.uint8)
        wa, wp, wt = values[K + "WEIGHTS"], values[K + "WEIGHTS_PIXELS"], values[K + "WEIGHTS_TIME"]
        rest = (values[K + "MIN_CONFLICTS"], values[K + "MIN_SPLIT"], values[K + "MIN_LENGTH"], wa, wp, wt)
        out["signal0_%d" % k] = root_signal(n, ages, mine, wa, wp, wt)          # `mine` carries the script's normalisation
        with contextlib.redirect_stdout(io.StringIO()):
            together = VideoSegmenter.from_group_conflicts_with_presegments(n, pre_segments, ages, mine, *rest)
            apart = [iv for seg in pre_segments for iv in
                     VideoSegmenter.split_video_from_group_conflicts(seg[0], seg[1], ages, mine, *rest, 0, [], [], n)]
        assert together == apart
        out["preseg_intervals_%d" % k] = np.asarray(together, np.int64).reshape(-1, 2)
        print(name, "params", k, "->", [tuple(int(v) for v in iv) for iv in intervals], "| pre-segmented:", len(together))
    np.savez_compressed(os.path.join(HERE, "g17_step04_conflicts_%s.npz" % name), **out)


# ---- G18 ---------------------------------------------------------------------------------------------------------------------
COMBOS = [(a, p, t) for a in (0, 3, 4, 5) for p in (0, 1, 2, 3) for t in (0, 1, 2)]
CASES_PER_COMBO = 20


def non_integer_weights(combo):
    return combo[0] == 5 or combo[1] == 3 or combo[2] == 2


def random_case(rng, combo):
    n_frames = int(rng.integers(1, 300))
    n_groups = int(rng.integers(0, 40))
    spans = []
    for _ in range(n_groups):
        first = int(rng.integers(0, n_frames))
        spans.append((first, min(n_frames - 1, first + int(rng.integers(0, 81)))))
    inner = {g: [] for g in range(n_groups)}
    for a in range(n_groups):
        for b in range(a + 1, n_groups):
            if rng.random() < 0.25:
                inter = int(rng.integers(1, 4000))
                d = (int(rng.integers(0, 500)), int(rng.integers(1, 500)), inter + int(rng.integers(0, 8000)), inter)
                inner[a].append((b, d))
                inner[b].append((a, d))
    group_order = [int(g) for g in rng.permutation(n_groups)]
    rows = []                                            # (group, other, matched, unmatched, area_union, area_intersection) in insertion order
    for g in group_order:
        for j in rng.permutation(len(inner[g])):
            o, d = inner[g][int(j)]
            rows.append((g, o) + d)
    unweighted = combo == (0, 0, 0)
    min_conflicts = float(rng.choice([0, 0.5, 3] if unweighted else [0, 0.01, 0.03, 1]))
    min_split, min_len = [(50, 25), (20, 15), (6, 3), (2, 1)][int(rng.integers(0, 4))]
    return n_frames, group_order, spans, rows, (min_conflicts, min_split, min_len)


def dicts_of(group_order, spans, rows, sort_inner=False):
    ages = {g: [spans[g][0], spans[g][1]] if spans[g][0] != spans[g][1] else [spans[g][0]] for g in group_order}
    conf = {g: {} for g in group_order}
    for g, o, matched, unmatched, union, inter in (sorted(rows) if sort_inner else rows):
        conf[g][o] = {"matched": matched, "unmatched": unmatched, "area_union": union, "area_intersection": inter}
    return ages, conf


def make_cases():
    rng = np.random.default_rng(1804)
    acc = {k: [] for k in ("n_frames", "combo", "params", "group_off", "group_order", "spans", "row_off", "rows", "pair_off", "pairs", "iv_off", "intervals",
                           "split_off", "split_data", "sig_off", "signal0", "resorted_differs")}
    printed = []
    for case in range(CASES_PER_COMBO * len(COMBOS)):
        combo = COMBOS[case % len(COMBOS)]              # rotating: any 48 consecutive cases cover every combination
        n_frames, group_order, spans, rows, (min_conflicts, min_split, min_len) = random_case(rng, combo)
        ages, conf = dicts_of(group_order, spans, rows)
        graph, split = [], []
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            intervals = VideoSegmenter.split_video_from_group_conflicts(0, n_frames - 1, ages, conf, min_conflicts, min_split, min_len, *combo,
                                                                        0, graph, split, n_frames)
        sig = bits([graph[0][1][f] for f in range(n_frames)]) if graph else np.zeros(0, np.int64)
        ages2, conf2 = dicts_of(group_order, spans, rows, sort_inner=True)
        acc["resorted_differs"].append(bool((root_signal(n_frames, ages2, conf2, *combo) != root_signal(n_frames, ages, conf, *combo)).any()))
        acc["n_frames"].append(n_frames)
        acc["combo"].append(combo)
        acc["params"].append((min_conflicts, min_split, min_len))
        acc["group_off"].append(len(group_order))
        acc["group_order"].extend(group_order)
        acc["spans"].extend(spans[g] for g in group_order)
        acc["row_off"].append(len(rows))
        acc["rows"].extend(r[:2] for r in rows)
        once = sorted(r for r in rows if r[0] < r[1])        # both directions carry the same four numbers: stored once
        acc["pair_off"].append(len(once))
        acc["pairs"].extend(once)
        acc["iv_off"].append(len(intervals))
        acc["intervals"].extend(intervals)
        acc["split_off"].append(len(split))
        acc["split_data"].extend(split)
        acc["sig_off"].append(len(sig))
        acc["signal0"].extend(sig.tolist())
        printed.append(text.getvalue())
    n = len(printed)
    out = {"n_cases": np.int64(n), "n_frames": np.asarray(acc["n_frames"], np.int32), "combo": np.asarray(acc["combo"], np.int8),
           "params": np.asarray(acc["params"], np.float64), "group_order": np.asarray(acc["group_order"], np.int16),
           "spans": np.asarray(acc["spans"], np.int16).reshape(-1, 2), "rows": np.asarray(acc["rows"], np.int8).reshape(-1, 2),
           "pairs": np.ascontiguousarray(np.asarray(acc["pairs"], np.int16).reshape(-1, 6).T),
           "intervals": np.asarray(acc["intervals"], np.int16).reshape(-1, 2), "split_data": np.asarray(acc["split_data"], np.int16).reshape(-1, 2),
           "signal0": np.asarray(acc["signal0"], np.int64), "resorted_differs": np.asarray(acc["resorted_differs"], np.bool_),
           "printed": np.frombuffer(json.dumps(printed).encode(), np.uint8)}
    for key in ("group_off", "row_off", "pair_off", "iv_off", "split_off", "sig_off"):
        out[key] = np.concatenate([[0], np.cumsum(acc[key])]).astype(np.int64)
    check_not_vacuous(out)
    np.savez_compressed(os.path.join(HERE, "g18_conflict_cases.npz"), **out)
    print("g18:", n, "cases,", os.path.getsize(os.path.join(HERE, "g18_conflict_cases.npz")), "bytes")


def check_not_vacuous(g):
    """The conditions that keep the fixture from being vacuous (tests/test_segment_conflicts_emulated.py re-asserts them)."""
    n = int(g["n_cases"])
    n_iv = np.diff(g["iv_off"])
    deep = np.array([(g["split_data"][g["split_off"][c]:g["split_off"][c + 1], 0] >= 2).any() for c in range(n)])
    combos = [tuple(int(v) for v in c) for c in g["combo"]]
    noninteger = np.array([non_integer_weights(c) for c in combos])
    print("g18: %.0f %% split, %.0f %% split at depth >= 2, re-sorting changes %.0f %% of the non-integer cases" % (
        100 * (n_iv >= 2).mean(), 100 * deep.mean(), 100 * g["resorted_differs"][noninteger].mean()))
    assert (n_iv >= 2).mean() >= 0.5
    assert deep.mean() >= 0.25
    assert {c for c, k in zip(combos, n_iv) if k >= 2} == set(COMBOS)
    assert g["resorted_differs"][noninteger].mean() >= 0.25


if __name__ == "__main__":
    for nm in ("accumulate_erase", "occluder_return", "short_gap_jitter"):
        make_stream(nm)
    make_cases()
