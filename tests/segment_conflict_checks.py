"""Checks of step 04's conflict-minimisation segmentation (VIDEO_SEGMENTATION_METHOD = 2) shared by the CPU tests (emulated
library) and the GPU tests: the drop-in VideoSegmenter / step script / pipeline against what the reference returned, printed and
summed (tests/golden/g17_step04_conflicts_<stream>.npz, g18_conflict_cases.npz; tests/golden/make_golden_step04_conflicts.py)."""
import contextlib
import copy
import io
import json
import os
import pickle
import sys

import numpy as np

import dropin_checks
import lm_checks

K = "VIDEO_SEGMENTATION_CONFLICTS_"
COMBOS = [(a, p, t) for a in (0, 3, 4, 5) for p in (0, 1, 2, 3) for t in (0, 1, 2)]
# what the reference's script prints around method 2 for work the drop-in script does not do: the progress lines of its debug mode (all
# frames decompressed, their sums computed for a plot) in front, and save_conflict_plot's warning for every depth without a plot
REFERENCE_PREAMBLE = "Decompressing input...\nComputing sums...\n"
REFERENCE_PLOT_WARNING = "WARNING: Cannot generate conflict plot at Depth <"


def without_plot_output(text):
    assert text.startswith(REFERENCE_PREAMBLE)
    return "".join(line for line in text[len(REFERENCE_PREAMBLE):].splitlines(True) if not line.startswith(REFERENCE_PLOT_WARNING))


def segmenter():
    if dropin_checks.DROPIN not in sys.path:
        sys.path.insert(0, dropin_checks.DROPIN)
    from AccessMath.preprocessing.content.video_segmenter import VideoSegmenter
    return VideoSegmenter


def pairs_of(iv):
    return [tuple(int(v) for v in r) for r in iv]


# ---- G18: random structures ------------------------------------------------------------------------------------------------------
_cases = None


def cases():
    global _cases
    if _cases is None:
        g = np.load(os.path.join(lm_checks.GOLD, "g18_conflict_cases.npz"))
        _cases = {k: g[k] for k in g.files}
        _cases["printed"] = json.loads(bytes(_cases["printed"]).decode())
    return _cases


def case_inputs(g, c):
    """(n_frames, group_ages, conflicts) of case c, the dicts filled in the recorded insertion orders"""
    sl = slice(g["group_off"][c], g["group_off"][c + 1])
    ages = {int(k): ([int(a), int(b)] if a != b else [int(a)]) for k, (a, b) in zip(g["group_order"][sl], g["spans"][sl])}
    numbers = {(int(r[0]), int(r[1])): tuple(int(v) for v in r[2:]) for r in g["pairs"][:, g["pair_off"][c]:g["pair_off"][c + 1]].T}
    conf = {k: {} for k in ages}
    for grp, other in g["rows"][g["row_off"][c]:g["row_off"][c + 1]]:
        grp, other = int(grp), int(other)
        matched, unmatched, union, inter = numbers[(min(grp, other), max(grp, other))]
        conf[grp][other] = {"matched": matched, "unmatched": unmatched, "area_union": union, "area_intersection": inter}
    return int(g["n_frames"][c]), ages, conf


def check_cases_not_vacuous(g):
    """The fixture is worth something: most cases split, many of them deep, every weight combination splits somewhere, and the
    order of the inner dicts matters for the combinations whose weights are not integers."""
    n = int(g["n_cases"])
    assert n == 960 and [tuple(int(v) for v in c) for c in g["combo"][:48]] == COMBOS and (g["combo"][48:] == g["combo"][:-48]).all()
    n_iv = np.diff(g["iv_off"])
    deep = np.array([(g["split_data"][g["split_off"][c]:g["split_off"][c + 1], 0] >= 2).any() for c in range(n)])
    combos = [tuple(int(v) for v in c) for c in g["combo"]]
    noninteger = np.array([c[0] == 5 or c[1] == 3 or c[2] == 2 for c in combos])
    assert (n_iv >= 2).mean() >= 0.5
    assert deep.mean() >= 0.25
    assert {c for c, k in zip(combos, n_iv) if k >= 2} == set(COMBOS)
    assert g["resorted_differs"][noninteger].mean() >= 0.25


def check_cases(lib, which):
    """split_video_from_group_conflicts of the drop-in on G18 cases: intervals, printed text, split_data and the depth-0 signal bit
    for bit."""
    dropin_checks.use_library(lib)
    VS = segmenter()
    g = cases()
    for c in which:
        n_frames, ages, conf = case_inputs(g, c)
        min_conflicts, min_split, min_len = float(g["params"][c][0]), int(g["params"][c][1]), int(g["params"][c][2])
        combo = tuple(int(v) for v in g["combo"][c])
        before = copy.deepcopy(conf)
        graph, split = [], []
        with contextlib.redirect_stdout(io.StringIO()) as text:
            intervals = VS.split_video_from_group_conflicts(0, n_frames - 1, ages, conf, min_conflicts, min_split, min_len, *combo, 0, graph, split, n_frames)
        assert intervals == pairs_of(g["intervals"][g["iv_off"][c]:g["iv_off"][c + 1]]), c
        assert text.getvalue() == g["printed"][c], c
        assert split == pairs_of(g["split_data"][g["split_off"][c]:g["split_off"][c + 1]]), c
        want = g["signal0"][g["sig_off"][c]:g["sig_off"][c + 1]]
        if len(want) == 0:
            assert graph == [], c
        else:
            depth, signal = graph[0]
            got = np.array([signal[f] for f in range(n_frames)], np.float64).view(np.int64)
            assert depth == 0 and len(signal) == n_frames and (got == want).all(), c
        assert conf == before and [list(conf[k]) for k in conf] == [list(before[k]) for k in before], c


# ---- G17: the golden streams -----------------------------------------------------------------------------------------------------
def g17(name):
    g = np.load(os.path.join(lm_checks.GOLD, "g17_step04_conflicts_%s.npz" % name))
    return g, json.loads(bytes(g["params"]).decode())


_step03 = {}


def steps_02_03(lib, name):
    """The drop-in's own steps 02 -> pickle -> 03 on a golden stream (the calls of dropin_checks.check_steps_02_03): step 03's outputs
    [(times, indices, compressed frames), (group_ages, conflicts), st3d] and the stream's spec.  Computed once per library and stream."""
    key = (lib.path, name)
    if key not in _step03:
        dropin_checks.use_library(lib)
        from lecturemath_amd import png
        g, spec, frames = lm_checks.load_stream(name)
        compressed = [png.encode_gray8(f) for f in frames]
        times, idxs = [1000.0 * i for i in range(len(frames))], list(range(len(frames)))
        s02 = dropin_checks.load_script("pre_ST3D_v3.0_02_cc_analaysis.py")
        s03 = dropin_checks.load_script("pre_ST3D_v3.0_03_cc_grouping.py")
        out02 = s02.process_input(dropin_checks.fake_process({"CC_STABILITY_MAX_GAP": str(spec["gap2"])}), (times, idxs, compressed))
        t2, i2, est2 = pickle.loads(pickle.dumps(out02, protocol=pickle.HIGHEST_PROTOCOL))
        with contextlib.redirect_stdout(io.StringIO()):
            out03 = s03.process_input(dropin_checks.fake_process({"CC_STABILITY_MAX_GAP": str(spec["gap3"])}), (t2, i2, est2))
        _step03[key] = (list(out03), spec, g)
    dropin_checks.use_library(lib)
    return _step03[key]


def method2_process(values):
    return dropin_checks.fake_process(dict({key: str(v) for key, v in values.items()}, VIDEO_SEGMENTATION_METHOD="2"))


def normalised(conflicts, values, spec):
    """the conflicts as the reference's script hands them to VideoSegmenter: areas divided by the image size for area modes 3 and 4"""
    conf = copy.deepcopy(conflicts)
    if values[K + "WEIGHTS"] in (3, 4):
        for grp in conf:
            for other in conf[grp]:
                conf[grp][other]["area_intersection"] /= spec["h"] * spec["w"]
                conf[grp][other]["area_union"] /= spec["h"] * spec["w"]
    return conf


def check_script_stream(lib, name):
    """pre_ST3D 04 with method 2 on the drop-in's own step-03 outputs: intervals and printed text of the reference for the six
    parameter sets of G17, the depth-0 signal bit for bit, and the caller's conflicts untouched."""
    step03, spec, _ = steps_02_03(lib, name)
    g, param_sets = g17(name)
    s04 = dropin_checks.load_script("pre_ST3D_v3.0_04_vid_segmentation.py")
    VS = segmenter()
    group_ages, conflicts = step03[1]
    before = copy.deepcopy(conflicts)
    order_before = [list(conflicts[k]) for k in conflicts]
    n = int(g["n_frames"])
    assert len(param_sets) == 6 and n == len(step03[0][1])
    for k, values in enumerate(param_sets):
        with contextlib.redirect_stdout(io.StringIO()) as text:
            intervals = s04.process_input(method2_process(values), step03[:2])
        assert pairs_of(intervals) == pairs_of(g["intervals_%d" % k]), (name, k)
        assert text.getvalue() == without_plot_output(bytes(g["printed_%d" % k]).decode()), (name, k)
        assert conflicts == before and [list(conflicts[j]) for j in conflicts] == order_before, (name, k)
        graph = []
        with contextlib.redirect_stdout(io.StringIO()):
            VS.split_video_from_group_conflicts(0, n - 1, group_ages, normalised(conflicts, values, spec), 0.0, 0, n + 1, values[K + "WEIGHTS"],
                                                values[K + "WEIGHTS_PIXELS"], values[K + "WEIGHTS_TIME"], 0, graph, [], n)
        got = np.array([graph[0][1][f] for f in range(n)], np.float64).view(np.int64)
        assert (got == g["signal0_%d" % k]).all(), (name, k)
    return len(pairs_of(g["intervals_1"]))


def check_conflict_order(lib, name):
    """The inner dicts of Grouping.result()'s conflicts are filled in the reference's first-encounter order (G3 keeps it)."""
    step03, _, g3 = steps_02_03(lib, name)
    conf = step03[1][1]
    got = [(grp, other) for grp in sorted(conf) for other in conf[grp]]
    want = [(int(r[0]), int(r[1])) for r in g3["conflicts"]]
    assert got == want and len(want) > 0
    return sum(1 for grp in conf if list(conf[grp]) != sorted(conf[grp]))


def check_presegments(lib, name):
    """from_group_conflicts_with_presegments on the pre-segments method 3 found (G7, parameter set 2) == the reference's result ==
    one split_video_from_group_conflicts call per pre-segment, for the six parameter sets."""
    step03, spec, _ = steps_02_03(lib, name)
    g, param_sets = g17(name)
    VS = segmenter()
    group_ages, conflicts = step03[1]
    n = int(g["n_frames"])
    pre = pairs_of(g["pre_segments"])
    assert pre == pairs_of(dropin_checks.g7(name)[0]["intervals_2"])
    for k, values in enumerate(param_sets):
        rest = (values[K + "MIN_CONFLICTS"], values[K + "MIN_SPLIT"], values[K + "MIN_LENGTH"], values[K + "WEIGHTS"], values[K + "WEIGHTS_PIXELS"],
                values[K + "WEIGHTS_TIME"])
        conf = normalised(conflicts, values, spec)
        with contextlib.redirect_stdout(io.StringIO()):
            together = VS.from_group_conflicts_with_presegments(n, pre, group_ages, conf, *rest)
            apart = [iv for seg in pre for iv in VS.split_video_from_group_conflicts(seg[0], seg[1], group_ages, conf, *rest, 0, [], [], n)]
            divisor = spec["h"] * spec["w"] if values[K + "WEIGHTS"] in (3, 4) else None
            scaled = VS.from_group_conflicts_with_presegments(n, pre, group_ages, conflicts, *rest, None, area_divisor=divisor)
        assert together == pairs_of(g["preseg_intervals_%d" % k]) and apart == together and scaled == together, (name, k)


def check_pipeline(lib, name, k=1):
    """LecturePipeline with VIDEO_SEGMENTATION_METHOD = 2 (parameter set k of G17; the shipped one by default) returns the
    reference's intervals and leaves the conflicts it returns as step 03 made them."""
    dropin_checks.use_library(lib)
    from lecturemath_amd.pipeline import LecturePipeline
    g3, spec, frames = lm_checks.load_stream(name)
    g, param_sets = g17(name)
    conf = dict(param_sets[k], VIDEO_SEGMENTATION_METHOD=2, CC_STABILITY_MAX_GAP=spec["gap2"])
    pipe = LecturePipeline(spec["w"], spec["h"], conf=conf, lib=lib)
    n = len(frames)
    pipe.add_binary_frames(np.stack(frames), [1000.0 * i for i in range(n)], list(range(n)))
    pipe.configuration.data["CC_STABILITY_MAX_GAP"] = str(spec["gap3"])      # the fixtures ran steps 02 and 03 with different values
    out = pipe.finish()         # no reconstructed PNGs: area mode 3 takes the image size from the SpaceTimeStruct the pipeline hands over
    assert pairs_of(out["intervals"]) == pairs_of(g["intervals_%d" % k]) and len(out["intervals"]) >= 2
    rows = [(grp, other, d["matched"], d["unmatched"], d["area_union"], float(d["area_intersection"]))
            for grp in sorted(out["conflicts"]) for other, d in out["conflicts"][grp].items()]
    assert [tuple(float(v) for v in r) for r in rows] == [tuple(float(v) for v in r) for r in g3["conflicts"]]
    assert len(out["keyframes"]) == len(out["intervals"])
