"""What step 04's conflict-minimisation segmentation (VIDEO_SEGMENTATION_METHOD = 2) costs at lecture scale, three ways.

    python tools/conflict_signal_timing.py --part reference --out result.json      # where the reference is installed (CPU only)
    python tools/conflict_signal_timing.py --part host --part device --merge result.json --out result.json      # on the GPU

One synthetic case: 10,000 frames, 3,000 groups with spans of at most 80 frames, conflicts drawn like tests/golden/g18_conflict_cases.npz
(same number ranges, shuffled insertion orders) but with a pair probability that gives a group eight conflicting partners on
average instead of a quarter of all groups, and the shipped parameters (configs/FCN_LectureNet.conf: weights 3 / 3 / 1, MIN_CONFLICTS
0.03, MIN_SPLIT 20, MIN_LENGTH 15; areas normalised by a 1920 x 1080 frame as the step script does).

  reference  the reference's VideoSegmenter.from_group_conflicts itself (tests/golden/ref_env.py), three times: a CPU time of the machine it ran on
  host       a numpy restatement inside this tool: pairs flattened once, per node `signal[gap] += weight` pair by pair (the same ordered sums)
  device     the drop-in's from_group_conflicts (flatten + upload + one lm_conflict_signal launch and copy per node), and the kernel alone on
             the whole lecture and on a 500-frame segment (HIP events)

Every part records a digest of its intervals; they must agree wherever two parts are present.  Each --part merges into the --merge file's content.
"""
import argparse
import contextlib
import copy
import hashlib
import importlib.util
import io
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N_FRAMES, N_GROUPS, PARTNERS, IMG_SIZE = 10000, 3000, 8, 1920 * 1080
WEIGHTS = (3, 3, 1)
MIN_CONFLICTS, MIN_SPLIT, MIN_LEN = 0.03, 20, 15


def synthetic_case(seed=7):
    rng = np.random.default_rng(seed)
    first = rng.integers(0, N_FRAMES, N_GROUPS)
    last = np.minimum(N_FRAMES - 1, first + rng.integers(0, 81, N_GROUPS))
    inner = {g: [] for g in range(N_GROUPS)}
    n_pairs = 0
    for a in range(N_GROUPS):
        others = a + 1 + np.flatnonzero(rng.random(N_GROUPS - a - 1) < PARTNERS / (N_GROUPS - 1))
        for b in others.tolist():
            inter = int(rng.integers(1, 4000))
            d = {"matched": int(rng.integers(0, 500)), "unmatched": int(rng.integers(1, 500)), "area_union": inter + int(rng.integers(0, 8000)),
                 "area_intersection": inter}
            inner[a].append((b, d))
            inner[b].append((a, dict(d)))
            n_pairs += 1
    ages, conf = {}, {}
    for g in rng.permutation(N_GROUPS).tolist():
        ages[g] = [int(first[g]), int(last[g])]
        conf[g] = {inner[g][j][0]: inner[g][j][1] for j in rng.permutation(len(inner[g])).tolist()}
    return ages, conf, n_pairs


def normalised(conf):
    out = copy.deepcopy(conf)
    for g in out:
        for o in out[g]:
            out[g][o]["area_intersection"] /= IMG_SIZE
            out[g][o]["area_union"] /= IMG_SIZE
    return out


def digest(intervals):
    return {"n_intervals": len(intervals), "intervals_sha256": hashlib.sha256(json.dumps([list(iv) for iv in intervals]).encode()).hexdigest()}


def timed(fn, warmup, repeats):
    seconds, result = [], None
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(warmup):
            fn()
    for _ in range(repeats):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            result = fn()
        seconds.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(seconds), "min_s": min(seconds), "max_s": max(seconds), "warmup": warmup, "repeats": repeats}, result


def load_by_path(name, path):
    """the reference's module and the drop-in's have the same dotted name: each is loaded from its file under a name of its own"""
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dropin_segmenter():
    return load_by_path("lm_timing_dropin_video_segmenter",
                        os.path.join(ROOT, "lecturemath_amd", "dropin", "AccessMath", "preprocessing", "content", "video_segmenter.py"))


def part_reference(ages, conf):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import ref_env
    here = os.getcwd()
    ref_env.enter()
    os.chdir(here)
    VideoSegmenter = load_by_path("lm_timing_reference_video_segmenter",
                                  os.path.join(ref_env.REF_ROOT, "AccessMath", "preprocessing", "content", "video_segmenter.py")).VideoSegmenter
    conf = normalised(conf)
    stats, intervals = timed(lambda: VideoSegmenter.from_group_conflicts(N_FRAMES, ages, conf, MIN_CONFLICTS, MIN_SPLIT, MIN_LEN, *WEIGHTS), 0, 3)
    return dict(stats, machine=platform.processor() or platform.machine(), **digest(intervals))


def part_host(ages, conf):
    vs = dropin_segmenter()
    peaks = vs.VideoSegmenter._peaks_of_values

    def run():
        (gap_first, gap_last, alive_from, alive_until, weight), failing = vs._ConflictPairs.flatten(ages, conf, *WEIGHTS, N_FRAMES, IMG_SIZE)
        assert not failing
        intervals, todo, nodes = [], [(0, N_FRAMES - 1)], 0
        while todo:
            lo, hi = todo.pop()
            if hi - lo + 1 < MIN_SPLIT:
                intervals.append((lo, hi))
                continue
            nodes += 1
            signal = np.zeros(hi - lo + 1)
            for p in np.flatnonzero((alive_from <= hi) & (alive_until >= lo) & (gap_first <= gap_last)).tolist():
                signal[max(gap_first[p], lo) - lo:min(gap_last[p], hi) - lo + 1] += weight[p]
            tops = np.array([top for _, top, _ in peaks(lo, hi, signal)], dtype=np.int64)
            heights = signal[tops - lo]
            keep = (heights > MIN_CONFLICTS) & (tops >= lo + MIN_LEN) & (tops <= hi - MIN_LEN)
            tops, heights = tops[keep], heights[keep]
            if len(tops) == 0:
                intervals.append((lo, hi))
                continue
            best = int(tops[np.lexsort((tops, heights))[-1]])
            todo.append((best + 1, hi))
            todo.append((lo, best - 1))
        return intervals, nodes
    stats, (intervals, nodes) = timed(run, 1, 5)
    return dict(stats, machine=platform.processor() or platform.machine(), nodes=nodes, **digest(intervals))


def part_device(ages, conf):
    import torch
    from lecturemath_amd import _lib, device
    vs = dropin_segmenter()
    lib = _lib.load()
    if not lib.is_device_build or not torch.cuda.is_available():
        raise SystemExit("--part device needs the HIP library and a GPU")
    whole, intervals = timed(lambda: vs.VideoSegmenter.from_group_conflicts(N_FRAMES, ages, conf, MIN_CONFLICTS, MIN_SPLIT, MIN_LEN, *WEIGHTS, None,
                                                                             area_divisor=IMG_SIZE), 2, 7)
    flatten, (pairs, _) = timed(lambda: vs._ConflictPairs.flatten(ages, conf, *WEIGHTS, N_FRAMES, IMG_SIZE), 1, 5)
    graph = []      # one entry per node that needed a signal
    with contextlib.redirect_stdout(io.StringIO()):
        vs.VideoSegmenter.split_video_from_group_conflicts(0, N_FRAMES - 1, ages, normalised(conf), MIN_CONFLICTS, MIN_SPLIT, MIN_LEN, *WEIGHTS, 0, graph, [],
                                                           N_FRAMES)
    cs = device.ConflictSignal(pairs, lib)
    be = cs.be
    out = be.empty((N_FRAMES,), np.float64)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def kernel_us(lo, hi, reps=200):
        args = [_lib.ptr(a) for a in cs._dev] + [cs.n_pairs, lo, hi, _lib.ptr(out), be.stream()]
        for _ in range(20):
            lib.check(lib.lm_conflict_signal(*args))
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(reps):
            lib.check(lib.lm_conflict_signal(*args))
        ev1.record()
        torch.cuda.synchronize()
        return 1000.0 * ev0.elapsed_time(ev1) / reps
    return dict(whole_from_group_conflicts=whole, flatten_on_host=flatten, nodes=len(graph), pairs_uploaded=int(cs.n_pairs),
                kernel_alone_us={"frames_0_9999": kernel_us(0, N_FRAMES - 1), "frames_5000_5499": kernel_us(5000, 5499)},
                device=torch.cuda.get_device_name(0), **digest(intervals))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", action="append", choices=["reference", "host", "device"], required=True)
    ap.add_argument("--merge", help="JSON of an earlier run to add to")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    ages, conf, n_pairs = synthetic_case()
    result = json.load(open(args.merge)) if args.merge and os.path.exists(args.merge) else {}
    result["case"] = {"n_frames": N_FRAMES, "n_groups": N_GROUPS, "conflicting_pairs": n_pairs, "weights": list(WEIGHTS),
                      "min_conflicts": MIN_CONFLICTS, "min_split": MIN_SPLIT, "min_length": MIN_LEN, "image_size": IMG_SIZE}
    for part in args.part:
        result[part] = {"reference": part_reference, "host": part_host, "device": part_device}[part](ages, conf)
        print(part, json.dumps(result[part]), flush=True)
    found = [result[p]["intervals_sha256"] for p in ("reference", "host", "device") if p in result]
    result["intervals_agree"] = all(iv == found[0] for iv in found)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    if not result["intervals_agree"]:
        raise SystemExit("the parts disagree on the intervals")


if __name__ == "__main__":
    main()
