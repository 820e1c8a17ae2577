#!/usr/bin/env python3
"""G11-G13: what the reference's own modules return on the inputs of the drop-in-vs-reference tests, run through THE REFERENCE in
this container, so that those tests need nothing outside the repository.

  g11_interval_index.npz      IntervalIndex.find_matches (tools/interval_index.py:42-99) on the random interval sets of
                              tests/test_reference_binding.py: per trial, the sorted (a, b) pairs
  g12_video_segmenter.npz     VideoSegmenter.find_signal_peaks / split_video_from_group_deletes (video_segmenter.py:133-182,
                              499-520) on the random signals of tests/test_step04_vs_reference.py: peaks, splits, printed text
  g13_ref_step02_short_gap_jitter.pkl.gz
                              the reference's step-02 pickle (times, indices, CCStabilityEstimator after add_frame over the G3
                              short_gap_jitter frames), as pre_ST3D_v3.0_02_cc_analaysis.py writes it
  g14_legacy_exports.json     the classical-binarizer exports of accessmath_lib.c, compiled by its own recipe, on the inputs of
                              tests/lm_checks.py:legacy_cases (up to 1080p): sha256 of every output array, speaker_detection results
"""
import contextlib
import ctypes
import gzip
import io
import json
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
import ref_env  # noqa: E402
import lm_checks  # noqa: E402
import test_reference_binding as trb  # noqa: E402
import test_step04_vs_reference as tsv  # noqa: E402

ref_env.enter()
from AccessMath.preprocessing.tools.interval_index import IntervalIndex  # noqa: E402
from AccessMath.preprocessing.content.video_segmenter import VideoSegmenter  # noqa: E402
from AccessMath.preprocessing.content.cc_stability_estimator import CCStabilityEstimator  # noqa: E402


def make_g11():
    off, pairs = [0], []
    for a, b in trb.interval_trials(IntervalIndex):
        p = sorted((int(x), int(y)) for x, y in a.find_matches(b))
        pairs.extend(p)
        off.append(len(pairs))
    np.savez_compressed(os.path.join(HERE, "g11_interval_index.npz"), off=np.asarray(off, np.int64),
                        pairs=np.asarray(pairs, np.int32).reshape(-1, 2))
    print("g11:", len(off) - 1, "trials,", len(pairs), "pairs")


def make_g12():
    cases = []
    for sig, a, b, ml, thr in tsv.segmenter_cases():
        peaks = [[int(v) for v in t] for t in VideoSegmenter.find_signal_peaks(a, b, sig)]
        with contextlib.redirect_stdout(io.StringIO()) as o:
            s = VideoSegmenter.split_video_from_group_deletes(sig, 0, len(sig) - 1, ml, thr)
        cases.append({"peaks": peaks, "splits": [[int(v) for v in t] for t in s], "printed": o.getvalue()})
    np.savez_compressed(os.path.join(HERE, "g12_video_segmenter.npz"), cases=np.frombuffer(json.dumps(cases).encode(), np.uint8))
    print("g12:", len(cases), "cases")


def make_g13():
    g, spec, frames = lm_checks.load_stream("short_gap_jitter")
    est = CCStabilityEstimator(spec["w"], spec["h"], 0.85, 0.85, spec["gap2"], False)
    for f in frames:
        est.add_frame(f, True)
    est.finish_processing = None
    times = [1000.0 * i for i in range(len(frames))]
    blob = pickle.dumps((times, list(range(len(frames))), est), protocol=pickle.HIGHEST_PROTOCOL)
    with gzip.GzipFile(os.path.join(HERE, "g13_ref_step02_short_gap_jitter.pkl.gz"), "wb", mtime=0) as fh:
        fh.write(blob)
    print("g13:", len(blob), "bytes of pickle")


def make_g14():
    lib = ctypes.CDLL(os.path.join(ref_env.enter(), "accessmath_lib.so"))
    cases = dict(lm_checks.legacy_cases(lib, big=True))
    with open(os.path.join(HERE, "g14_legacy_exports.json"), "w") as fh:
        json.dump(cases, fh, indent=0, sort_keys=True)
    print("g14:", len(cases), "cases")


if __name__ == "__main__":
    make_g14()
    make_g11()
    make_g12()
    make_g13()
