"""The drop-in VideoSegmenter's peak finder and recursive splitter -- own formulations on the sign of the first difference / an
explicit stack -- against the reference's implementations (AccessMath/preprocessing/content/video_segmenter.py:133-182, 499-520) on
thousands of random signals full of ties and plateaus, including what they print.  What the reference returned and printed on these
signals is stored in tests/golden/g12_video_segmenter.npz (tests/golden/make_golden_reference_checks.py)."""
import contextlib
import importlib.util
import io
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def segmenter_cases():
    """(signal, a, b, min_length, threshold) of the 2000 trials"""
    rng = np.random.default_rng(0)
    for trial in range(2000):
        n = int(rng.integers(1, 60))
        sig = (rng.integers(0, 4, n).astype(float), np.round(rng.random(n), 1), np.cumsum(rng.integers(-1, 2, n)).astype(float))[trial % 3]
        a = int(rng.integers(0, n))
        b = int(rng.integers(a, n))
        ml, thr = int(rng.integers(0, 6)), float(rng.choice([0.0, 0.5, 1.0, 2.0]))
        yield sig, a, b, ml, thr


def test_peaks_and_splits_match_the_reference():
    spec = importlib.util.spec_from_file_location(
        "lm_dropin_video_segmenter", os.path.join(os.path.dirname(HERE), "lecturemath_amd/dropin/AccessMath/preprocessing/content/video_segmenter.py"))
    mine = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mine)
    ref = json.loads(bytes(np.load(os.path.join(HERE, "golden", "g12_video_segmenter.npz"))["cases"]).decode())
    n = 0
    for trial, (sig, a, b, ml, thr) in enumerate(segmenter_cases()):
        r = ref[trial]
        assert mine.VideoSegmenter.find_signal_peaks(a, b, sig) == [tuple(t) for t in r["peaks"]], trial
        with contextlib.redirect_stdout(io.StringIO()) as o2:
            s2 = mine.VideoSegmenter.split_video_from_group_deletes(sig, 0, len(sig) - 1, ml, thr)
        assert s2 == [tuple(t) for t in r["splits"]] and o2.getvalue() == r["printed"], trial
        n += 1
    assert n == len(ref) == 2000
