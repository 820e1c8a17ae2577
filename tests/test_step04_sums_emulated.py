"""CPU: step 04's SUMS segmentation (VIDEO_SEGMENTATION_METHOD = 1).  The regression tree restated without sklearn and the
VideoSegmenter methods around it against the reference's results (G20: 400 random signals, the three golden streams through the
reference's step script), the step script and LecturePipeline, and lm_group_frame_sums -- the sums of the reconstructed frames read
off the render tiles' cover counts -- against the rendered frames, running in the emulated build of the HIP sources."""
import numpy as np
import pytest

import lm_checks
import step04_sums_checks as ssc


def test_random_cases_fixture_is_not_vacuous():
    ssc.check_cases_not_vacuous(ssc.g20())


def test_fixture_names_its_sklearn():
    assert bytes(ssc.g20()["sklearn_version"]).decode() == "1.7.2"


def test_random_cases_match_the_reference():
    """all cases: interval_idxs, interval_vals bit for bit, segments"""
    ssc.check_cases()


def test_tree_matches_sklearn_on_fresh_signals():
    pytest.importorskip("sklearn")
    ssc.check_tree_vs_sklearn()


def test_segment_quirks_of_the_reference():
    VS = ssc.segmenter()
    # an erasure that starts at frame 0 leaves a segment ending at -1; a single frame behind the last erasure is no segment
    assert VS.video_segments_from_erasing_intervals([(0, 4), (10, 18)], 20) == [(0, -1), (5, 9)]
    assert VS.video_segments_from_erasing_intervals([(3, 4)], 7) == [(0, 2), (5, 6)]
    assert VS.video_segments_from_erasing_intervals([], 1) == []
    assert VS.identify_descend_intervals([5.0, 4.0, 3.0, 3.0, 2.5, 9.0, 1.0], 1.0) == [(1, 2), (6, 6)]
    assert VS.identify_descend_intervals([5.0, 4.0], 0.0) == [(1, 1)]
    # the unused ratio is still divided: Python floats raise, numpy floats warn
    with pytest.raises(ZeroDivisionError):
        VS.identify_descend_intervals([0.0, -1.0], 0.5)
    with pytest.warns(RuntimeWarning):
        assert VS.identify_descend_intervals([np.float64(0.0), np.float64(-1.0)], 0.5) == [(1, 1)]
    tree = VS.create_regresor_from_sums([3.0, 3.0, 9.0, 9.0, 1.0, 1.0], 2)
    assert tree.predict(np.arange(6).reshape(6, 1)).tolist() == [3.0, 3.0, 9.0, 9.0, 1.0, 1.0]
    assert VS.get_tree_decision_boundaries(tree, 6) == ([0, 2, 4], [3.0, 9.0, 1.0])
    assert VS.video_segments_from_sums([3.0, 3.0, 9.0, 9.0, 1.0, 1.0], 2, 0.05) == [(0, 3)]


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_script_on_golden_stream(emu_lib, name):
    ssc.check_script_stream(emu_lib, name)


def test_every_golden_stream_splits():
    g = ssc.g20()
    for name in lm_checks.STREAMS:
        assert max(len(g["%s.intervals_%d" % (name, k)]) for k in range(len(g["params"]))) >= 2, name


def test_script_sums_parameter(emu_lib):
    ssc.check_script_sums_parameter(emu_lib, "short_gap_jitter")


def test_script_device_codec(emu_lib):
    """the first 10 frames, 4 files per decode call (three calls, the last one short)"""
    ssc.check_script_device_codec(emu_lib, "short_gap_jitter", n_frames=10, batch=4)


def test_other_methods_still_refused(emu_lib):
    ssc.dropin_checks.use_library(emu_lib)
    s04 = ssc.dropin_checks.load_script("pre_ST3D_v3.0_04_vid_segmentation.py")
    for method in ("0", "4"):
        with pytest.raises(NotImplementedError):
            s04.process_input(ssc.dropin_checks.fake_process({"VIDEO_SEGMENTATION_METHOD": method}), ([], [], []))


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_pipeline_method_1(emu_lib, name):
    ssc.check_pipeline(emu_lib, name)


def test_abi_has_group_frame_sums(emu_lib):
    assert hasattr(emu_lib.cdll, "lm_group_frame_sums") and "lm_group_frame_sums" in ssc._lib.SIGNATURES


@pytest.mark.parametrize("name", ssc.KERNEL_STREAMS)
def test_group_frame_sums_vs_rendered_frames(emu_lib, name):
    values = ssc.check_kernel_stream(emu_lib, name)
    if name == "blink_overlap":
        assert {0, 253, 254, 255} <= values


def test_group_frame_sums_argument_checks(emu_lib):
    ssc.check_kernel_arguments(emu_lib)
