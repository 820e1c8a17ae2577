"""CPU: step 04's conflict-minimisation segmentation (VIDEO_SEGMENTATION_METHOD = 2) of the drop-in layer, its kernel running in the
emulated build of the HIP sources, against the reference's own results (G17: the golden streams through the reference's step
script; G18: 960 random structures through the reference's VideoSegmenter.split_video_from_group_conflicts)."""
import pytest

import lm_checks
import segment_conflict_checks as scc


def test_random_cases_fixture_is_not_vacuous():
    scc.check_cases_not_vacuous(scc.cases())


def test_random_cases_match_the_reference(emu_lib):
    """all 960 cases: intervals, printed text, split_data and the depth-0 signal bit for bit"""
    scc.check_cases(emu_lib, range(960))


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_script_on_golden_stream(emu_lib, name):
    scc.check_script_stream(emu_lib, name)


def test_golden_streams_split():
    """what the three streams are expected to do under the shipped parameters and the script's defaults"""
    want = {"accumulate_erase": (3, 3), "occluder_return": (4, 4), "short_gap_jitter": (1, 2)}
    for name in lm_checks.STREAMS:
        g, _ = scc.g17(name)
        assert (len(g["intervals_0"]), len(g["intervals_1"])) == want[name]


def test_conflicts_come_in_reference_order(emu_lib):
    """(group, other) of Grouping.result()'s conflicts, in order, == the reference's; on at least one stream that order is not
    the ascending one for some group"""
    unsorted_groups = [scc.check_conflict_order(emu_lib, name) for name in lm_checks.STREAMS]
    assert max(unsorted_groups) > 0, unsorted_groups


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_presegments(emu_lib, name):
    scc.check_presegments(emu_lib, name)


def test_pipeline_method_2(emu_lib):
    scc.check_pipeline(emu_lib, "short_gap_jitter")


def test_zero_denominators_raise_like_the_reference(emu_lib):
    """A zero denominator raises ZeroDivisionError where both groups of the pair are alive in the segment (the reference divides
    before it adds, whatever the gap); a segment below min_segment_split is returned before anything is looked at."""
    scc.dropin_checks.use_library(emu_lib)
    VS = scc.segmenter()
    ages = {0: [0, 3], 1: [6, 9], 2: [20, 29]}
    d = {"matched": 0, "unmatched": 0, "area_union": 0, "area_intersection": 0}
    conf = {0: {1: dict(d)}, 1: {0: dict(d)}, 2: {}}
    for combo in ((5, 0, 0), (0, 3, 0)):
        with pytest.raises(ZeroDivisionError):
            VS.split_video_from_group_conflicts(0, 29, ages, conf, 0.0, 2, 1, *combo, 0, [], [], 30)
        assert VS.split_video_from_group_conflicts(12, 29, ages, conf, 0.0, 2, 1, *combo, 0, [], [], 30)      # neither group is alive there
        assert VS.split_video_from_group_conflicts(0, 29, ages, conf, 0.0, 31, 1, *combo, 0, [], [], 30) == [(0, 29)]
    with pytest.raises(ZeroDivisionError):
        VS.split_video_from_group_conflicts(0, 29, ages, conf, 0.0, 2, 1, 0, 0, 2, 0, [], [], 0)


def test_kernel_argument_checks(emu_lib):
    import numpy as np
    from lecturemath_amd import _lib, device
    out = np.zeros(4)
    one = np.zeros(1, np.int32)
    w = np.ones(1)
    args = [one.ctypes.data] * 4 + [w.ctypes.data]
    assert emu_lib.lm_conflict_signal(*args, 1, 3, 2, out.ctypes.data, None) == _lib.LM_ERR_ARG and "lm_conflict_signal" in emu_lib.last_error()
    assert emu_lib.lm_conflict_signal(*args, -1, 0, 3, out.ctypes.data, None) == _lib.LM_ERR_ARG
    assert emu_lib.lm_conflict_signal(*args, 1, 0, 3, None, None) == _lib.LM_ERR_ARG
    assert emu_lib.lm_conflict_signal(None, *args[1:], 1, 0, 3, out.ctypes.data, None) == _lib.LM_ERR_ARG
    out[:] = 7.0
    assert emu_lib.lm_conflict_signal(None, None, None, None, None, 0, 5, 8, out.ctypes.data, None) == _lib.LM_OK and (out == 0.0).all()
    empty = device.ConflictSignal(([], [], [], [], []), emu_lib)
    assert empty.signal(3, 70).tolist() == [0.0] * 68
