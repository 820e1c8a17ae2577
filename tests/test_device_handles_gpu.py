"""GPU: the handle lifecycle, counters and pickling of the lecturemath_amd.device package on the MI355X; the checks are
tests/device_handle_checks.py, the same ones tests/test_device_handles_emulated.py runs on the emulated build.  No check calls the
library through a closed handle."""
import pytest

import device_handle_checks as dc

pytestmark = pytest.mark.gpu


def test_frame_labeler(hip_lib):
    dc.check_labeler(hip_lib)


def test_frame_stream_grouping_and_its_views(hip_lib):
    dc.check_stream_and_grouping(hip_lib)


def test_group_images_from_host(hip_lib):
    dc.check_group_images(hip_lib)


def test_frame_history(hip_lib):
    dc.check_history(hip_lib)


def test_translation_aligner(hip_lib):
    dc.check_aligner(hip_lib)


def test_cc_pair_counts(hip_lib):
    dc.check_pair_counts(hip_lib)


def test_keyframe_ccs(hip_lib):
    dc.check_keyframe_ccs(hip_lib)


def test_device_cc_pickles_as_a_plain_connected_component(hip_lib):
    dc.check_device_cc_pickles_plain(hip_lib)
