"""GPU: lm_group_frame_sums (the sums of the reconstructed frames from the render tiles' cover counts, no frame written) against
lm_group_render + numpy and + lm_frame_sums on streams with overlapping group images across tile borders (80 x 300), crowded tiles
(72 x 520, the largest shape) and the three golden streams, whole and in sub-ranges; method 1 through LecturePipeline and through
the step script with the PNG list decoded and summed on the device."""
import pytest

import step04_sums_checks as ssc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ssc.KERNEL_STREAMS)
def test_group_frame_sums_vs_rendered_frames(hip_lib, name):
    values = ssc.check_kernel_stream(hip_lib, name)
    if name == "blink_overlap":
        assert {0, 253, 254, 255} <= values


def test_group_frame_sums_argument_checks(hip_lib):
    ssc.check_kernel_arguments(hip_lib)


def test_pipeline_method_1(hip_lib):
    ssc.check_pipeline(hip_lib, "short_gap_jitter")


def test_script_device_codec(hip_lib):
    assert ssc.check_script_device_codec(hip_lib, "occluder_return") == 4
