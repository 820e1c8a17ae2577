"""CPU: the handle lifecycle, counters, exported names and host-side helpers of the lecturemath_amd.device package with the emulated
build of the HIP sources; the checks are tests/device_handle_checks.py, the same ones tests/test_device_handles_gpu.py runs on the GPU."""
import device_handle_checks as dc


def test_public_names_of_the_package():
    dc.check_public_names()


def test_csr_and_flatten_images_equal_the_expressions_they_replace():
    dc.check_helpers()


def test_frame_labeler(emu_lib):
    dc.check_labeler(emu_lib)


def test_frame_stream_grouping_and_its_views(emu_lib):
    dc.check_stream_and_grouping(emu_lib)


def test_group_images_from_host(emu_lib):
    dc.check_group_images(emu_lib)


def test_frame_history(emu_lib):
    dc.check_history(emu_lib)


def test_translation_aligner(emu_lib):
    dc.check_aligner(emu_lib)


def test_cc_pair_counts(emu_lib):
    dc.check_pair_counts(emu_lib)


def test_keyframe_ccs(emu_lib):
    dc.check_keyframe_ccs(emu_lib)


def test_device_cc_pickles_as_a_plain_connected_component(emu_lib):
    dc.check_device_cc_pickles_plain(emu_lib)
