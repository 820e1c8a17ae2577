"""GPU: keyframes -> CC table (lm_kf_create_from_frames, device.KeyframeCCs, lecturemath_amd.keyframes, the overlay Evaluator's view
route, lm_kf_pixel_sums) on the MI355X; the checks are tests/keyframe_cc_checks.py, plus the two full-size cases."""
import pytest

import keyframe_cc_checks as kc

pytestmark = pytest.mark.gpu


def test_word_arithmetic_of_the_layout_conversion(hip_lib):
    kc.check_word_arithmetic(hip_lib)


def test_ring_around_a_dot_and_comb(hip_lib):
    kc.check_ring_and_comb(hip_lib)


def test_non_binary_bytes_empty_and_full_frames(hip_lib):
    kc.check_non_binary_empty_full(hip_lib)


def test_batches_masks_and_min_pixels(hip_lib):
    kc.check_batching_and_min_pixels(hip_lib)


def test_clean_tails_against_an_all_ink_mask(hip_lib):
    kc.check_clean_tails(hip_lib)


def test_g24_ccs_against_the_reference(hip_lib):
    kc.check_g24_ccs(hip_lib)


def test_keyframe_objects_fake_info_background_and_pickling(hip_lib):
    kc.check_keyframe_objects(hip_lib)


def test_summary_metrics_on_the_table_against_the_reference(hip_lib):
    kc.check_evaluator_reference(hip_lib)


def test_summary_metrics_on_the_table_against_the_upload_route(hip_lib):
    kc.check_evaluator_host_route(hip_lib)


def test_summary_metrics_after_a_cc_was_moved(hip_lib):
    kc.check_evaluator_moved_cc(hip_lib)


def test_pixel_sums_against_numpy(hip_lib):
    kc.check_pixel_sums(hip_lib, shapes=((3, 45, 70), (2, 40, 97), (2, 1, 1), (1, 1, 65), (1, 64, 128), (2, 1080, 1920)))


def test_pixel_binary_metrics(hip_lib):
    kc.check_pixel_metrics(hip_lib)


def test_argument_checks(hip_lib):
    kc.check_argument_errors(hip_lib)


def test_glyph_grid_1080p(hip_lib):
    kc.check_glyph_grid_1080p(hip_lib)


def test_pipeline_keyframes_1080p(hip_lib):
    kc.check_pipeline_1080p(hip_lib)
