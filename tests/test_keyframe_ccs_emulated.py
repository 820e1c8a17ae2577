"""CPU: keyframes -> CC table (lm_kf_create_from_frames, device.KeyframeCCs, lecturemath_amd.keyframes, the overlay Evaluator's view
route, lm_kf_pixel_sums) with the kernels running in the emulated build of the HIP sources; the checks are
tests/keyframe_cc_checks.py, the same ones tests/test_keyframe_ccs_gpu.py runs on the GPU.  Left to the GPU file for time: the two
1080p cases (check_glyph_grid_1080p, check_pipeline_1080p)."""
import keyframe_cc_checks as kc


def test_fixture_is_not_vacuous():
    kc.check_fixture_not_vacuous()


def test_word_arithmetic_of_the_layout_conversion(emu_lib):
    kc.check_word_arithmetic(emu_lib)


def test_ring_around_a_dot_and_comb(emu_lib):
    kc.check_ring_and_comb(emu_lib)


def test_non_binary_bytes_empty_and_full_frames(emu_lib):
    kc.check_non_binary_empty_full(emu_lib)


def test_batches_masks_and_min_pixels(emu_lib):
    kc.check_batching_and_min_pixels(emu_lib)


def test_clean_tails_against_an_all_ink_mask(emu_lib):
    kc.check_clean_tails(emu_lib)


def test_g24_ccs_against_the_reference(emu_lib):
    kc.check_g24_ccs(emu_lib)


def test_keyframe_objects_fake_info_background_and_pickling(emu_lib):
    kc.check_keyframe_objects(emu_lib)


def test_summary_metrics_on_the_table_against_the_reference(emu_lib):
    kc.check_evaluator_reference(emu_lib)


def test_summary_metrics_on_the_table_against_the_upload_route(emu_lib):
    kc.check_evaluator_host_route(emu_lib)


def test_summary_metrics_after_a_cc_was_moved(emu_lib):
    kc.check_evaluator_moved_cc(emu_lib)


def test_pixel_sums_against_numpy(emu_lib):
    kc.check_pixel_sums(emu_lib)


def test_pixel_binary_metrics(emu_lib):
    kc.check_pixel_metrics(emu_lib)


def test_argument_checks(emu_lib):
    kc.check_argument_errors(emu_lib)
