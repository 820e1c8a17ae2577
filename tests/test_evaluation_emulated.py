"""CPU: the summary evaluation on the device (lm_kf_pair_counts, device.CCPairCounts, the overlay's AccessMath.evaluation package)
with the kernels running in the emulated build of the HIP sources; the checks are tests/evaluation_checks.py, the same ones
tests/test_evaluation_gpu.py runs on the GPU."""
import evaluation_checks as ec


def test_fixture_is_not_vacuous():
    ec.check_not_vacuous()


def test_rows_and_counts_of_every_fixture_query_against_numpy(emu_lib):
    ec.check_raw_counts(emu_lib)


def test_batch_of_uneven_queries_against_numpy(emu_lib):
    ec.check_mixed_batch(emu_lib)


def test_check_equivalent_cc(emu_lib):
    ec.check_equivalent(emu_lib)


def test_keyframes_unique_cc(emu_lib):
    ec.check_unique(emu_lib)


def test_overlapping_groups_matches_and_background(emu_lib):
    ec.check_pairs(emu_lib)


def test_summary_metrics_and_reports(emu_lib):
    ec.check_summary(emu_lib)


def test_pixel_binary_metrics():
    ec.check_pixel_metrics()


def test_handle_reuse_leaves_no_stale_counts(emu_lib):
    ec.check_reuse(emu_lib)


def test_argument_checks(emu_lib):
    ec.check_argument_errors(emu_lib)


def test_all_ink_closed_form_across_row_and_word_blocks(emu_lib):
    """45 rows and 70 columns: two row blocks; the word-block split needs more than 2048 columns and is exercised on one row pair"""
    ec.check_all_ink(emu_lib, 45, 70, 2)
    ec.check_all_ink(emu_lib, 2, 2100, 1)
