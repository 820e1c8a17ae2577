"""GPU: the summary evaluation on the device (lm_kf_pair_counts, device.CCPairCounts, the overlay's AccessMath.evaluation package) on
the MI355X; the checks are tests/evaluation_checks.py, the same ones tests/test_evaluation_emulated.py runs on the emulated build,
and three that need the device: a full 1080p item, 2,000 x 2,000 glyphs, and keyframes rendered from a G8 stream."""
import pytest

import evaluation_checks as ec

pytestmark = pytest.mark.gpu


def test_fixture_is_not_vacuous():
    ec.check_not_vacuous()


def test_rows_and_counts_of_every_fixture_query_against_numpy(hip_lib):
    ec.check_raw_counts(hip_lib)


def test_batch_of_uneven_queries_against_numpy(hip_lib):
    ec.check_mixed_batch(hip_lib)


def test_check_equivalent_cc(hip_lib):
    ec.check_equivalent(hip_lib)


def test_keyframes_unique_cc(hip_lib):
    ec.check_unique(hip_lib)


def test_overlapping_groups_matches_and_background(hip_lib):
    ec.check_pairs(hip_lib)


def test_summary_metrics_and_reports(hip_lib):
    ec.check_summary(hip_lib)


def test_handle_reuse_leaves_no_stale_counts(hip_lib):
    ec.check_reuse(hip_lib)


def test_argument_checks(hip_lib):
    ec.check_argument_errors(hip_lib)


def test_all_ink_closed_form_across_row_and_word_blocks(hip_lib):
    ec.check_all_ink(hip_lib, 45, 70, 2)
    ec.check_all_ink(hip_lib, 2, 2100, 1)


def test_all_ink_1080p(hip_lib):
    """2,073,600 shared pixels at the centre, 34 row blocks of 60 words, 49 displacements: counter width and the row-block split"""
    ec.check_all_ink(hip_lib, 1080, 1920, 3)


def test_glyph_grid_2000_by_2000(hip_lib):
    """a 40 x 50 grid of glyph-sized items against a jittered copy in one query: 4,000,000 box tests, more rows than the first
    capacity"""
    ec.check_glyph_grid(hip_lib)


def test_unique_ccs_of_rendered_g8_keyframes(hip_lib):
    ec.check_g8_unique(hip_lib)
