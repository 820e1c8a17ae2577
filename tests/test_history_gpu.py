"""GPU: the pixel history on the device (lm_hist_*, device.FrameHistory, CCStabilityEstimator.
compute_group_images_from_raw_binary, KeyframeExtractor.extract) on the MI355X; the checks are tests/history_checks.py, the same
ones tests/test_history_emulated.py runs on the emulated build."""
import pytest

import history_checks as hc
import lm_checks

pytestmark = pytest.mark.gpu

CASES = lm_checks.STREAMS + hc.SYNTHETIC


def test_fixtures_are_not_vacuous():
    hc.check_not_vacuous()


@pytest.mark.parametrize("name", CASES)
def test_raw_binary_images_against_the_reference(hip_lib, name):
    hc.check_raw_images(hip_lib, name)


def test_raw_binary_images_from_a_list_and_a_tensor(hip_lib):
    hc.check_raw_images_from_a_list(hip_lib)


def test_raw_binary_images_after_the_estimators_own_steps_02_03(hip_lib):
    hc.check_after_steps_02_03(hip_lib)


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_step05_keyframes_from_raw_binary_images(hip_lib, name):
    hc.check_step05(hip_lib, name)


@pytest.mark.parametrize("name", lm_checks.STREAMS + ["long"])
def test_extract_against_the_reference(hip_lib, name):
    hc.check_extract(hip_lib, name)


def test_extract_inputs_and_a_shared_history(hip_lib, tmp_path):
    hc.check_extract_inputs(hip_lib, tmp_path)


def test_append_in_batches(hip_lib):
    hc.check_append_batches(hip_lib)


def test_random_jobs_against_numpy(hip_lib):
    hc.check_random_jobs(hip_lib)


def test_refusals(hip_lib):
    hc.check_refusals(hip_lib)
