"""CPU: the pixel history on the device (lm_hist_*, device.FrameHistory, CCStabilityEstimator.
compute_group_images_from_raw_binary, KeyframeExtractor.extract) with the kernels running in the emulated build of the HIP sources;
the checks are tests/history_checks.py, the same ones tests/test_history_gpu.py runs on the GPU."""
import pytest

import history_checks as hc
import lm_checks

CASES = lm_checks.STREAMS + hc.SYNTHETIC


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_equals_the_reference(name):
    hc.check_restatement(name)


def test_fixtures_are_not_vacuous():
    hc.check_not_vacuous()


@pytest.mark.parametrize("name", CASES)
def test_raw_binary_images_against_the_reference(emu_lib, name):
    hc.check_raw_images(emu_lib, name)


def test_raw_binary_images_from_a_list_and_a_tensor(emu_lib):
    hc.check_raw_images_from_a_list(emu_lib)


def test_raw_binary_images_after_the_estimators_own_steps_02_03(emu_lib):
    """(steps 02-03 of the smallest stream take some twenty seconds on the emulator, as in test_dropin_emulated.py)"""
    hc.check_after_steps_02_03(emu_lib)


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_step05_keyframes_from_raw_binary_images(emu_lib, name):
    hc.check_step05(emu_lib, name)


@pytest.mark.parametrize("name", lm_checks.STREAMS + ["long"])
def test_extract_against_the_reference(emu_lib, name):
    hc.check_extract(emu_lib, name)


def test_extract_inputs_and_a_shared_history(emu_lib, tmp_path):
    hc.check_extract_inputs(emu_lib, tmp_path)


def test_append_in_batches(emu_lib):
    hc.check_append_batches(emu_lib)


def test_random_jobs_against_numpy(emu_lib):
    hc.check_random_jobs(emu_lib)


def test_refusals(emu_lib):
    hc.check_refusals(emu_lib)
