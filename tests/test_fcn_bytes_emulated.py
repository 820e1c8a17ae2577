"""CPU: step 01's byte images on the device (lm_fcn_bytes, FcnEngine.byte_images, FCN_LectureNet.binarize_device, the worker's device
route) with the kernels running in the emulated build of the HIP sources; the checks are tests/fcn_bytes_checks.py, the same ones
tests/test_fcn_bytes_gpu.py runs on the GPU."""
import pytest

import fcn_bytes_checks as fc


def test_fixtures_and_restatement_are_not_vacuous():
    fc.check_not_vacuous()


@pytest.mark.parametrize("name", fc.CASES)
def test_kernel_against_the_reference_bytes(emu_lib, name):
    fc.check_reference_bytes(emu_lib, name)


def test_hard_mode_equals_lm_threshold(emu_lib):
    fc.check_hard_equals_threshold(emu_lib)


@pytest.mark.parametrize("n", fc.SHAPE_SIZES)
def test_shapes_against_the_restatement(emu_lib, n):
    fc.check_shapes(emu_lib, n)


def test_absent_pairs(emu_lib):
    fc.check_absent_pairs(emu_lib)


def test_batch_written_frame_by_frame_into_slices(emu_lib):
    fc.check_batch_slices(emu_lib)


def test_argument_checks(emu_lib):
    fc.check_argument_errors(emu_lib)


def test_dropin_class_and_worker(emu_lib):
    """one G5 case and the short form here (an emulated forward pass takes most of a minute, as in test_dropin_emulated.py); the GPU
    file runs all three cases in full"""
    fc.check_dropin_class(emu_lib, "k7_70x94", full=False)


def test_soft_outputs_above_25mp_are_refused(emu_lib):
    fc.check_soft_above_25mp_is_refused(emu_lib)
