"""GPU: step 01's byte images on the device (lm_fcn_bytes, FcnEngine.byte_images, FCN_LectureNet.binarize_device, the worker's device
route) on the MI355X; the checks are tests/fcn_bytes_checks.py, the same ones tests/test_fcn_bytes_emulated.py runs on the emulated
build."""
import pytest

import dropin_checks
import fcn_bytes_checks as fc

pytestmark = pytest.mark.gpu


def test_fixtures_and_restatement_are_not_vacuous():
    fc.check_not_vacuous()


@pytest.mark.parametrize("name", fc.CASES)
def test_kernel_against_the_reference_bytes(hip_lib, name):
    fc.check_reference_bytes(hip_lib, name)


def test_hard_mode_equals_lm_threshold(hip_lib):
    fc.check_hard_equals_threshold(hip_lib)


@pytest.mark.parametrize("n", fc.SHAPE_SIZES)
def test_shapes_against_the_restatement(hip_lib, n):
    fc.check_shapes(hip_lib, n)


def test_absent_pairs(hip_lib):
    fc.check_absent_pairs(hip_lib)


def test_batch_written_frame_by_frame_into_slices(hip_lib):
    fc.check_batch_slices(hip_lib)


def test_argument_checks(hip_lib):
    fc.check_argument_errors(hip_lib)


@pytest.mark.parametrize("name", fc.CASES)
def test_dropin_class_and_worker(hip_lib, name):
    fc.check_dropin_class(hip_lib, name)


def test_4k_resize_branch_over_the_device_route(hip_lib):
    dropin_checks.check_fcn_4k_resize_branch(hip_lib)


def test_soft_outputs_above_25mp_are_refused(hip_lib):
    fc.check_soft_above_25mp_is_refused(hip_lib)
