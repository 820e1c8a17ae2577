"""GPU: steps 02-03 under non-default configuration values against the oracle (tests/config_sweep_checks.py; what the streams
exercise is asserted from the oracle alone in tests/test_config_sweep_emulated.py)."""
import pytest

import config_sweep_checks as csc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("axis", [name for name, _ in csc.axis_points()])
def test_step03_axis(hip_lib, oracle_built, axis):
    csc.check_sweep_axis(hip_lib, axis)


@pytest.mark.parametrize("axis", [name for name, _ in csc.axis_points() if name.startswith(("img_threshold", "mixed"))])
def test_step03_axis_without_frames(hip_lib, oracle_built, axis):
    csc.check_sweep_axis(hip_lib, axis, reconstruct=False)


def test_step03_two_runs_alive(hip_lib, oracle_built):
    csc.check_two_runs_alive(hip_lib)


@pytest.mark.parametrize("max_gap", csc.STEP02_GAPS)
@pytest.mark.parametrize("thresholds", csc.STEP02_THRESHOLDS)
def test_step02_thresholds(hip_lib, oracle_built, thresholds, max_gap):
    csc.check_step02(hip_lib, thresholds, max_gap)


@pytest.mark.parametrize("by_setter", [False, True])
@pytest.mark.parametrize("min_pixels", csc.MIN_PIXELS)
def test_min_pixels(hip_lib, oracle_built, min_pixels, by_setter):
    csc.check_min_pixels(hip_lib, min_pixels, by_setter)


def test_dropin_parameter_sets(hip_lib, oracle_built):
    csc.check_dropin_parameter_sets(hip_lib)


def test_huge_img_threshold(hip_lib, oracle_built):
    """The emulated twin of this test passes first: lm_group_run maps these values on the host, no kernel receives them."""
    csc.check_huge_img_threshold(hip_lib)


def test_nan_thresholds_rejected(hip_lib):
    csc.check_nan_rejected(hip_lib)
