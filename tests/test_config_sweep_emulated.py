"""CPU: steps 02-03 under non-default configuration values on the emulated library, and what the sweep's streams exercise
(from the oracle alone)."""
import pytest

import config_sweep_checks as csc


def test_sweep_stream_not_vacuous(oracle_built):
    csc.check_sweep_stream_not_vacuous()


def test_step02_stream_not_vacuous(oracle_built):
    csc.check_step02_stream_not_vacuous()


def test_min_pixels_stream_not_vacuous(oracle_built):
    csc.check_min_pixels_stream_not_vacuous()


@pytest.mark.parametrize("axis", [name for name, _ in csc.axis_points()])
def test_step03_axis(emu_lib, oracle_built, axis):
    csc.check_sweep_axis(emu_lib, axis)


@pytest.mark.parametrize("axis", [name for name, _ in csc.axis_points() if name.startswith(("img_threshold", "mixed"))])
def test_step03_axis_without_frames(emu_lib, oracle_built, axis):
    csc.check_sweep_axis(emu_lib, axis, reconstruct=False)


def test_step03_two_runs_alive(emu_lib, oracle_built):
    csc.check_two_runs_alive(emu_lib)


@pytest.mark.parametrize("max_gap", csc.STEP02_GAPS)
@pytest.mark.parametrize("thresholds", csc.STEP02_THRESHOLDS)
def test_step02_thresholds(emu_lib, oracle_built, thresholds, max_gap):
    csc.check_step02(emu_lib, thresholds, max_gap)


@pytest.mark.parametrize("by_setter", [False, True])
@pytest.mark.parametrize("min_pixels", csc.MIN_PIXELS)
def test_min_pixels(emu_lib, oracle_built, min_pixels, by_setter):
    csc.check_min_pixels(emu_lib, min_pixels, by_setter)


def test_dropin_parameter_sets(emu_lib, oracle_built):
    csc.check_dropin_parameter_sets(emu_lib)


def test_huge_img_threshold(emu_lib, oracle_built):
    csc.check_huge_img_threshold(emu_lib)


def test_nan_thresholds_rejected(emu_lib):
    csc.check_nan_rejected(emu_lib)
